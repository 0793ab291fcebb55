"""The DroQ critic without a GPU: the numpy model of the mask law (tests/droq_cases.py) against Philox known answers, the law's
constants, what the references of tests/test_droq_kernels_gpu.py guarantee, `DoubleQDropoutLayerNorm` on the CPU (construction,
state_dict, deepcopy), the configuration and every refusal."""
import math
import os
import re
from copy import deepcopy

import numpy as np
import pytest
import torch

import droq_cases as dc
import layernorm_cases as lc
from support import cfg_of as _cfg
from task_cases import load_script

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_NULL, E_SHAPE = 1, 2
DROQ = "algo.cri_class=DoubleQDropoutLayerNorm"


# --------------------------------------------------------------------------- the mask law's model
def test_philox_known_answers():
    """Random123's known answers for philox4x32-10 (kat_vectors: counter, key -> block).  tests/test_droq_kernels_gpu.py ties the same
    model to torch's device generator."""
    hexs = lambda w: " ".join(f"{int(x):08x}" for x in w)  # noqa: E731
    assert hexs(dc.philox4x32_10((0, 0), (0, 0, 0, 0))) == "6627e8d5 e169c58d bc57ac4c 9b00dbd8"
    ones = 0xFFFFFFFF
    assert hexs(dc.philox4x32_10((ones, ones), (ones,) * 4)) == "408f276d 41c83b0e a20bc7c6 6d5451fd"


def test_threshold_and_scale():
    assert dc.threshold(0.0) == 0 and dc.threshold(0.5) == 2 ** 31
    assert dc.threshold(0.01) == math.floor(float(np.float32(0.01)) * 2.0 ** 32) == 42949672
    assert dc.scale(0.0) == np.float32(1.0) and dc.scale(0.5) == np.float32(2.0)
    assert dc.scale(0.01) == np.float32(1.0) / np.float32(np.float32(1.0) - np.float32(0.01))
    z = lc.generic_inputs(5, 33)[0]
    u, keep = dc.dropped(z, dc.SEED, dc.TAGS[0], 0.0)      # p = 0: thr = 0, s = 1: u is z bit for bit
    assert keep.all() and np.array_equal(u.view(np.uint32), z.view(np.uint32))


def test_dropped_share():
    """257 x 513 at p = 0.5: within 5 standard deviations, 5 * sqrt(0.25 / 131841) = 0.0069, of 0.5."""
    for tag in dc.TAGS:
        share = 1.0 - dc.keep_mask(dc.SEED, tag, 0.5, 257, 513).mean()
        assert abs(share - 0.5) <= 5 * math.sqrt(0.25 / (257 * 513)), share
    share = 1.0 - dc.keep_mask(dc.SEED, dc.TAGS[0], 0.01, 257, 513).mean()
    assert abs(share - 0.01) <= 5 * math.sqrt(0.01 * 0.99 / (257 * 513)), share


def test_masks_differ_in_every_tag_field_and_in_the_seed():
    base = dict(call=3, stream=1, net=0, layer=2)
    m0 = dc.keep_mask(dc.SEED, dc.make_tag(**base), 0.5, 5, 130)
    for field, other in (("call", 4), ("stream", 2), ("net", 1), ("layer", 3)):
        m1 = dc.keep_mask(dc.SEED, dc.make_tag(**{**base, field: other}), 0.5, 5, 130)
        assert 0.3 < (m0 != m1).mean() < 0.7, field      # independent fair coins differ in half the places
    assert 0.3 < (m0 != dc.keep_mask(dc.SEED + 1, dc.make_tag(**base), 0.5, 5, 130)).mean() < 0.7
    fields = [dc.make_tag(c, s, n, l) for c in (0, 1, 2 ** 40) for s in range(8) for n in (0, 1) for l in range(16)]
    assert len(set(fields)) == len(fields)              # the layout packs without overlap
    # a row's mask does not depend on how many rows there are, nor a column's on the width: r and c are absolute
    big = dc.keep_mask(dc.SEED, dc.TAGS[1], 0.5, 9, 130)
    assert np.array_equal(big[:4, :65], dc.keep_mask(dc.SEED, dc.TAGS[1], 0.5, 4, 65))


def _misses(got, ref, rtol, atol):
    d = np.abs(np.asarray(got, np.float64) - ref)
    lim = atol + rtol * np.abs(ref)
    return float((d / np.maximum(lim, 1e-300)).max())


def _torch32(case):
    (m, cols), p = case
    (z, gamma, beta, dy), keep, u, ref = dc.drop_case(m, cols, p)
    r32 = dict(lc.torch_reference(u, gamma, beta, dy, dtype=torch.float32))
    r32["dz"] = np.where(keep, r32["dz"] * dc.scale(p), np.float32(0.0))
    return r32, ref


def test_bars_hold_for_torch_fp32_on_every_compared_shape():
    """What the GPU test asks of the kernels, torch's own fp32 CPU `F.elu(F.layer_norm(u))` and its autograd deliver: inside the
    layernorm_cases bars against float64 on every shape of the forward and of the backward comparison."""
    bwd = set(dc.bwd_cases())
    for case in dc.fwd_cases():
        r32, ref = _torch32(case)
        assert _misses(r32["y"], ref["y"], **lc.Y_BAR) <= 1, case
        assert _misses(r32["mean"], ref["mean"], lc.STAT_RTOL, lc.MEAN_ATOL) <= 1, case
        assert _misses(r32["rstd"], ref["rstd"], lc.STAT_RTOL, 0.0) <= 1, case
        if case in bwd:
            for name in ("dz", "dgamma", "dbeta"):
                assert _misses(r32[name], ref[name], lc.BWD_RTOL, lc.bwd_atol(ref[name])) <= 1, (case, name)


def test_the_excluded_backward_shape_is_out_of_reach_of_fp32():
    """The one shape taken out of the backward comparison is one that torch's fp32 autograd misses, by far; nothing else is excluded."""
    assert dc.BWD_EXCLUDED == {(1, 3, 0.5)}
    assert len(dc.bwd_cases()) == len([c for c in dc.fwd_cases() if c[0][1] >= 2]) - 1
    r32, ref = _torch32(((1, 3), 0.5))
    assert int(dc.drop_case(1, 3, 0.5)[1].sum()) == 1                      # one column kept of three
    assert _misses(r32["dz"], ref["dz"], lc.BWD_RTOL, lc.bwd_atol(ref["dz"])) > 100


def test_shape_table():
    assert sorted({c for _, c in dc.SHAPES}) == [1, 3, 33, 64, 65, 128, 129, 130, 257, 513, 1025]
    assert {(m, c) for m in (1, 5, 257) for c in dc.COLS} <= set(dc.SHAPES)
    assert (lc.M_PAST_ROW_BLOCKS, 33) in dc.SHAPES and (lc.M_PAST_CHUNKS, 130) in dc.SHAPES
    assert all(c != 2 for _, c in dc.SHAPES) and {(m, 2) for m in (1, 5, 257)} <= set(dc.MASK_SHAPES)
    assert dc.P == [0.0, 0.01, 0.5]


# --------------------------------------------------------------------------- the entries on the host
def test_exports_declared_and_bound():
    from pql_amd import _lib as L
    text = open(os.path.join(ROOT, "include", "pqlk.h")).read()
    for name in ("pqlk_drop_mask", "pqlk_drop_ln_elu_forward", "pqlk_drop_ln_elu_backward"):
        assert re.search(rf"\b{name}\s*\(", text), name
        assert name in L.PROTOTYPES and hasattr(L.lib, name)
    import ctypes as C
    assert L.PROTOTYPES["pqlk_drop_mask"][1][:3] == [C.c_uint64, C.c_uint64, C.c_float]


def test_host_argument_errors():
    """A bad p (negative, 1, above 1, NaN, Inf), m > 2^32, NULL pointers and bad shapes are refused on the host, before any launch."""
    from pql_amd import _lib as L
    p = L.ptr(torch.zeros(64))      # a valid host address, never dereferenced: every call below stops before its launch
    fwd, bwd, mask = L.lib.pqlk_drop_ln_elu_forward, L.lib.pqlk_drop_ln_elu_backward, L.lib.pqlk_drop_mask
    ok_f = [p, 8, 2, 8, p, p, 1e-5, 0.01, 1, 2, p, p, p, None]           # z ld m cols gamma beta eps p seed tag y mean rstd stream
    ok_b = [p, p, p, 8, 2, 8, p, p, p, 0.01, 1, 2, p, p, p, p, None]     # dy y z ld m cols mean rstd gamma p seed tag dz dgamma dbeta scratch
    ok_m = [1, 2, 0.01, 2, 8, p, 8, None]                                # seed tag p m cols keep ld_keep stream
    for bad in (-0.01, 1.0, 1.5, float("nan"), float("inf"), -float("inf")):
        for fn, ok, i in ((fwd, ok_f, 7), (bwd, ok_b, 9), (mask, ok_m, 2)):
            a = list(ok); a[i] = bad
            assert fn(*a) == E_SHAPE, (fn.__name__, bad)
    for fn, ok, i in ((fwd, ok_f, 2), (bwd, ok_b, 4), (mask, ok_m, 3)):
        a = list(ok); a[i] = 2 ** 32 + 1
        assert fn(*a) == E_SHAPE, fn.__name__
    for i in (0, 4, 5, 10, 11, 12):
        a = list(ok_f); a[i] = None
        assert fwd(*a) == E_NULL, i
    for i in (0, 1, 2, 6, 7, 8, 12, 15):
        a = list(ok_b); a[i] = None
        assert bwd(*a) == E_NULL, i
    for fn, ok, edits in ((fwd, ok_f, ((2, 0), (3, 0), (1, 7))), (bwd, ok_b, ((4, 0), (5, -1), (3, 7))), (mask, ok_m, ((3, 0), (4, 0), (6, 7)))):
        for i, v in edits:
            a = list(ok); a[i] = v
            assert fn(*a) == E_SHAPE, (fn.__name__, i, v)
    a = list(ok_m); a[5] = None
    assert mask(*a) == E_NULL


# --------------------------------------------------------------------------- the module on the CPU
def test_construction_matches_the_layernorm_critic():
    from pql_amd.models.droq import DoubleQDropoutLayerNorm
    from pql_amd.models.layernorm import DoubleQLayerNorm
    torch.manual_seed(1234)
    a = DoubleQLayerNorm((11,), 3, hidden_layers=[64, 33])
    state_a, next_a = torch.get_rng_state(), torch.rand(3)
    torch.manual_seed(1234)
    b = DoubleQDropoutLayerNorm((11,), 3, hidden_layers=[64, 33])
    assert torch.equal(torch.get_rng_state(), state_a) and torch.equal(torch.rand(3), next_a)   # nothing more was drawn
    assert torch.equal(a.arena.data, b.arena.data) and list(a.state_dict()) == list(b.state_dict())
    assert (b.seed, b.drop_calls, b.drop_stream, b.dropout) == (1234, 0, 0, 0.01)
    assert [k for k, _ in b.named_parameters()] == ["arena"] and list(b.named_buffers()) == []
    assert DoubleQDropoutLayerNorm((11,), 3, seed=2 ** 63 + 5).seed == 2 ** 63 + 5


def test_state_dict_loads_across_the_two_classes():
    from pql_amd.models.droq import DoubleQDropoutLayerNorm
    from pql_amd.models.layernorm import DoubleQLayerNorm
    a, b = DoubleQLayerNorm((8,), 2, hidden_layers=[32, 24]), DoubleQDropoutLayerNorm((8,), 2, hidden_layers=[32, 24], dropout=0.5)
    assert not torch.equal(a.arena.data, b.arena.data)
    b.load_state_dict(a.state_dict(), strict=True)
    assert torch.equal(a.arena.data, b.arena.data)
    with torch.no_grad():
        b.arena.mul_(0.5)
    a.load_state_dict(b.state_dict(), strict=True)
    assert torch.equal(a.arena.data, b.arena.data)


def test_deepcopy_bumps_the_stream_and_the_tag_layout():
    from pql_amd.models.droq import MAX_DROP_STREAM, DoubleQDropoutLayerNorm
    q = DoubleQDropoutLayerNorm((8,), 2, hidden_layers=[32], seed=7)
    q.drop_calls = 5
    q._ws[64] = {"dev": "stand-in"}
    t = deepcopy(q)
    assert (t.drop_stream, t.drop_calls, t.seed, t.dropout) == (1, 5, 7, 0.01) and q.drop_stream == 0 and t._ws == {}
    assert torch.equal(t.arena, q.arena) and t.arena.data_ptr() != q.arena.data_ptr()
    assert q.tag(5, 1, 0) == dc.make_tag(5, 0, 1, 0) and t.tag(5, 1, 0) == dc.make_tag(5, 1, 1, 0)
    t.load_drop_state(q.drop_state())
    assert t.drop_state() == {"seed": 7, "drop_calls": 5, "drop_stream": 0}
    c = q
    for _ in range(MAX_DROP_STREAM):
        c = deepcopy(c)
    with pytest.raises(ValueError, match="stream"):
        deepcopy(c)
    with pytest.raises(ValueError, match="hidden layers"):
        DoubleQDropoutLayerNorm((8,), 2, hidden_layers=[4] * 17)
    for bad in (-0.1, 1.0, float("nan"), "0.1", True):
        with pytest.raises(ValueError, match=r"critic_dropout"):
            DoubleQDropoutLayerNorm((8,), 2, hidden_layers=[4], dropout=bad)


# --------------------------------------------------------------------------- configuration and refusals (env = None: nothing allocated)
def _script(name):
    return load_script(f"scripts/{name}.py", name)


def test_droq_algo_composes_to_sac_on_the_dropout_critic():
    from pql_amd.algo.critics import check_critic_class
    from pql_amd.models import model_name_to_path
    algo = _cfg("droq_algo").algo
    assert (algo.name, algo.cri_class, algo.critic_dropout, algo.update_times) == ("SAC", "DoubleQDropoutLayerNorm", 0.01, 20)
    sac = _cfg("sac_algo").algo
    for key in ("act_class", "alpha_lr", "alpha", "eval_freq", "tau", "batch_size", "nstep"):
        assert algo[key] == sac[key], key
    assert "DoubleQDropoutLayerNorm" in model_name_to_path
    assert model_name_to_path.resolve("DoubleQDropoutLayerNorm").__name__ == "DoubleQDropoutLayerNorm"
    for name in ("sac_algo", "ddpg_algo", "pql_algo"):
        assert _cfg(name).algo.critic_dropout == 0.01 and _cfg(name).algo.cri_class != "DoubleQDropoutLayerNorm"
    check_critic_class(_cfg("droq_algo"))
    check_critic_class(_cfg("droq_algo", "algo.critic_dropout=0"))
    check_critic_class(_cfg("sac_algo", DROQ, "algo.per.enabled=True"))
    check_critic_class(_cfg("ddpg_algo", DROQ, "algo.critic_dropout=0.5"))
    text = open(os.path.join(ROOT, "pql_amd", "cfg", "algo", "off_policy.yaml")).read()
    assert re.search(r"#.*critic_dropout", text)


def test_critic_dropout_is_no_part_of_a_checkpoints_structure():
    from pql_amd.utils import checkpoint as CK
    a, b = CK.structure(_cfg("droq_algo"), 8, 2), CK.structure(_cfg("droq_algo", "algo.critic_dropout=0.1"), 8, 2)
    assert a == b and a["algo.cri_class"] == "DoubleQDropoutLayerNorm"
    CK.check_structure(a, b)


@pytest.mark.parametrize("algo", ["droq_algo", "ddpg_algo", "sac_algo"])
def test_distl_refused(algo):
    from pql_amd.algo.ddpg import AgentDDPG
    from pql_amd.algo.sac import AgentSAC
    cfg = _cfg(algo, DROQ, "algo.distl=True")
    with pytest.raises(ValueError, match=r"algo\.distl=True.*DoubleQDropoutLayerNorm"):
        (AgentDDPG if algo == "ddpg_algo" else AgentSAC)(None, cfg)


def test_fused_learners_refuse_the_class():
    from pql_amd.algo.pql_p_learner import PQLPLearner
    from pql_amd.algo.pql_v_learner import PQLVLearner
    cfg = _cfg("pql_algo", DROQ)
    for make in (lambda: PQLVLearner((8,), 2, cfg), lambda: PQLPLearner((8,), 2, cfg), lambda: _script("train_pql").main(cfg)):
        with pytest.raises(ValueError, match=r"algo\.cri_class=DoubleQDropoutLayerNorm cannot run in .*droq_algo.*sac_algo.*ddpg_algo"):
            make()


def test_crossq_and_tqc_refuse_the_class():
    from pql_amd.algo.critics import check_critic_class
    with pytest.raises(ValueError, match=r"algo\.cri_class=DoubleQDropoutLayerNorm cannot run with algo=crossq_algo"):
        check_critic_class(_cfg("crossq_algo", DROQ))
    from pql_amd.algo.crossq import AgentCrossQ
    with pytest.raises(ValueError, match="DoubleQDropoutLayerNorm"):
        AgentCrossQ(None, _cfg("crossq_algo", DROQ))
    with pytest.raises(ValueError, match=r"algo=tqc_algo needs algo\.cri_class=QuantileDoubleQ"):
        check_critic_class(_cfg("tqc_algo", DROQ))


@pytest.mark.parametrize("bad", ["-0.01", "1", "1.5", "nan", "abc"])
def test_critic_dropout_outside_the_unit_interval_refused(bad):
    from pql_amd.algo.sac import AgentSAC
    with pytest.raises(ValueError, match=r"algo\.critic_dropout must be a number in \[0, 1\)"):
        AgentSAC(None, _cfg("droq_algo", f"algo.critic_dropout={bad}"))
    from pql_amd.algo.critics import check_critic_class
    check_critic_class(_cfg("sac_algo", f"algo.critic_dropout={bad}"))    # only this class reads the key
