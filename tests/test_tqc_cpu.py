"""The truncated pooled target (algo.qr_drop) without a GPU: the float64 reference of tests/tqc_cases.py against torch.autograd on
the literal formulation (stable sort, first M, quantile Huber), the config key and its refusals, the checkpoint structure, and the C
boundary's declarations and argument checks."""
import ctypes as C

import numpy as np
import pytest
import torch

import quantile_cases as Q
import tqc_cases as TQ
from support import cfg_of as _cfg
from tqc_cases import _tied_case

QR = "algo.cri_class=QuantileDoubleQ"
E_NULL, E_SHAPE, E_ALIGN, E_UNSUPPORTED = 1, 2, 4, 5   # include/pqlk.h


# ------------------------------------------------------------------------------------------------ the reference vs autograd
@pytest.mark.parametrize("per", [False, True])
@pytest.mark.parametrize("B,N", [(8, 2), (9, 5), (12, 8), (8, 33)])
def test_reference_matches_autograd_of_the_literal_formulation(B, N, per):
    case = _tied_case(B, N, 100 + N)
    gamma_n, kappa = 0.97, (1.0 if N != 5 else 0.5)
    drops = sorted({0, 1, N - 1})
    base = TQ.tqc_base(case["theta"], case["theta_t"], case["rew"], case["done"], gamma_n, kappa, drops, chunk=5)
    for d in drops:
        ref = TQ.tqc_ref(base, d, case["w"] if per else None, case["wmax"] if per else None)
        th = torch.tensor(case["theta"], dtype=torch.float64, requires_grad=True)
        tt, rew, done = (torch.tensor(case[k], dtype=torch.float64) for k in ("theta_t", "rew", "done"))
        wh = torch.tensor(case["w"], dtype=torch.float64) / float(case["wmax"][0]) if per else None
        loss, kept, T = TQ.tqc_torch(th, tt, rew, done, Q.f32(gamma_n), Q.f32(kappa), d, wh)
        (grad,) = torch.autograd.grad(loss, th)
        M = 2 * (N - d)
        # the kept set of the counting ranks is the first M of the stable sort, as a set of pool indices
        want = np.zeros((B, 2 * N), bool)
        np.put_along_axis(want, kept.numpy(), True, axis=1)
        assert np.array_equal(ref["keep"], want) and kept.shape == (B, M)
        if d > 0:   # ties across the cut: equal atoms on both sides of it, in the rows made for that
            zs = np.sort(base["z"], axis=1)
            assert (zs[[0, 1, 4], M - 1] == zs[[0, 1, 4], M]).all()
        np.testing.assert_allclose(ref["loss"], float(loss.detach()), rtol=1e-12, atol=0)
        np.testing.assert_allclose(ref["dy"], grad.numpy(), rtol=1e-12, atol=1e-18)
        np.testing.assert_allclose(ref["abs_td"], TQ.tqc_abs_td_torch(th.detach(), T).numpy(), rtol=1e-12, atol=1e-15)
        assert (base["T"][4:6] == base["r"][4:6, None]).all()   # done = 1: every target is r, and the kept set is still M atoms
        assert ref["keep"].sum(axis=1).tolist() == [M] * B


def test_ranks_are_a_permutation_and_ties_go_by_pool_index():
    case = _tied_case(8, 8, 5)
    base = TQ.tqc_base(case["theta"], case["theta_t"], case["rew"], case["done"], 0.97, 1.0, [0])
    assert (np.sort(base["rank"], axis=1) == np.arange(16)[None]).all()
    assert base["rank"][1].tolist() == list(range(16))          # all atoms equal: the pool index decides
    assert (base["rank"][2, 8:] == base["rank"][2, :8] + 1).all()   # identical nets: net 0's copy of a value comes first


def test_drop_zero_is_not_the_law_without_the_key():
    """d = 0 regresses on all atoms of both target nets; the law without the key on one whole net per row."""
    case = Q.normal_case(6, 4, 3)
    a = TQ.tqc_ref_of(case["theta"], case["theta_t"], case["rew"], case["done"], 0.97, 1.0, 0)
    b = Q.qr_huber_ref(case["theta"], case["theta_t"], case["rew"], case["done"], 0.97, 1.0)
    assert a["keep"].all() and not np.allclose(a["dy"], b["dy"]) and abs(a["loss"] - b["loss"]) > 1e-6


def test_dyadic_cases_are_exact_in_fp32():
    """What the GPU test relies on: targets, terms and every partial sum of the chain in increasing p (dropped atoms skipped)."""
    for B, N in [(16, 2), (64, 8), (16, 64)]:
        case = TQ.dyadic_case(B, N, 17 * N + B)
        base = TQ.tqc_base(case["theta"], case["theta_t"], case["rew"], case["done"], Q.DYADIC_GAMMA, Q.DYADIC_KAPPA, TQ.drops_for(N), terms=True)
        assert Q.survives_fp32(base["T"]) and Q.survives_fp32(base["u"]) and Q.survives_fp32(base["p"])
        for d in TQ.drops_for(N):
            ref = TQ.tqc_ref(base, d)
            chain = np.cumsum(base["p"] * ref["keep"][None, :, None, :], axis=3)
            assert Q.survives_fp32(chain) and np.array_equal(chain[..., -1], ref["G"])


# ------------------------------------------------------------------------------------------------ config, refusals
@pytest.mark.parametrize("algo", ["pql_algo", "ddpg_algo"])
def test_key_defaults_to_null_and_accepts_the_range(algo):
    from pql_amd.algo.critics import check_critic_class
    from pql_amd.algo.learner import qr_drop, qr_targets
    cfg = _cfg(algo)
    assert cfg.algo.qr_drop is None and qr_drop(cfg.algo) is None and qr_targets(cfg.algo, 32) == 32
    check_critic_class(cfg)
    check_critic_class(_cfg(algo, QR))
    for n, d in [(32, 0), (32, 2), (32, 31), (2, 1), (64, 63), (8, 2.0)]:
        cfg = _cfg(algo, QR, f"algo.num_quantiles={n}", f"algo.qr_drop={d}")
        check_critic_class(cfg)
        assert qr_drop(cfg.algo) == int(d) and qr_targets(cfg.algo, n) == 2 * (n - int(d))
    where = ("PQLVLearner",) if algo == "pql_algo" else ()
    check_critic_class(_cfg(algo, QR, "algo.qr_drop=2", "algo.per.enabled=True", *(("algo.per.refresh=run",) if where else ())), *where)


@pytest.mark.parametrize("cri", ["DoubleQ", "DoubleQLayerNorm"])
def test_key_with_another_critic_is_refused_naming_both_keys(cri):
    from pql_amd.algo.critics import check_critic_class
    with pytest.raises(ValueError, match=r"algo\.qr_drop=2 needs algo\.cri_class=QuantileDoubleQ"):
        check_critic_class(_cfg("ddpg_algo", f"algo.cri_class={cri}", "algo.qr_drop=2"))
    with pytest.raises(ValueError, match=r"algo\.qr_drop=0 needs algo\.cri_class=QuantileDoubleQ"):
        check_critic_class(_cfg("pql_algo", "algo.qr_drop=0", "algo.distl=True"), "PQLVLearner")


@pytest.mark.parametrize("n,bad", [(32, -1), (32, 32), (8, 8), (8, 2.5), (2, 2), (8, "half")])
def test_key_out_of_range_names_the_key_the_range_and_num_quantiles(n, bad):
    from pql_amd.algo.critics import check_critic_class
    with pytest.raises(ValueError, match=rf"algo\.qr_drop must be null or an integer from 0 to algo\.num_quantiles - 1 = {n - 1}\b"):
        check_critic_class(_cfg("pql_algo", QR, f"algo.num_quantiles={n}", f"algo.qr_drop={bad}"), "PQLVLearner")


def test_refusals_come_before_anything_is_allocated():
    from pql_amd.algo.ddpg import AgentDDPG
    from pql_amd.algo.pql_v_learner import PQLVLearner
    with pytest.raises(ValueError, match=r"algo\.qr_drop must be null or an integer"):
        PQLVLearner((8,), 2, _cfg("pql_algo", QR, "algo.num_quantiles=8", "algo.qr_drop=8"))
    with pytest.raises(ValueError, match=r"algo\.qr_drop=1 needs algo\.cri_class=QuantileDoubleQ"):
        AgentDDPG(env=None, cfg=_cfg("ddpg_algo", "algo.qr_drop=1"))


def test_key_is_not_part_of_the_checkpoint_structure():
    from pql_amd.utils import checkpoint as CK
    null = CK.structure(_cfg("pql_algo", QR, "algo.num_quantiles=16"), 8, 2)
    assert not any("qr_drop" in k for k in null)
    assert CK.structure(_cfg("pql_algo", QR, "algo.num_quantiles=16", "algo.qr_drop=3"), 8, 2) == null
    assert CK.structure(_cfg("pql_algo"), 8, 2)["algo.num_quantiles"] == 0


# ------------------------------------------------------------------------------------------------ the C boundary
def test_prototypes_hold_both_entries_with_drop_before_the_stream():
    from pql_amd import _lib as L
    for name, base in (("pqlk_tqc_huber_loss", "pqlk_qr_huber_loss"), ("pqlk_tqc_huber_loss_per", "pqlk_qr_huber_loss_per")):
        assert name in L.PROTOTYPES
        res, args = L.PROTOTYPES[name]
        bres, bargs = L.PROTOTYPES[base]
        assert res is bres and args == bargs[:-1] + [C.c_int32, bargs[-1]]
        assert getattr(L.lib, name).argtypes == args
    assert L.lib.pqlk_version() == 100


def _tqc(L, per=False, **k):
    P = C.c_void_p(4096)   # never dereferenced: every call here fails its checks
    a = dict(theta=P, theta_t=P, ld=32, n=8, rew=P, done=P, g=0.97, kappa=1.0, b=4, dy=P, out=None, slot=None, ring=0, scratch=P,
             w=P, wmax=P, abs_td=P, drop=2)
    a.update(k)
    head = (a["theta"], a["theta_t"], a["ld"], a["n"], a["rew"], a["done"], a["g"], a["kappa"], a["b"], a["dy"], a["out"], a["slot"], a["ring"],
            a["scratch"])
    if per:
        return L.lib.pqlk_tqc_huber_loss_per(*head, a["w"], a["wmax"], a["abs_td"], a["drop"], None)
    return L.lib.pqlk_tqc_huber_loss(*head, a["drop"], None)


@pytest.mark.parametrize("per", [False, True])
def test_entries_refuse_bad_arguments_before_any_launch(per):
    """Every error of the entries is returned before a launch, so it shows without a device."""
    from pql_amd import _lib as L
    for name in ("theta", "theta_t", "rew", "done", "dy", "scratch") + (("w", "wmax", "abs_td") if per else ()):
        assert _tqc(L, per, **{name: None}) == E_NULL, name
    for bad in (dict(b=0), dict(b=-3), dict(kappa=0.0), dict(kappa=-1.0), dict(slot=C.c_void_p(4096), ring=0)):
        assert _tqc(L, per, **bad) == E_SHAPE, bad
    for bad in (dict(n=1, drop=0), dict(n=0, drop=0), dict(n=65, ld=96), dict(n=65, ld=96, drop=64)):
        assert _tqc(L, per, **bad) == E_UNSUPPORTED, bad
    for bad in (dict(drop=-1), dict(drop=8), dict(drop=9), dict(n=2, drop=2), dict(n=64, ld=64, drop=64)):
        assert _tqc(L, per, **bad) == E_SHAPE, bad
    for bad in (dict(ld=48), dict(ld=0), dict(n=33, ld=32, drop=0)):
        assert _tqc(L, per, **bad) == E_ALIGN, bad
