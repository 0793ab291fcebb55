"""The residual LayerNorm critic without a GPU: the two exports and their host argument errors, `DoubleQBroNet`'s construction, keys,
parameter count and state_dict against the torch twin, the configuration keys, every refusal, and the checkpoint structure."""
import os
import re

import pytest
import torch

import bronet_cases as bc
from support import cfg_of as _cfg
from task_cases import load_script

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_NULL, E_SHAPE = 1, 2
BRO = "algo.cri_class=DoubleQBroNet"


# --------------------------------------------------------------------------- the two exports
def test_header_parses_and_both_prototypes_are_bound():
    import ctypes as C
    from pql_amd import _lib as L
    text = open(os.path.join(ROOT, "include", "pqlk.h")).read()
    for name, n_args in (("pqlk_ln_res_forward", 12), ("pqlk_ln_sum_backward", 16)):
        assert re.search(rf"\b{name}\s*\(", text), name
        assert name in L.PROTOTYPES and hasattr(L.lib, name)
        res, args = L.PROTOTYPES[name]
        assert res is C.c_int and len(args) == n_args
    assert L.parse_header(text)[2].keys() == L.PROTOTYPES.keys()
    assert L.lib.pqlk_version() == 100


def test_host_argument_errors():
    """NULL required pointers, m <= 0, cols <= 0, ld < cols are refused on the host, before any launch (so this runs without a GPU);
    the optional pointers may be NULL."""
    from pql_amd import _lib as L
    p = L.ptr(torch.zeros(64))      # a valid host address: never dereferenced, a refused call launches nothing
    fwd, bwd = L.lib.pqlk_ln_res_forward, L.lib.pqlk_ln_sum_backward
    ok_f = [p, 8, 2, 8, p, p, 1e-5, p, p, p, p, None]          # z ld m cols gamma beta eps res y mean rstd stream
    for i in (0, 4, 5, 7, 8, 9, 10):
        a = list(ok_f); a[i] = None
        assert fwd(*a) == E_NULL, i
    for i, v in ((2, 0), (2, -1), (3, 0), (3, -4), (1, 7)):
        a = list(ok_f); a[i] = v
        assert fwd(*a) == E_SHAPE, (i, v)
    # dy dy2 y z ld m cols mean rstd gamma dsum dz dgamma dbeta scratch stream
    ok_b = [p, p, p, p, 8, 2, 8, p, p, p, p, p, p, p, p, None]
    for i in (0, 3, 7, 8, 9, 11):
        a = list(ok_b); a[i] = None
        assert bwd(*a) == E_NULL, i
    a = list(ok_b); a[14] = None
    assert bwd(*a) == E_NULL                                   # parameter gradients wanted, no scratch
    for i, v in ((5, 0), (5, -1), (6, 0), (6, -4), (4, 7)):
        for optional in ((), (1, 2, 10), (12, 13, 14), (1, 2, 10, 12, 13, 14)):   # the shape is checked whatever is left out
            a = list(ok_b); a[i] = v
            for j in optional:
                a[j] = None
            assert bwd(*a) == E_SHAPE, (i, v, optional)


# --------------------------------------------------------------------------- the class
def test_class_is_in_the_plugin_table():
    from pql_amd.models import model_name_to_path
    assert "DoubleQBroNet" in model_name_to_path
    assert model_name_to_path.resolve("DoubleQBroNet").__name__ == "DoubleQBroNet"


@pytest.mark.parametrize("O,A,W,K", [(8, 2, 64, 2), (8, 2, 130, 1), (11, 3, 40, 0), (88, 16, 512, 2)])
def test_construction_count_and_state_dict_against_the_twin(O, A, W, K):
    from pql_amd.models.bronet import DoubleQBroNet
    q = DoubleQBroNet((O,), A, width=W, blocks=K)
    twin = bc.Twin(O + A, W, K)
    assert list(q.named_buffers()) == [] and [k for k, _ in q.named_parameters()] == ["arena"]
    assert q.dims == [O + A, *[W] * (2 * K + 1), 1] and q.n_layers == 2 * K + 2
    sd = q.state_dict()
    assert list(sd.keys()) == list(twin.state_dict().keys())
    assert [tuple(v.shape) for v in sd.values()] == [tuple(v.shape) for v in twin.state_dict().values()]
    twin.load_state_dict(sd, strict=True)
    assert q.num_params() == bc.num_params(O + A, W, K) == sum(p.numel() for p in twin.parameters())
    # fresh norms are (1, 0), Linears inside the nn.Linear bound; the pad entries of the arena are zero
    for k, v in sd.items():
        if re.search(r"(stem\.1|blocks\.\d+\.[14])\.weight$", k):
            assert bool((v == 1).all()), k
        elif re.search(r"(stem\.1|blocks\.\d+\.[14])\.bias$", k):
            assert bool((v == 0).all()), k
        else:
            fan_in = O + A if ".stem.0." in k else W
            assert float(v.abs().max()) <= fan_in ** -0.5 and float(v.abs().max()) > 0, k
    assert int((q.arena.data != 0).sum()) <= q.num_params() < q.arena.numel()
    st = bc.twin_state(O + A, W, K, 5)
    q.load_state_dict(st, strict=True)
    back = q.state_dict()
    assert all(torch.equal(back[k], v) for k, v in st.items())
    missing = dict(st); del missing["net_q2.out.bias"]
    with pytest.raises(RuntimeError, match="net_q2.out.bias"):
        q.load_state_dict(missing, strict=True)
    again = DoubleQBroNet(**q.init_kwargs)
    again.load_state_dict(back)
    assert torch.equal(again.arena.data, q.arena.data)


def test_fixed_draw_order_and_the_zero_block_tie():
    """Parameters are drawn from the CPU generator net by net, layer by layer, W then b: with K = 0 the class has
    `DoubleQLayerNorm(hidden_layers=[W])`'s arena, bit for bit, from the same seed."""
    from pql_amd.models.bronet import DoubleQBroNet
    from pql_amd.models.layernorm import DoubleQLayerNorm
    torch.manual_seed(3)
    a = DoubleQBroNet((8,), 2, width=130, blocks=0)
    torch.manual_seed(3)
    b = DoubleQLayerNorm((8,), 2, hidden_layers=[130])
    assert torch.equal(a.arena.data, b.arena.data) and a.off == b.off
    torch.manual_seed(3)
    c = DoubleQBroNet((8,), 2, width=64, blocks=2)
    torch.manual_seed(3)
    d = DoubleQLayerNorm((8,), 2, hidden_layers=[64] * 5)
    assert torch.equal(c.arena.data, d.arena.data)
    g = torch.Generator().manual_seed(3)
    w0 = torch.empty(64, 10).uniform_(-(10 ** -0.5), 10 ** -0.5, generator=g)
    torch.manual_seed(3)
    assert torch.equal(DoubleQBroNet((8,), 2, width=64, blocks=2).state_dict()["net_q1.stem.0.weight"], w0)


def test_deepcopy_gets_its_own_empty_workspace():
    from copy import deepcopy
    from pql_amd.models.bronet import DoubleQBroNet
    q = DoubleQBroNet((8,), 2, width=32, blocks=1)
    q._ws[64] = {"dev": "stand-in"}
    t = deepcopy(q)
    assert t._ws == {} and q._ws != {} and torch.equal(t.arena, q.arena) and t.arena.data_ptr() != q.arena.data_ptr()
    assert (t.width, t.blocks) == (32, 1)


# --------------------------------------------------------------------------- configuration and refusals (env = None: nothing allocated)
def _script(name):
    return load_script(f"scripts/{name}.py", name)


def test_config_keys_defaults_and_the_factory(monkeypatch):
    import contextlib
    monkeypatch.setattr(torch.cuda, "device", lambda d: contextlib.nullcontext())   # (make_critic selects the device; none here)
    from pql_amd.algo.critics import check_critic_class, make_critic
    for name in ("ddpg_algo", "sac_algo", "pql_algo"):
        algo = _cfg(name).algo
        assert (algo.critic_width, algo.critic_blocks, algo.cri_class) == (512, 2, "DoubleQ")
    for name in ("ddpg_algo", "sac_algo"):
        text = open(os.path.join(ROOT, "pql_amd", "cfg", "algo", f"{name}.yaml")).read()
        assert re.search(r"#.*cri_class.*DoubleQBroNet", text), name
    text = open(os.path.join(ROOT, "pql_amd", "cfg", "algo", "off_policy.yaml")).read()
    assert re.search(r"#.*critic_width", text) and re.search(r"#.*critic_blocks", text)
    check_critic_class(_cfg("ddpg_algo", BRO))
    check_critic_class(_cfg("sac_algo", BRO, "algo.per.enabled=True"))
    check_critic_class(_cfg("ddpg_algo", BRO, "algo.critic_blocks=0", "algo.critic_width=1"))
    check_critic_class(_cfg("ddpg_algo", BRO, "algo.critic_blocks=16"))
    cfg = _cfg("ddpg_algo", BRO, "algo.critic_width=48", "algo.critic_blocks=3")
    cfg.algo.hidden_layers = [64, 64]
    critic = make_critic(cfg, (8,), 2, torch.device("cpu"))
    assert type(critic).__name__ == "DoubleQBroNet" and (critic.width, critic.blocks) == (48, 3) and critic.dims == [10, *[48] * 7, 1]
    default = make_critic(_cfg("sac_algo", BRO), (8,), 2, torch.device("cpu"))
    assert (default.width, default.blocks) == (512, 2)


@pytest.mark.parametrize("algo", ["ddpg_algo", "sac_algo"])
def test_distl_refused(algo):
    from pql_amd.algo.ddpg import AgentDDPG
    from pql_amd.algo.sac import AgentSAC
    with pytest.raises(ValueError, match=r"algo\.distl=True.*algo\.cri_class=DoubleQBroNet"):
        (AgentDDPG if algo == "ddpg_algo" else AgentSAC)(None, _cfg(algo, BRO, "algo.distl=True"))


def test_fused_learners_refuse_the_class():
    from pql_amd.algo.pql_p_learner import PQLPLearner
    from pql_amd.algo.pql_v_learner import PQLVLearner
    cfg = _cfg("pql_algo", BRO)
    for make in (lambda: PQLVLearner((8,), 2, cfg), lambda: PQLPLearner((8,), 2, cfg), lambda: _script("train_pql").main(cfg)):
        with pytest.raises(ValueError, match=r"algo\.cri_class=DoubleQBroNet cannot run in .*ddpg_algo.*sac_algo"):
            make()


def test_crossq_tqc_and_qr_drop_refuse_the_class():
    from pql_amd.algo.crossq import AgentCrossQ
    from pql_amd.algo.critics import check_critic_class
    with pytest.raises(ValueError, match=r"algo\.cri_class=DoubleQBroNet cannot run with algo=crossq_algo"):
        check_critic_class(_cfg("crossq_algo", BRO))
    with pytest.raises(ValueError, match=r"algo\.cri_class.*DoubleQBroNet"):
        AgentCrossQ(None, _cfg("crossq_algo", BRO))
    with pytest.raises(ValueError, match=r"algo=tqc_algo needs algo\.cri_class=QuantileDoubleQ \(got algo\.cri_class=DoubleQBroNet\)"):
        check_critic_class(_cfg("tqc_algo", BRO))
    with pytest.raises(ValueError, match=r"algo\.qr_drop=2 needs algo\.cri_class=QuantileDoubleQ \(got algo\.cri_class=DoubleQBroNet\)"):
        check_critic_class(_cfg("ddpg_algo", BRO, "algo.qr_drop=2"))


@pytest.mark.parametrize("bad", ["0", "-4", "2.5", "abc", "null"])
def test_critic_width_refused(bad):
    from pql_amd.algo.ddpg import AgentDDPG
    from pql_amd.models.bronet import DoubleQBroNet
    with pytest.raises(ValueError, match=r"algo\.critic_width must be an integer >= 1"):
        AgentDDPG(None, _cfg("ddpg_algo", BRO, f"algo.critic_width={bad}"))
    for v in (0, -4, 2.5, "abc", None, True):
        with pytest.raises(ValueError, match=r"algo\.critic_width"):
            DoubleQBroNet((8,), 2, width=v, blocks=1)


@pytest.mark.parametrize("bad", ["-1", "17", "1.5", "abc", "null"])
def test_critic_blocks_refused(bad):
    from pql_amd.algo.sac import AgentSAC
    from pql_amd.models.bronet import DoubleQBroNet
    with pytest.raises(ValueError, match=r"algo\.critic_blocks must be an integer from 0 to 16"):
        AgentSAC(None, _cfg("sac_algo", BRO, f"algo.critic_blocks={bad}"))
    for v in (-1, 17, 1.5, "abc", None, True):
        with pytest.raises(ValueError, match=r"algo\.critic_blocks"):
            DoubleQBroNet((8,), 2, width=8, blocks=v)


def test_other_classes_do_not_read_the_keys():
    from pql_amd.algo.critics import check_critic_class
    check_critic_class(_cfg("ddpg_algo", "algo.critic_width=0", "algo.critic_blocks=99"))
    check_critic_class(_cfg("sac_algo", "algo.cri_class=DoubleQLayerNorm", "algo.critic_width=-1"))


# --------------------------------------------------------------------------- checkpoint structure
def test_checkpoint_structure_carries_width_and_blocks():
    from pql_amd.utils import checkpoint as CK
    for extra in ((), ("algo.cri_class=DoubleQLayerNorm",), ("algo.critic_width=64",)):
        plain = CK.structure(_cfg("ddpg_algo", *extra), 8, 2)
        assert (plain["algo.critic_width"], plain["algo.critic_blocks"]) == (0, 0)
    plain = CK.structure(_cfg("ddpg_algo"), 8, 2)
    saved = CK.structure(_cfg("ddpg_algo", BRO, "algo.critic_width=64"), 8, 2)
    assert (saved["algo.cri_class"], saved["algo.critic_width"], saved["algo.critic_blocks"]) == ("DoubleQBroNet", 64, 2)
    CK.check_structure(saved, CK.structure(_cfg("ddpg_algo", BRO, "algo.critic_width=64"), 8, 2))
    with pytest.raises(ValueError, match=r"resume: algo\.critic_width=512 but the checkpoint was written with algo\.critic_width=64"):
        CK.check_structure(saved, CK.structure(_cfg("ddpg_algo", BRO), 8, 2))
    with pytest.raises(ValueError, match=r"resume: algo\.critic_blocks=3 but the checkpoint was written with algo\.critic_blocks=2"):
        CK.check_structure(saved, CK.structure(_cfg("ddpg_algo", BRO, "algo.critic_width=64", "algo.critic_blocks=3"), 8, 2))
    old = {k: v for k, v in plain.items() if k not in ("algo.critic_width", "algo.critic_blocks")}   # from before the keys existed
    CK.check_structure(old, plain)
    with pytest.raises(ValueError, match=r"resume: algo\.(cri_class|critic_width|critic_blocks)="):
        CK.check_structure(old, CK.structure(_cfg("ddpg_algo", BRO), 8, 2))
