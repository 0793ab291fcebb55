"""The TQC agent (algo=tqc_algo) without a GPU: the float64 references of tests/tqc_sac_cases.py against torch.autograd on the
literal formulation (shift every pooled atom by alpha logp', stable sort, first M, quantile Huber; the mean over both heads for the
actor), the config and its refusals, the class index, the checkpoint structure, and the C boundary's declarations and argument checks."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import quantile_cases as Q
import tqc_cases as TQ
import tqc_sac_cases as TS
from support import cfg_of as _cfg
from tqc_cases import _tied_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QR = "algo.cri_class=QuantileDoubleQ"
E_NULL, E_SHAPE, E_ALIGN, E_UNSUPPORTED = 1, 2, 4, 5   # include/pqlk.h


# ------------------------------------------------------------------------------------------------ the references vs autograd
@pytest.mark.parametrize("per", [False, True])
@pytest.mark.parametrize("B,N", [(8, 2), (9, 5), (12, 8), (8, 33)])
def test_soft_reference_matches_autograd_of_the_literal_formulation(B, N, per):
    """tests/test_tqc_cpu.py's rows made for the ranking (two values only, all atoms equal, identical nets, a reversed net, done = 1
    with ties) with log-probabilities of both signs and alpha = 0.2; d of {0, 1, N - 1}."""
    case = _tied_case(B, N, 100 + N)
    logp, log_alpha = TS.logp_normal(B, 7 + N), np.log(0.2)
    gamma_n, kappa = 0.97, (1.0 if N != 5 else 0.5)
    drops = sorted({0, 1, N - 1})
    base = TS.soft_base(case["theta"], case["theta_t"], case["rew"], case["done"], logp, log_alpha, gamma_n, kappa, drops, chunk=5)
    raw = TQ.tqc_base(case["theta"], case["theta_t"], case["rew"], case["done"], gamma_n, kappa, drops, chunk=5)
    assert np.array_equal(base["rank"], raw["rank"]) and np.array_equal(base["keep"], raw["keep"])   # ranks: the raw atoms', f18's
    assert (logp > 0).any() and (logp < 0).any() and not np.allclose(base["T"], raw["T"])
    for d in drops:
        ref = TS.soft_ref(base, d, case["w"] if per else None, case["wmax"] if per else None)
        th = torch.tensor(case["theta"], dtype=torch.float64, requires_grad=True)
        tt, rew, done, lp = (torch.tensor(x, dtype=torch.float64) for x in (case["theta_t"], case["rew"], case["done"], logp))
        wh = torch.tensor(case["w"], dtype=torch.float64) / float(case["wmax"][0]) if per else None
        loss, kept, T = TS.soft_torch(th, tt, rew, done, lp, TS.alpha_of(log_alpha), Q.f32(gamma_n), Q.f32(kappa), d, wh)
        (grad,) = torch.autograd.grad(loss, th)
        M = 2 * (N - d)
        want = np.zeros((B, 2 * N), bool)   # the kept set of the counting ranks on the raw atoms = the first M of the sorted shifted atoms
        np.put_along_axis(want, kept.numpy(), True, axis=1)
        assert np.array_equal(ref["keep"], want) and kept.shape == (B, M)
        if d > 0:   # ties across the cut, in the rows made for that
            zs = np.sort(base["z"], axis=1)
            assert (zs[[0, 1, 4], M - 1] == zs[[0, 1, 4], M]).all()
        np.testing.assert_allclose(ref["loss"], float(loss.detach()), rtol=1e-12, atol=0)
        np.testing.assert_allclose(ref["dy"], grad.numpy(), rtol=1e-12, atol=1e-18)
        np.testing.assert_allclose(ref["abs_td"], TQ.tqc_abs_td_torch(th.detach(), T).numpy(), rtol=1e-12, atol=1e-15)
        assert (base["T"][4:6] == base["r"][4:6, None]).all()   # done = 1: every target is r, whatever the shift
        assert ref["keep"].sum(axis=1).tolist() == [M] * B


def test_zero_log_probabilities_give_the_hard_law():
    case = Q.normal_case(7, 6, 3, per=True)
    for log_alpha in (0.0, np.log(0.2), 3.0):
        a = TS.soft_ref_of(case["theta"], case["theta_t"], case["rew"], case["done"], np.zeros(7, np.float32), log_alpha, 0.97, 1.0, 2, case["w"], case["wmax"])
        b = TQ.tqc_ref_of(case["theta"], case["theta_t"], case["rew"], case["done"], 0.97, 1.0, 2, case["w"], case["wmax"])
        assert a["loss"] == b["loss"] and np.array_equal(a["dy"], b["dy"]) and np.array_equal(a["abs_td"], b["abs_td"])


@pytest.mark.parametrize("B,N", [(1, 2), (5, 3), (9, 33), (16, 64)])
def test_mean_actor_reference_matches_autograd(B, N):
    theta = np.random.default_rng(B + N).standard_normal((2, B, N)).astype(np.float32)
    ref = TS.dpg_mean_ref(theta)
    th = torch.tensor(theta, dtype=torch.float64, requires_grad=True)
    loss = TS.dpg_mean_torch(th)
    (grad,) = torch.autograd.grad(loss, th)
    np.testing.assert_allclose(ref["loss"], float(loss.detach()), rtol=1e-12, atol=1e-15)
    np.testing.assert_allclose(ref["dy"], grad.numpy(), rtol=1e-12, atol=0)
    assert not np.isclose(ref["loss"], Q.dpg_quantile_ref(theta)["loss"]) or B * N <= 2   # not the min-of-means law


def test_dyadic_cases_are_exact_in_fp32():
    """What the GPU test relies on, with the shift: targets, terms and every partial sum of the chain in increasing p."""
    for B, N in [(16, 2), (64, 8), (16, 64)]:
        case = TQ.dyadic_case(B, N, 17 * N + B)
        logp = TS.logp_dyadic(B, N)
        base = TS.soft_base(case["theta"], case["theta_t"], case["rew"], case["done"], logp, 0.0, Q.DYADIC_GAMMA, Q.DYADIC_KAPPA, TQ.drops_for(N), terms=True)
        assert Q.survives_fp32(base["s"]) and Q.survives_fp32(base["z"] - base["s"][:, None])
        assert Q.survives_fp32(base["T"]) and Q.survives_fp32(base["u"]) and Q.survives_fp32(base["p"])
        for d in TQ.drops_for(N):
            ref = TS.soft_ref(base, d)
            chain = np.cumsum(base["p"] * ref["keep"][None, :, None, :], axis=3)
            assert Q.survives_fp32(chain) and np.array_equal(chain[..., -1], ref["G"])


# ------------------------------------------------------------------------------------------------ config, refusals, plumbing
def test_config_composes_with_the_papers_values_and_sacs_keys():
    from pql_amd.algo.critics import check_critic_class
    from pql_amd.algo.learner import qr_drop, qr_targets
    cfg, sac = _cfg("tqc_algo"), _cfg("sac_algo")
    a = cfg.algo
    assert (a.name, a.act_class, a.cri_class, a.num_quantiles, a.qr_drop) == ("TQC", "TanhDiagGaussianMLPPolicy", "QuantileDoubleQ", 25, 2)
    for key in ("update_times", "alpha_lr", "alpha", "eval_freq", "batch_size", "nstep", "gamma", "tau", "huber_kappa", "no_tgt_actor"):
        assert a[key] == sac.algo[key], key
    check_critic_class(cfg)
    assert qr_drop(a) == 2 and qr_targets(a, 25) == 46
    for extra in (("algo.num_quantiles=32", "algo.qr_drop=0"), ("algo.num_quantiles=64", "algo.qr_drop=63"), ("algo.alpha=0.2",),
                  ("algo.per.enabled=True",)):
        check_critic_class(_cfg("tqc_algo", *extra))


def test_new_refusals_name_their_keys_and_come_before_anything_is_allocated():
    from pql_amd.algo.tqc import AgentTQC
    for cri in ("DoubleQ", "DoubleQLayerNorm"):
        with pytest.raises(ValueError, match=rf"algo=tqc_algo needs algo\.cri_class=QuantileDoubleQ \(got algo\.cri_class={cri}\)"):
            AgentTQC(env=None, cfg=_cfg("tqc_algo", f"algo.cri_class={cri}"))
    with pytest.raises(ValueError, match=r"algo\.qr_drop=null cannot run with algo=tqc_algo.*non-truncated soft quantile law.*not built"):
        AgentTQC(env=None, cfg=_cfg("tqc_algo", "algo.qr_drop=null"))
    # the quantile critic's own refusals apply as they are
    with pytest.raises(ValueError, match=r"algo\.distl=True is not supported with algo\.cri_class=QuantileDoubleQ"):
        AgentTQC(env=None, cfg=_cfg("tqc_algo", "algo.distl=True"))
    with pytest.raises(ValueError, match=r"algo\.target_dtype=bfloat16 is not supported with algo\.cri_class=QuantileDoubleQ"):
        AgentTQC(env=None, cfg=_cfg("tqc_algo", "+algo.target_dtype=bfloat16"))
    with pytest.raises(ValueError, match=r"algo\.qr_drop must be null or an integer from 0 to algo\.num_quantiles - 1 = 24\b"):
        AgentTQC(env=None, cfg=_cfg("tqc_algo", "algo.qr_drop=25"))
    with pytest.raises(ValueError, match=r"algo\.num_quantiles must be an integer from 2 to 64"):
        AgentTQC(env=None, cfg=_cfg("tqc_algo", "algo.num_quantiles=65"))
    with pytest.raises(ValueError, match=r"algo\.huber_kappa must be > 0"):
        AgentTQC(env=None, cfg=_cfg("tqc_algo", "algo.huber_kappa=0"))
    with pytest.raises(ValueError, match=r"algo\.per\.refresh=run cannot run in algo=TQC"):
        AgentTQC(env=None, cfg=_cfg("tqc_algo", "algo.per.enabled=True", "algo.per.refresh=run"))


def test_sac_keeps_refusing_the_quantile_critic_and_points_at_the_new_algorithm():
    from pql_amd.algo.critics import check_critic_class
    from pql_amd.algo.sac import AgentSAC
    pat = r"algo\.cri_class=QuantileDoubleQ cannot run with algo=sac_algo.*entropy shift.*algo=tqc_algo"
    with pytest.raises(ValueError, match=pat):
        check_critic_class(_cfg("sac_algo", QR))
    with pytest.raises(ValueError, match=pat):
        AgentSAC(env=None, cfg=_cfg("sac_algo", QR))


def test_class_index_resolves_the_agent():
    from pql_amd.algo import alg_name_to_path
    from pql_amd.algo.sac import AgentSAC
    from pql_amd.utils.common import load_class_from_path
    cls = load_class_from_path("AgentTQC", alg_name_to_path["AgentTQC"])
    assert cls.__name__ == "AgentTQC" and issubclass(cls, AgentSAC) and str(alg_name_to_path["AgentTQC"]).endswith("tqc.py")
    assert cls.update_once is AgentSAC.update_once   # SAC's sequence; only the two hooks differ
    assert cls._soft_td_loss is not AgentSAC._soft_td_loss and cls._actor_q_loss is not AgentSAC._actor_q_loss


def test_checkpoint_structure_carries_the_head_width():
    from pql_amd.utils import checkpoint as CK
    s = CK.structure(_cfg("tqc_algo"), 8, 2)
    assert s["algo.num_quantiles"] == 25 and s["algo.cri_class"] == "QuantileDoubleQ" and s["algo.act_class"] == "TanhDiagGaussianMLPPolicy"
    assert CK.structure(_cfg("tqc_algo", "algo.num_quantiles=32"), 8, 2)["algo.num_quantiles"] == 32
    assert CK.structure(_cfg("tqc_algo", "algo.qr_drop=5"), 8, 2) == s   # a hyper-parameter, as in f18
    with pytest.raises(ValueError, match=r"algo\.num_quantiles"):
        CK.check_structure(s, CK.structure(_cfg("tqc_algo", "algo.num_quantiles=32"), 8, 2))


# ------------------------------------------------------------------------------------------------ the C boundary
def test_prototypes_match_the_header():
    from pql_amd import _lib as L
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pqlk.h")).read(), flags=re.S)
    ctype = {"const float*": C.c_void_p, "float*": C.c_void_p, "const int32_t*": C.c_void_p, "int64_t": C.c_int64, "int32_t": C.c_int32,
             "float": C.c_float, "pqlk_stream_t": C.c_void_p}
    for name in ("pqlk_tqc_huber_loss_soft", "pqlk_tqc_huber_loss_soft_per", "pqlk_dpg_loss_quantile_mean"):
        m = re.search(rf"\bint\s+{name}\s*\(([^)]*)\)\s*;", hdr)
        assert m, f"{name} is not declared in include/pqlk.h"
        params = [p.strip().rsplit(" ", 1) for p in m.group(1).replace("\n", " ").split(",")]
        res, args = L.PROTOTYPES[name]
        assert res is C.c_int and args == [ctype[t.strip()] for t, _ in params], name
        assert getattr(L.lib, name).argtypes == args
    names = lambda n: [p.strip().rsplit(" ", 1)[1] for p in re.search(rf"\bint\s+{n}\s*\(([^)]*)\)\s*;", hdr).group(1).split(",")]   # noqa: E731
    # the two new pointers stand in front of drop; the mean entry takes pqlk_dpg_loss_quantile's arguments
    for soft, hard in (("pqlk_tqc_huber_loss_soft", "pqlk_tqc_huber_loss"), ("pqlk_tqc_huber_loss_soft_per", "pqlk_tqc_huber_loss_per")):
        h = names(hard)
        assert names(soft) == h[:-2] + ["logp", "log_alpha"] + h[-2:] and h[-2:] == ["drop", "stream"]
        assert L.PROTOTYPES[soft][1] == L.PROTOTYPES[hard][1][:-2] + [C.c_void_p, C.c_void_p] + L.PROTOTYPES[hard][1][-2:]
    assert names("pqlk_dpg_loss_quantile_mean") == names("pqlk_dpg_loss_quantile")
    assert L.PROTOTYPES["pqlk_dpg_loss_quantile_mean"] == L.PROTOTYPES["pqlk_dpg_loss_quantile"]
    assert L.lib.pqlk_version() == 100


def _soft(L, per=False, **k):
    P = C.c_void_p(4096)   # never dereferenced: every call here fails its checks
    a = dict(theta=P, theta_t=P, ld=32, n=8, rew=P, done=P, g=0.97, kappa=1.0, b=4, dy=P, out=None, slot=None, ring=0, scratch=P,
             w=P, wmax=P, abs_td=P, logp=P, log_alpha=P, drop=2)
    a.update(k)
    head = (a["theta"], a["theta_t"], a["ld"], a["n"], a["rew"], a["done"], a["g"], a["kappa"], a["b"], a["dy"], a["out"], a["slot"], a["ring"],
            a["scratch"])
    if per:
        return L.lib.pqlk_tqc_huber_loss_soft_per(*head, a["w"], a["wmax"], a["abs_td"], a["logp"], a["log_alpha"], a["drop"], None)
    return L.lib.pqlk_tqc_huber_loss_soft(*head, a["logp"], a["log_alpha"], a["drop"], None)


@pytest.mark.parametrize("per", [False, True])
def test_soft_entries_refuse_bad_arguments_before_any_launch(per):
    """Every error of the entries is returned before a launch, so it shows without a device."""
    from pql_amd import _lib as L
    for name in ("theta", "theta_t", "rew", "done", "dy", "scratch", "logp", "log_alpha") + (("w", "wmax", "abs_td") if per else ()):
        assert _soft(L, per, **{name: None}) == E_NULL, name
    for bad in (dict(b=0), dict(b=-3), dict(kappa=0.0), dict(kappa=-1.0), dict(slot=C.c_void_p(4096), ring=0)):
        assert _soft(L, per, **bad) == E_SHAPE, bad
    for bad in (dict(n=1, drop=0), dict(n=0, drop=0), dict(n=65, ld=96), dict(n=65, ld=96, drop=64)):
        assert _soft(L, per, **bad) == E_UNSUPPORTED, bad
    for bad in (dict(drop=-1), dict(drop=8), dict(drop=9), dict(n=2, drop=2), dict(n=64, ld=64, drop=64)):
        assert _soft(L, per, **bad) == E_SHAPE, bad
    for bad in (dict(ld=48), dict(ld=0), dict(n=33, ld=32, drop=0)):
        assert _soft(L, per, **bad) == E_ALIGN, bad


def test_mean_actor_entry_refuses_bad_arguments_before_any_launch():
    from pql_amd import _lib as L
    P = C.c_void_p(4096)

    def call(**k):
        a = dict(theta=P, ld=32, n=8, b=4, dy=P, out=None, slot=None, ring=0, scratch=P)
        a.update(k)
        return L.lib.pqlk_dpg_loss_quantile_mean(a["theta"], a["ld"], a["n"], a["b"], a["dy"], a["out"], a["slot"], a["ring"], a["scratch"], None)

    for name in ("theta", "dy", "scratch"):
        assert call(**{name: None}) == E_NULL, name
    for bad in (dict(b=0), dict(b=-1), dict(slot=P, ring=0)):
        assert call(**bad) == E_SHAPE, bad
    for bad in (dict(n=1), dict(n=0), dict(n=65, ld=96)):
        assert call(**bad) == E_UNSUPPORTED, bad
    for bad in (dict(ld=48), dict(ld=0), dict(n=33, ld=32)):
        assert call(**bad) == E_ALIGN, bad
