"""The quantile-regression critic without a GPU: the float64 references of tests/quantile_cases.py against torch.autograd on a
literal formulation of the law (include/pqlk.h), the class, the config keys, the refusals and the checkpoint structure."""
import numpy as np
import pytest
import torch

import quantile_cases as Q
from support import cfg_of as _cfg

QR = "algo.cri_class=QuantileDoubleQ"


# ------------------------------------------------------------------------------------------------ references vs autograd
def _autograd(case, gamma_n, kappa, per):
    th = torch.tensor(case["theta"], dtype=torch.float64, requires_grad=True)
    wh = torch.tensor(case["w"], dtype=torch.float64) / float(case["wmax"][0]) if per else None
    loss = Q.qr_huber_torch(th, torch.tensor(case["theta_t"], dtype=torch.float64), torch.tensor(case["rew"], dtype=torch.float64),
                            torch.tensor(case["done"], dtype=torch.float64), Q.f32(gamma_n), Q.f32(kappa), wh)
    return float(loss.detach()), torch.autograd.grad(loss, th)[0].numpy()


@pytest.mark.parametrize("per", [False, True])
@pytest.mark.parametrize("B,N,kappa", [(5, 2, 1.0), (7, 3, 0.5), (9, 33, 1.0), (4, 64, 2.0)])
def test_huber_reference_is_the_gradient_of_its_loss(B, N, kappa, per):
    case = Q.normal_case(B, N, 100 + N, per=True)
    assert case["done"].max() == 1.0 or B < 6   # rows with done = 1 are among them
    case["done"][0] = 1.0
    ref = Q.qr_huber_ref(case["theta"], case["theta_t"], case["rew"], case["done"], 0.97, kappa,
                         *((case["w"], case["wmax"]) if per else ()))
    loss, grad = _autograd(case, 0.97, kappa, per)
    np.testing.assert_allclose(ref["loss"], loss, rtol=1e-12, atol=0)
    np.testing.assert_allclose(ref["dy"], grad, rtol=1e-12, atol=1e-15)
    # a terminal row's targets are the reward, whatever the target heads hold
    assert (ref["T"][0] == np.float64(case["rew"][0])).all()


def test_huber_reference_takes_net_0_on_an_exact_tie_of_the_sums():
    case = Q.dyadic_case(16, 8, 3)
    ref = Q.qr_huber_ref(case["theta"], case["theta_t"], case["rew"], case["done"], Q.DYADIC_GAMMA, Q.DYADIC_KAPPA)
    assert (ref["S"][0, :4] == ref["S"][1, :4]).all() and (ref["istar"][:4] == 0).all()
    assert (ref["S"][1, 4:8] == ref["S"][0, 4:8] - 2.0 ** -4).all() and (ref["istar"][4:8] == 1).all()
    loss, grad = _autograd(case, Q.DYADIC_GAMMA, Q.DYADIC_KAPPA, False)
    np.testing.assert_allclose(ref["loss"], loss, rtol=1e-12)
    np.testing.assert_allclose(ref["dy"], grad, rtol=1e-12, atol=1e-15)
    other = Q.qr_huber_ref(case["theta"], case["theta_t"], case["rew"], case["done"], Q.DYADIC_GAMMA, Q.DYADIC_KAPPA,
                           force_net=1 - ref["istar"])
    for row in range(8):   # the choice shows in these rows' gradients
        assert (other["dy"][:, row] != ref["dy"][:, row]).any(), row


def test_dpg_reference_against_autograd_with_an_exact_tie():
    case = Q.dyadic_case(16, 8, 4)
    ref = Q.dpg_quantile_ref(case["theta"])
    assert (ref["Q"][0, 8:12] == ref["Q"][1, 8:12]).all() and (ref["share"][:, 8:12] == 0.5).all()
    assert (ref["share"][1, 12:16] == 1.0).all() and (ref["share"][0, 12:16] == 0.0).all()
    for theta in (case["theta"], Q.normal_case(11, 33, 5)["theta"]):
        ref = Q.dpg_quantile_ref(theta)
        th = torch.tensor(theta, dtype=torch.float64, requires_grad=True)
        loss = Q.dpg_quantile_torch(th)
        np.testing.assert_allclose(ref["loss"], float(loss.detach()), rtol=1e-12)
        np.testing.assert_allclose(ref["dy"], torch.autograd.grad(loss, th)[0].numpy(), rtol=1e-12, atol=1e-18)


def test_bounds_are_small_and_the_exact_case_is_exact():
    """The kernel tests' inputs: the dyadic reference survives fp32 (every k term, every partial sum, the result), and the bounds of
    the general case are a few roundings wide, not a tolerance in disguise."""
    case = Q.dyadic_case(16, 64, 7)
    ref = Q.qr_huber_ref(case["theta"], case["theta_t"], case["rew"], case["done"], Q.DYADIC_GAMMA, Q.DYADIC_KAPPA)
    assert Q.survives_fp32(ref["T"]) and Q.survives_fp32(ref["p"]) and Q.survives_fp32(np.cumsum(ref["p"], axis=3)) and Q.survives_fp32(ref["dy"])
    case = Q.normal_case(257, 32, 8)
    assert Q.margins_hold(case["theta"]) and Q.margins_hold(case["theta_t"])
    ref = Q.qr_huber_ref(case["theta"], case["theta_t"], case["rew"], case["done"], 0.97, 1.0)
    dy_b, loss_b, td_b = Q.qr_bounds(ref, 65)
    assert dy_b.max() < 1e-6 * np.abs(ref["dy"]).max() * 32 and loss_b < 1e-5 and td_b.max() < 1e-5
    assert Q.loss_chain(257, 32, 65) == 32 + 1 + 1 + 8 + 1 + 8


# ------------------------------------------------------------------------------------------------ the class
def test_class_keeps_doubleq_keys_and_rebuilds_from_plain_kwargs():
    from pql_amd.models import model_name_to_path
    from pql_amd.models.mlp import DistributionalDoubleQ, DoubleQ, QuantileDoubleQ
    from pql_amd.utils.common import load_class_from_path
    found = load_class_from_path("QuantileDoubleQ", model_name_to_path["QuantileDoubleQ"])   # (the plugin table loads its own copy)
    assert found.__name__ == "QuantileDoubleQ" and found.head == "quantile"
    assert (DoubleQ.head, DistributionalDoubleQ.head, QuantileDoubleQ.head) == ("scalar", "categorical", "quantile")
    q = QuantileDoubleQ((8,), 2, num_quantiles=33, hidden_layers=[64, 64])
    assert q.num_quantiles == 33 and q.num_atoms == 1 and q.layout.dims == [10, 64, 64, 33]
    plain = DoubleQ((8,), 2, hidden_layers=[64, 64], out_dim=33)
    sd = q.state_dict()
    assert list(sd) == list(plain.state_dict()) and all(k.startswith(("net_q1.net.", "net_q2.net.")) for k in sd)
    assert QuantileDoubleQ((8,), 2).num_quantiles == 32
    kw = q.init_kwargs
    assert all(isinstance(v, (int, list)) for v in kw.values()) and kw["num_quantiles"] == 33
    again = QuantileDoubleQ(**kw)
    again.load_state_dict(sd)
    assert again.layout.dims == q.layout.dims and again.num_quantiles == 33
    assert all(torch.equal(a, b) for a, b in zip(again.state_dict().values(), sd.values()))


def test_q_min_is_the_min_of_the_means(monkeypatch):
    from pql_amd.models.mlp import QuantileDoubleQ
    q = QuantileDoubleQ((3,), 1, num_quantiles=5, hidden_layers=[32])
    heads = torch.tensor(np.random.default_rng(0).standard_normal((2, 6, 5)), dtype=torch.float32)
    monkeypatch.setattr(q, "_heads", lambda s, a: heads)   # (the forward itself needs the GPU)
    s, a = torch.zeros(6, 3), torch.zeros(6, 1)
    assert torch.equal(q.get_q_min(s, a), torch.min(heads[0].mean(dim=1), heads[1].mean(dim=1)))
    q1, q2 = q.get_q1_q2(s, a)
    assert torch.equal(q1, heads[0]) and torch.equal(q2, heads[1]) and torch.equal(q.get_q1(s, a), heads[0])


@pytest.mark.parametrize("bad", [1, 65, 2.5])
def test_num_quantiles_out_of_range_names_the_key(bad):
    from pql_amd.algo.critics import check_critic_class
    from pql_amd.models.mlp import QuantileDoubleQ, check_num_quantiles
    for make in (lambda: check_num_quantiles(bad), lambda: QuantileDoubleQ((8,), 2, num_quantiles=bad),
                 lambda: check_critic_class(_cfg("pql_algo", QR, f"algo.num_quantiles={bad}"), "PQLVLearner")):
        with pytest.raises(ValueError, match=r"algo\.num_quantiles must be an integer from 2 to 64"):
            make()
    for ok in (2, 64, 32.0):
        check_num_quantiles(ok)


# ------------------------------------------------------------------------------------------------ config, refusals
@pytest.mark.parametrize("algo", ["pql_algo", "ddpg_algo"])
def test_config_keys_and_make_critic(algo, monkeypatch):
    import contextlib
    monkeypatch.setattr(torch.cuda, "device", lambda d: contextlib.nullcontext())   # (make_critic selects the device; none here)
    from pql_amd.algo.critics import make_critic
    from pql_amd.models.mlp import DoubleQ, QuantileDoubleQ
    cfg = _cfg(algo)
    assert cfg.algo.num_quantiles == 32 and cfg.algo.huber_kappa == 1.0 and cfg.algo.cri_class == "DoubleQ"
    assert type(make_critic(cfg, (8,), 2, torch.device("cpu"))).__name__ == DoubleQ.__name__
    cfg = _cfg(algo, QR, "algo.num_quantiles=8")
    cfg.algo.hidden_layers = [64, 64]
    critic = make_critic(cfg, (8,), 2, torch.device("cpu"))
    assert type(critic).__name__ == QuantileDoubleQ.__name__ and critic.head == "quantile" and critic.num_quantiles == 8 and critic.layout.dims == [10, 64, 64, 8]
    assert cfg.algo.cri_class == "QuantileDoubleQ" and not cfg.algo.distl


def test_refusals_name_their_keys():
    from pql_amd.algo.critics import check_critic_class
    with pytest.raises(ValueError, match=r"algo\.distl=True is not supported with algo\.cri_class=QuantileDoubleQ.*drop algo\.distl=True"):
        check_critic_class(_cfg("pql_algo", QR, "algo.distl=True"), "PQLVLearner")
    with pytest.raises(ValueError, match=r"algo\.cri_class=QuantileDoubleQ cannot run with algo=sac_algo.*entropy shift"):
        check_critic_class(_cfg("sac_algo", QR))
    with pytest.raises(ValueError, match=r"algo\.cri_class=QuantileDoubleQ cannot run with algo=crossq_algo.*BatchNorm critic"):
        check_critic_class(_cfg("crossq_algo", QR))
    with pytest.raises(ValueError, match=r"algo\.target_dtype=bfloat16 is not supported with algo\.cri_class=QuantileDoubleQ"):
        check_critic_class(_cfg("pql_algo", QR, "algo.target_dtype=bfloat16"), "PQLVLearner")
    with pytest.raises(ValueError, match=r"algo\.huber_kappa must be > 0"):
        check_critic_class(_cfg("ddpg_algo", QR, "algo.huber_kappa=0"))
    # accepted: the class alone, and with prioritized replay in either home
    check_critic_class(_cfg("ddpg_algo", QR, "algo.per.enabled=True"))
    for name in ("scripts/train_pql.py", "PQLVLearner", "PQLPLearner"):
        check_critic_class(_cfg("pql_algo", QR, "algo.per.enabled=True", "algo.per.refresh=run"), name)


def test_refusals_come_before_anything_is_allocated():
    """The agents and learners raise them from their constructors' first lines: no environment, no device."""
    from pql_amd.algo.pql_p_learner import PQLPLearner
    from pql_amd.algo.pql_v_learner import PQLVLearner
    from pql_amd.algo.sac import AgentSAC
    for make in (PQLVLearner, PQLPLearner):
        with pytest.raises(ValueError, match=r"algo\.distl=True is not supported with algo\.cri_class=QuantileDoubleQ"):
            make((8,), 2, _cfg("pql_algo", QR, "algo.distl=True"))
    with pytest.raises(ValueError, match=r"cannot run with algo=sac_algo"):
        AgentSAC(env=None, cfg=_cfg("sac_algo", QR))


# ------------------------------------------------------------------------------------------------ checkpoint structure
def test_checkpoint_structure_carries_num_quantiles():
    from pql_amd.utils import checkpoint as CK
    plain = CK.structure(_cfg("pql_algo"), 8, 2)
    assert plain["algo.num_quantiles"] == 0
    saved = CK.structure(_cfg("pql_algo", QR, "algo.num_quantiles=16"), 8, 2)
    assert saved["algo.num_quantiles"] == 16 and saved["algo.num_atoms"] == 0
    CK.check_structure(saved, CK.structure(_cfg("pql_algo", QR, "algo.num_quantiles=16"), 8, 2))
    with pytest.raises(ValueError, match=r"resume: algo\.num_quantiles=32 but the checkpoint was written with algo\.num_quantiles=16"):
        CK.check_structure(saved, CK.structure(_cfg("pql_algo", QR), 8, 2))
    old = {k: v for k, v in plain.items() if k != "algo.num_quantiles"}   # a checkpoint from before the key existed
    CK.check_structure(old, plain)
    with pytest.raises(ValueError, match=r"resume: algo\.(cri_class|num_quantiles)="):
        CK.check_structure(old, CK.structure(_cfg("pql_algo", QR), 8, 2))


# ------------------------------------------------------------------------------------------------ the C boundary
E_NULL, E_SHAPE, E_ALIGN, E_UNSUPPORTED = 1, 2, 4, 5   # include/pqlk.h


def _huber(L, per=False, **k):
    import ctypes as C
    P = C.c_void_p(4096)   # never dereferenced: every call here fails its checks
    a = dict(theta=P, theta_t=P, ld=32, n=8, rew=P, done=P, g=0.97, kappa=1.0, b=4, dy=P, out=None, slot=None, ring=0, scratch=P,
             w=P, wmax=P, abs_td=P)
    a.update(k)
    head = (a["theta"], a["theta_t"], a["ld"], a["n"], a["rew"], a["done"], a["g"], a["kappa"], a["b"], a["dy"], a["out"], a["slot"], a["ring"],
            a["scratch"])
    if per:
        return L.lib.pqlk_qr_huber_loss_per(*head, a["w"], a["wmax"], a["abs_td"], None)
    return L.lib.pqlk_qr_huber_loss(*head, None)


def _dpg(L, **k):
    import ctypes as C
    P = C.c_void_p(4096)
    a = dict(theta=P, ld=32, n=8, b=4, dy=P, out=None, slot=None, ring=0, scratch=P)
    a.update(k)
    return L.lib.pqlk_dpg_loss_quantile(a["theta"], a["ld"], a["n"], a["b"], a["dy"], a["out"], a["slot"], a["ring"], a["scratch"], None)


@pytest.mark.parametrize("per", [False, True])
def test_huber_entries_refuse_bad_arguments_before_any_launch(per):
    """Every error of the entries is returned before a launch, so it shows without a device."""
    import ctypes as C
    from pql_amd import _lib as L
    assert L.lib.pqlk_version() == 100 and L.QR_MAX_QUANTILES == 64
    for name in ("theta", "theta_t", "rew", "done", "dy", "scratch") + (("w", "wmax", "abs_td") if per else ()):
        assert _huber(L, per, **{name: None}) == E_NULL, name
    for bad in (dict(b=0), dict(b=-3), dict(kappa=0.0), dict(kappa=-1.0), dict(slot=C.c_void_p(4096), ring=0)):
        assert _huber(L, per, **bad) == E_SHAPE, bad
    for bad in (dict(ld=48), dict(ld=0), dict(ld=32, n=33)):
        assert _huber(L, per, **bad) == E_ALIGN, bad
    for bad in (dict(n=1), dict(n=0), dict(n=65, ld=96)):
        assert _huber(L, per, **bad) == E_UNSUPPORTED, bad


def test_dpg_entry_refuses_bad_arguments_before_any_launch():
    import ctypes as C
    from pql_amd import _lib as L
    for name in ("theta", "dy", "scratch"):
        assert _dpg(L, **{name: None}) == E_NULL, name
    assert _dpg(L, b=0) == E_SHAPE and _dpg(L, slot=C.c_void_p(4096), ring=0) == E_SHAPE
    assert _dpg(L, ld=40) == E_ALIGN and _dpg(L, ld=32, n=33) == E_ALIGN
    assert _dpg(L, n=1) == E_UNSUPPORTED and _dpg(L, n=65, ld=96) == E_UNSUPPORTED
