"""PPO baseline against tests/golden/ppo.npz, generated from the reference's own DiagGaussianMLPPolicy / MLPCritic / AgentPPO on
the CPU (tools/gen_golden.py gen_ppo): GAE bit-exact on the compute_adv traces, the policy's known-answer vectors, compute_adv
end to end over use_gae x value_norm, and a two-epoch update_net trace with a short last minibatch."""
import numpy as np
import pytest
import torch

import detdata as dd
from support import T, dev  # noqa: F401

pytestmark = pytest.mark.gpu
TRACES = [(g, v) for g in (1, 0) for v in (0, 1)]


def _cfg(extra=()):
    from pql_amd.utils.cfg import load_cfg
    return load_cfg(["algo=ppo_algo", "task.name=Toy", "device=cuda:0", *extra])


def _agent(n, extra, actor_seed, critic_seed, logstd, dev):
    from pql_amd.algo.ppo import AgentPPO
    from pql_amd.envs.synthetic import create_task_env
    O, A = 8, 2
    cfg = _cfg([f"num_envs={n}", *extra])
    ag = AgentPPO(create_task_env(cfg), cfg)
    st = {k: T(v) for k, v in dd.mlp_state(O, A, actor_seed).items()}
    st["logstd"] = T(logstd)
    ag.actor.load_state_dict(st)
    ag.critic.load_state_dict({k: T(v) for k, v in dd.mlp_state(O, 1, critic_seed, prefix="critic.net.").items()})
    ag.obs_rms.mean, ag.obs_rms.var = T(dd.uniform((O,), 901, -0.5, 0.5)).to(dev), T(dd.uniform((O,), 902, 0.5, 2.0)).to(dev)
    return ag


def _adv_inputs(dev):
    Tn, N, O = 5, 37, 8
    return dict(obs=T(dd.uniform((Tn, N, O), 84, -3, 3)).to(dev), rew=T(dd.uniform((Tn, N), 85, -2, 2)).to(dev),
                done=T(dd.bernoulli((Tn, N), 86, 0.2)).to(dev), val=T(dd.uniform((Tn, N), 87, -3, 3)).to(dev),
                nobs=T(dd.uniform((N, O), 88, -3, 3)).to(dev), ndone=T(dd.bernoulli((N,), 89, 0.2)).to(dev),
                tmo=T(dd.bernoulli((Tn, N), 90, 0.15)).to(dev))


@pytest.mark.parametrize("gae,vn", TRACES)
def test_gae_bit_exact_on_the_reference_traces(golden, dev, gae, vn):
    """pqlk_gae with the next value the reference's GAE read: advantages (and, without value_norm, returns) bit for bit."""
    from pql_amd import _lib as L
    g, tag = golden("ppo"), f"adv_g{gae}_v{vn}"
    d = _adv_inputs(dev)
    Tn, N = d["rew"].shape
    nv = T(g[f"{tag}_gae_next_value"]).to(dev)
    adv, ret = torch.empty_like(d["rew"]), torch.empty_like(d["rew"])
    L.check(L.lib.pqlk_gae(L.ptr(d["rew"]), L.ptr(d["done"]), L.ptr(d["val"]), L.ptr(nv), L.ptr(d["ndone"]), L.ptr(d["tmo"]), Tn, N, 0.99,
                           0.95, gae, L.ptr(adv), L.ptr(ret), L.stream(dev)))
    assert np.array_equal(adv.reshape(-1).cpu().numpy(), g[f"{tag}_adv"])
    if not vn:
        assert np.array_equal(ret.reshape(-1).cpu().numpy(), g[f"{tag}_ret"])


@pytest.mark.parametrize("gae,vn", TRACES)
def test_compute_adv_against_the_reference_traces(golden, dev, gae, vn):
    """AgentPPO.compute_adv end to end (critic on the next obs through the MFMA MLP, value_rms updates in the reference's order)."""
    g, tag = golden("ppo"), f"adv_g{gae}_v{vn}"
    ag = _agent(37, [f"algo.use_gae={bool(gae)}", f"algo.value_norm={bool(vn)}"], 81, 82, dd.uniform((2,), 83, -0.5, 0.0), dev)
    d = _adv_inputs(dev)
    r = ag._rollout_bufs(5)
    for k in ("obs", "rew", "done", "val"):
        r[k].copy_(d[k])
    b = ag.compute_adv(r, d["nobs"], d["ndone"], gae=bool(gae), timeout=d["tmo"])
    np.testing.assert_array_equal(b[0].cpu().numpy(), d["obs"].reshape(-1, 8).cpu().numpy())
    for k, got in zip(("adv", "ret", "val"), b[3:]):
        np.testing.assert_allclose(got.cpu().numpy(), g[f"{tag}_{k}"], rtol=2e-5, atol=2e-5, err_msg=k)
    if vn:
        m, v, c = g[f"{tag}_vrms"]
        np.testing.assert_allclose([ag.value_rms.mean.item(), ag.value_rms.var.item()], [m, v], rtol=2e-5, atol=1e-6)
        assert abs(ag.value_rms.count - c) < 1e-6


@pytest.mark.parametrize("tag", ["kat_toy", "kat_allegro"])
def test_policy_known_answer_vectors(golden, dev, tag):
    from torch.distributions import Independent, Normal
    from pql_amd.models.mlp import DiagGaussianMLPPolicy
    g = golden("ppo")
    O, A, B = (int(v) for v in g[f"{tag}_meta"])
    pol = DiagGaussianMLPPolicy((O,), A).to(dev)
    st = {k: T(v) for k, v in dd.mlp_state(O, A, 71).items()}
    st["logstd"] = T(dd.uniform((A,), 72, -1.0, 0.5))
    pol.load_state_dict(st)
    x, eps = T(dd.uniform((B, O), 73, -2, 2)).to(dev), T(g[f"{tag}_eps"]).to(dev)
    # the rollout head (HIP)
    act, logp, ent = pol.sample(x, eps, want_entropy=True)
    np.testing.assert_allclose(act.cpu().numpy(), g[f"{tag}_act"], rtol=2e-5, atol=2e-6)
    np.testing.assert_allclose(logp.cpu().numpy(), g[f"{tag}_logp"], rtol=2e-5, atol=2e-5)
    np.testing.assert_allclose(ent.cpu().numpy(), g[f"{tag}_ent"], rtol=2e-5, atol=2e-5)
    # the module's autograd path: rsample = loc + eps * scale with the recorded draw
    mean, dist = pol.get_actions(x, sample=False)
    a = mean + eps * torch.exp(pol.logstd)
    lp, en = dist.log_prob(a), dist.entropy()
    w = T(dd.uniform((B,), 74, -1, 1)).to(dev)
    loss = (lp * w).mean() + 0.3 * en.mean() - (a * a).mean()
    loss.backward()
    np.testing.assert_allclose(loss.item(), float(g[f"{tag}_loss"]), rtol=2e-5, atol=1e-6)
    grad, lay = pol.arena.grad, pol.layout
    for l in range(lay.n_layers):
        for kind, view in (("weight", lay.weight(grad, 0, l)), ("bias", lay.bias(grad, 0, l))):
            got, want = dd.summarize(view.cpu().numpy()), g[f"{tag}_g_net.{2 * l}.{kind}"]
            np.testing.assert_allclose(got[1:], want[1:], rtol=1e-4, atol=1e-6, err_msg=f"net.{2 * l}.{kind}")
    np.testing.assert_allclose(pol.logstd_block(grad)[:A].cpu().numpy(), g[f"{tag}_g_logstd_exact"], rtol=1e-4, atol=1e-6)


def _check(module, g, prefix, rtol=5e-5, atol=5e-7):
    """Parameter fingerprints as in test_learners_gpu._check_module (sum held to an l2-scaled absolute bar)."""
    for key, view in module.named_views():
        got, want = dd.summarize(view.cpu().numpy()), g[f"{prefix}{key}"]
        np.testing.assert_allclose(got[1:], want[1:], rtol=rtol, atol=atol, err_msg=prefix + key)
        np.testing.assert_allclose(got[0], want[0], rtol=rtol, atol=atol + 2e-6 * float(want[1]), err_msg=prefix + key + " (sum)")


@pytest.mark.parametrize("tag,value_clip,lam", [("upd_c1_e0", True, 0.0), ("upd_c0_e1", False, 0.01)])
def test_update_net_golden_trace(golden, dev, tag, value_clip, lam):
    """Two epochs over 64 rows at batch 24 (minibatches 24, 24, 16) with the reference's recorded permutations: losses per minibatch
    and every parameter after every minibatch, then update_net's own loop on a fresh agent gives the same."""
    g = golden("ppo")
    extra = ["algo.batch_size=24", "algo.update_times=2", f"algo.value_clip={value_clip}", f"algo.lambda_entropy={lam}"]
    mk = lambda: _agent(16, extra, 91, 92, dd.uniform((2,), 93, -0.7, 0.2), dev)  # noqa: E731
    ag = mk()
    raw = T(g[f"{tag}_data"]).to(dev)
    data = (raw[:, :8].contiguous(), raw[:, 8:10].contiguous(), *(raw[:, c].contiguous() for c in range(10, 14)))
    perms, want = g[f"{tag}_perms"], g[f"{tag}_losses"]
    plan = ag.minibatch_plan(64)
    k = len(perms) * len(plan)
    ag._loss_rings(k)
    m = 0
    for p in perms:
        idx = T(p).to(dev)
        for s, e in plan:
            ag.update_minibatch(data, idx[s:e], k)
            np.testing.assert_allclose([ag.aloss[m].item(), ag.closs[m].item()], want[m], rtol=2e-5, atol=1e-6, err_msg=f"minibatch {m}")
            _check(ag.actor, g, f"{tag}_m{m}_")
            _check(ag.critic, g, f"{tag}_m{m}_")
            m += 1
    np.testing.assert_allclose(ag.actor.state_dict()["logstd"].cpu().numpy(), g[f"{tag}_final_logstd"], rtol=5e-5, atol=5e-7)
    np.testing.assert_allclose(ag.actor.state_dict()["net.6.weight"].cpu().numpy(), g[f"{tag}_final_actor_last_w"], rtol=5e-5, atol=5e-7)
    np.testing.assert_allclose(ag.critic.state_dict()["critic.net.6.weight"].cpu().numpy(), g[f"{tag}_final_critic_last_w"],
                               rtol=5e-5, atol=5e-7)
    ag2 = mk()
    info = ag2.update_net(data, perms=perms)
    a2, c2 = ag2.loss_history()
    assert np.array_equal(a2, ag.aloss.cpu().numpy()) and np.array_equal(c2, ag.closs.cpu().numpy())
    assert torch.equal(ag2.actor.arena.data, ag.actor.arena.data) and torch.equal(ag2.critic.arena.data, ag.critic.arena.data)
    assert abs(info["train/actor_loss"] - want[:, 0].mean()) < 1e-5 and abs(info["train/critic_loss"] - want[:, 1].mean()) < 1e-5


def test_update_net_draws_the_discarded_rsample(dev):
    """ppo.py:154 draws an (mb, A) rsample per minibatch inside logprob_entropy and discards it: the generator advances by the same."""
    ag = _agent(16, ["algo.batch_size=24", "algo.update_times=2"], 91, 92, dd.uniform((2,), 93, -0.7, 0.2), dev)
    data = (T(dd.uniform((64, 8), 1, -1, 1)).to(dev), T(dd.uniform((64, 2), 2)).to(dev), *(T(dd.uniform((64,), s)).to(dev) for s in (3, 4, 5, 6)))
    torch.manual_seed(5)
    ag.update_net(data, perms=[np.arange(64)] * 2)
    after = torch.randn(8, device=dev)
    torch.manual_seed(5)
    for n in (24, 24, 16, 24, 24, 16):
        torch.empty((n, 2), device=dev).normal_()
    assert torch.equal(after, torch.randn(8, device=dev))


def test_one_row_last_minibatch_gives_nan_like_the_reference(dev):
    """rows % batch_size == 1: the reference's std() of one advantage is NaN and so is that minibatch's actor loss; no error here."""
    ag = _agent(16, ["algo.batch_size=21", "algo.update_times=1"], 91, 92, dd.uniform((2,), 93, -0.7, 0.2), dev)
    data = (T(dd.uniform((64, 8), 1, -1, 1)).to(dev), T(dd.uniform((64, 2), 2)).to(dev), *(T(dd.uniform((64,), s)).to(dev) for s in (3, 4, 5, 6)))
    ag.update_net(data, perms=[np.arange(64)])
    a, c = ag.loss_history()
    assert np.all(np.isfinite(a[:3])) and np.isnan(a[3]) and np.all(np.isfinite(c))
