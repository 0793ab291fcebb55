"""PPO baseline on the GPU: the HIP kernels of pql_amd/csrc/ppo.hip and AgentPPO against plain-torch restatements of the
reference's equations (pql/algo/ppo.py, pql/models/mlp.py:43-75) run on the same device."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn
from torch.distributions import Independent, Normal

import detdata as dd
from ppo_cases import _gae_torch
from support import T, dev  # noqa: F401

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _ppo_cfg(extra=()):
    from pql_amd.utils.cfg import load_cfg
    return load_cfg(["algo=ppo_algo", "task.name=Toy", "num_envs=16", "device=cuda:0", *extra])


# ---------------------------------------------------------------------------------------------------- GAE
def _gae_hip(rew, dones, values, nv, nd, gamma, lam, gae, timeout):
    from pql_amd import _lib as L
    Tn, n = rew.shape
    adv, ret = torch.empty_like(rew), torch.empty_like(rew)
    tmo = timeout.to(torch.float32).contiguous() if timeout is not None else None
    L.check(L.lib.pqlk_gae(L.ptr(rew), L.ptr(dones), L.ptr(values), L.ptr(nv), L.ptr(nd), L.ptr(tmo), Tn, n, gamma, lam, int(gae),
                           L.ptr(adv), L.ptr(ret), L.stream(rew.device)))
    return adv, ret


@pytest.mark.parametrize("Tn,n", [(5, 37), (16, 16384), (8, 4096), (40, 300)])
@pytest.mark.parametrize("gae", [True, False])
@pytest.mark.parametrize("with_timeout", [False, True])
def test_gae_bit_exact_against_the_reference_loop(dev, Tn, n, gae, with_timeout):
    rew = T(dd.uniform((Tn, n), 11, -2, 2)).to(dev)
    dones = T(dd.bernoulli((Tn, n), 12, 0.15)).to(dev)
    values = T(dd.uniform((Tn, n), 13, -3, 3)).to(dev)
    nv = T(dd.uniform((n,), 14, -3, 3)).to(dev)
    nd = T(dd.bernoulli((n,), 15, 0.2)).to(dev)
    timeout = T(dd.bernoulli((Tn, n), 16, 0.1)).to(dev).bool() if with_timeout else None
    want = _gae_torch(rew, dones, values, nv, nd, 0.99, 0.95, gae, timeout)
    got = _gae_hip(rew, dones, values, nv, nd, 0.99, 0.95, gae, timeout)
    for g, w in zip(got, want):
        assert torch.equal(g, w), (g - w).abs().max().item()


# ---------------------------------------------------------------------------------------------------- Gaussian head
@pytest.mark.parametrize("O,A", [(8, 2), (88, 16)])
def test_gaussian_head_and_module_methods(dev, O, A):
    from pql_amd.models.mlp import DiagGaussianMLPPolicy
    pol = DiagGaussianMLPPolicy((O,), A, init_log_std=0.0).to(dev)
    st = {k: T(v) for k, v in dd.mlp_state(O, A, 31).items()}
    st["logstd"] = T(dd.uniform((A,), 32, -1.0, 0.5))
    pol.load_state_dict(st)
    B = 77
    x = T(dd.uniform((B, O), 33, -2, 2)).to(dev)
    eps = T(dd.uniform((B, A), 34, -2, 2)).to(dev)
    # torch restatement of mlp.py:43-75 on the same weights
    net = nn.Sequential(nn.Linear(O, 512), nn.ELU(), nn.Linear(512, 256), nn.ELU(), nn.Linear(256, 128), nn.ELU(), nn.Linear(128, A)).to(dev)
    net.load_state_dict({k[4:]: v for k, v in st.items() if k.startswith("net.")})
    logstd = nn.Parameter(st["logstd"].clone().to(dev))
    mean = net(x)
    dist = Independent(Normal(loc=mean, scale=torch.exp(logstd.expand_as(mean))), 1)
    act_t = mean + eps * torch.exp(logstd)
    lp_t, ent_t = dist.log_prob(act_t), dist.entropy()
    act, lp, ent = pol.sample(x, eps, want_entropy=True)
    np.testing.assert_allclose(act.cpu().numpy(), act_t.detach().cpu().numpy(), rtol=2e-5, atol=2e-6)
    np.testing.assert_allclose(lp.cpu().numpy(), lp_t.detach().cpu().numpy(), rtol=2e-5, atol=2e-5)
    np.testing.assert_allclose(ent.cpu().numpy(), ent_t.detach().cpu().numpy(), rtol=2e-5, atol=2e-5)
    m_act, _, _ = pol.sample(x, None)
    np.testing.assert_allclose(m_act.cpu().numpy(), mean.detach().cpu().numpy(), rtol=2e-5, atol=2e-6)
    # module methods: autograd through the fused MLP and the flat buffer's logstd block
    _, _, lp_m, ent_m = pol.logprob_entropy(x, act_t.detach())
    w = T(dd.uniform((B,), 35)).to(dev)
    loss_m = (lp_m * w).mean() + 0.3 * ent_m.mean()
    loss_t = (dist.log_prob(act_t.detach()) * w).mean() + 0.3 * ent_t.mean()
    loss_m.backward()
    loss_t.backward()
    np.testing.assert_allclose(loss_m.item(), loss_t.item(), rtol=2e-5)
    g_ls = pol.logstd_block(pol.arena.grad)[:A]
    np.testing.assert_allclose(g_ls.cpu().numpy(), logstd.grad.cpu().numpy(), rtol=1e-4, atol=1e-6)
    assert torch.count_nonzero(pol.logstd_block(pol.arena.grad)[A:]) == 0
    g_w = pol.layout.weight(pol.arena.grad, 0, 3)
    np.testing.assert_allclose(g_w.cpu().numpy(), net[6].weight.grad.cpu().numpy(), rtol=1e-4, atol=1e-6)
    a2, d2, lp2, e2 = pol.get_actions_logprob_entropy(x, sample=False)
    np.testing.assert_allclose(a2.detach().cpu().numpy(), mean.detach().cpu().numpy(), rtol=2e-5, atol=2e-6)
    assert tuple(lp2.shape) == (B,) and tuple(e2.shape) == (B,)


# ---------------------------------------------------------------------------------------------------- gather + heads
def _trajectory(rows, O, A, seed, dev):
    return (T(dd.uniform((rows, O), seed, -3, 3)).to(dev), T(dd.uniform((rows, A), seed + 1, -2, 2)).to(dev),
            T(dd.uniform((rows,), seed + 2, -5, -1)).to(dev), T(dd.uniform((rows,), seed + 3, -2, 3)).to(dev),
            T(dd.uniform((rows,), seed + 4, -2, 2)).to(dev), T(dd.uniform((rows,), seed + 5, -2, 2)).to(dev))


def _gather(data, idx, mean, var, eps, dev):
    from pql_amd import _lib as L
    b_obs, b_act, b_logp, b_adv, b_ret, b_val = data
    mb, O, A = idx.numel(), b_obs.shape[1], b_act.shape[1]
    ldx = L.ld(O)
    x = torch.full((mb, ldx), 7.0, device=dev)
    act = torch.empty((mb, A), device=dev)
    outs = [torch.empty(mb, device=dev) for _ in range(4)]
    part = torch.empty(3 * int(L.lib.pqlk_ppo_gather_parts(mb)), device=dev)
    L.check(L.lib.pqlk_ppo_gather(L.ptr(idx), mb, b_obs.shape[0], L.ptr(b_obs), O, L.ptr(mean), L.ptr(var), float(eps), L.ptr(x), ldx,
                                  L.ptr(b_act), A, L.ptr(act), L.ptr(b_logp), L.ptr(b_adv), L.ptr(b_ret), L.ptr(b_val),
                                  *[L.ptr(o) for o in outs], L.ptr(part), L.stream(dev)))
    return x, act, outs, part


@pytest.mark.parametrize("rows,mb", [(4096 * 16, 32768), (1000, 1000 % 384)])
def test_gather_is_bit_equal_to_torch_indexing(dev, rows, mb):
    O, A = 88, 16
    data = _trajectory(rows, O, A, 200, dev)
    perm = torch.from_numpy(np.random.RandomState(3).permutation(rows)).to(dev)
    idx = perm[rows - mb:]   # a short last minibatch when mb is not the batch size
    mean, var = T(dd.uniform((O,), 210, -0.5, 0.5)).to(dev), T(dd.uniform((O,), 211, 0.5, 2.0)).to(dev)
    x, act, (lp, adv, ret, val), part = _gather(data, idx, mean, var, 1e-4, dev)
    want_x = (data[0][idx] - mean) / torch.sqrt(var + 1e-4)
    assert torch.equal(x[:, :O], want_x)
    assert torch.count_nonzero(x[:, O:]) == 0
    assert torch.equal(act, data[1][idx])
    for got, src in zip((lp, adv, ret, val), data[2:]):
        assert torch.equal(got, src[idx])
    p = part.view(-1, 3).double().cpu()
    assert int(p[:, 0].sum()) == mb
    np.testing.assert_allclose(p[:, 1].sum().item(), data[3][idx].double().sum().item(), rtol=1e-5, atol=1e-3)


def _policy_ref(y, logstd, act, old_logp, adv, clip, lam, logp_kernel):
    """ppo.py:156-175 with autograd; the log-prob takes the kernel's values (same graph) so the ratio ties are the kernel's."""
    mean = y.clone().requires_grad_(True)
    ls = logstd.clone().requires_grad_(True)
    dist = Independent(Normal(loc=mean, scale=torch.exp(ls.expand_as(mean))), 1)
    lp = dist.log_prob(act)
    lp = lp + (logp_kernel - lp).detach()
    ratio = (lp - old_logp).exp()
    na = (adv - adv.mean()) / (adv.std() + 1e-8)
    loss = torch.max(-na * ratio, -na * torch.clamp(ratio, 1 - clip, 1 + clip)).mean() - lam * dist.entropy().mean()
    loss.backward()
    return loss.item(), mean.grad, ls.grad, ratio.detach()


def _policy_hip(y, logstd, act, old_logp, adv, part, clip, lam, dev):
    from pql_amd import _lib as L
    B, A = act.shape
    ld = L.ld(A)
    yp = torch.zeros((B, ld), device=dev); yp[:, :A] = y
    dy = torch.zeros((B, ld), device=dev)
    dls = torch.zeros(A, device=dev)
    logp = torch.empty(B, device=dev)
    sc = torch.empty(int(L.lib.pqlk_ppo_scratch_floats(B, A)), device=dev)
    ring = torch.zeros(3, device=dev)
    slot = torch.full((1,), 4, dtype=torch.int32, device=dev)
    L.check(L.lib.pqlk_ppo_policy_loss(L.ptr(yp), ld, L.ptr(logstd), L.ptr(act), L.ptr(old_logp), L.ptr(adv), L.ptr(part), part.numel() // 3,
                                       B, A, float(clip), float(lam), L.ptr(dy), L.ptr(dls), L.ptr(logp), L.ptr(sc), sc.numel(), L.ptr(ring),
                                       L.ptr(slot), 3, L.stream(dev)))
    return ring[1].item(), dy, dls, logp


@pytest.mark.parametrize("A", [1, 16, 21])
@pytest.mark.parametrize("clip,lam", [(0.2, 0.0), (0.2, 0.01), (0.0, 0.0)])
def test_policy_head_matches_autograd(dev, A, clip, lam):
    B, O = 32768, 4
    data = _trajectory(B, O, A, 300 + A, dev)
    idx = torch.arange(B, device=dev)
    _, act, (_, adv, _, _), part = _gather(data, idx, None, None, 0.0, dev)
    y = T(dd.uniform((B, A), 320, -1, 1)).to(dev)
    logstd = T(dd.uniform((A,), 321, -1.0, 0.3)).to(dev)
    # kernel log-probs first, then old log-probs that put the ratio in range, on both clipped sides and exactly at 1 (= 1 +- 0 clip)
    _, _, _, logp0 = _policy_hip(y, logstd, act, torch.zeros(B, device=dev), adv, part, clip, lam, dev)
    shift = torch.tensor([0.0, 0.05, -0.05, 0.5, -0.5, 0.0, 1.0, -1.0], device=dev)[torch.arange(B, device=dev) % 8]
    old = logp0 - shift
    l_h, dy_h, dls_h, logp_h = _policy_hip(y, logstd, act, old, adv, part, clip, lam, dev)
    assert torch.equal(logp_h, logp0)
    l_r, dmu_r, dls_r, ratio = _policy_ref(y, logstd, act, old, adv, clip, lam, logp_h)
    assert bool((ratio == 1).any()) and bool((ratio > 1 + clip).any()) and bool((ratio < 1 - clip).any())
    np.testing.assert_allclose(l_h, l_r, rtol=2e-5, atol=1e-7)
    sc = dmu_r.abs().max().item()
    np.testing.assert_allclose(dy_h[:, :A].cpu().numpy(), dmu_r.cpu().numpy(), rtol=2e-5, atol=2e-5 * sc)
    assert torch.count_nonzero(dy_h[:, A:]) == 0
    np.testing.assert_allclose(dls_h.cpu().numpy(), dls_r.cpu().numpy(), rtol=2e-5, atol=2e-5 * dls_r.abs().max().item())
    again = _policy_hip(y, logstd, act, old, adv, part, clip, lam, dev)
    assert again[0] == l_h and torch.equal(again[1], dy_h) and torch.equal(again[2], dls_h)


@pytest.mark.parametrize("value_clip", [True, False])
def test_value_head_matches_autograd(dev, value_clip):
    from pql_amd import _lib as L
    B, clip = 32768, 0.2
    v = T(dd.uniform((B,), 400, -2, 2)).to(dev)
    R = T(dd.uniform((B,), 401, -2, 2)).to(dev)
    V = v - torch.tensor([0.0, 0.1, -0.1, 0.5, -0.5, 0.2, -0.2, 1.0], device=dev)[torch.arange(B, device=dev) % 8]
    R[::16] = V[::16]   # (v - R)^2 == (V + clamp(v - V) - R)^2 ties where v - V is inside the clip
    vv = v.clone().requires_grad_(True)
    if value_clip:
        lu = (vv - R) ** 2
        lc = (V + torch.clamp(vv - V, -clip, clip) - R) ** 2
        loss = 0.5 * torch.max(lu, lc).mean()
    else:
        loss = 0.5 * ((vv - R) ** 2).mean()
    loss.backward()
    ld = 32
    vp = torch.zeros((B, ld), device=dev); vp[:, 0] = v
    dy = torch.zeros((B, ld), device=dev)
    sc = torch.empty(int(L.lib.pqlk_ppo_scratch_floats(B, 1)), device=dev)
    ring = torch.zeros(2, device=dev)
    for _ in range(2):
        L.check(L.lib.pqlk_ppo_value_loss(L.ptr(vp), ld, L.ptr(R), L.ptr(V), B, int(value_clip), clip, L.ptr(dy), ld, L.ptr(sc), sc.numel(),
                                          L.ptr(ring), None, 2, L.stream(dev)))
        if _ == 0:
            first = (ring[0].item(), dy.clone())
    assert first[0] == ring[0].item() and torch.equal(first[1], dy)
    np.testing.assert_allclose(ring[0].item(), loss.item(), rtol=2e-5)
    np.testing.assert_allclose(dy[:, 0].cpu().numpy(), vv.grad.cpu().numpy(), rtol=2e-5, atol=1e-12)
    assert torch.count_nonzero(dy[:, 1:]) == 0


# ---------------------------------------------------------------------------------------------------- agent
class _RefPPO:
    """Plain-torch restatement of AgentPPO.update_net (ppo.py:141-183) with nn.Linear nets, AdamW and clip_grad_norm_."""

    def __init__(self, O, A, actor_sd, critic_sd, algo, dev):
        def mlp(out):
            return nn.Sequential(nn.Linear(O, 512), nn.ELU(), nn.Linear(512, 256), nn.ELU(), nn.Linear(256, 128), nn.ELU(),
                                 nn.Linear(128, out)).to(dev)
        self.net, self.critic = mlp(A), mlp(1)
        self.net.load_state_dict({k[4:]: v for k, v in actor_sd.items() if k.startswith("net.")})
        self.critic.load_state_dict({k[len("critic.net."):]: v for k, v in critic_sd.items()})
        self.logstd = nn.Parameter(actor_sd["logstd"].clone().to(dev))
        self.algo = algo
        self.aopt = torch.optim.AdamW(list(self.net.parameters()) + [self.logstd], algo.actor_lr)
        self.copt = torch.optim.AdamW(self.critic.parameters(), algo.critic_lr)

    def minibatch(self, obs, act, old, adv, ret, val):
        a = self.algo
        mean = self.net(obs)
        dist = Independent(Normal(loc=mean, scale=torch.exp(self.logstd.expand_as(mean))), 1)
        ratio = (dist.log_prob(act) - old).exp()
        na = (adv - adv.mean()) / (adv.std() + 1e-8)
        al = torch.max(-na * ratio, -na * torch.clamp(ratio, 1 - a.ratio_clip, 1 + a.ratio_clip)).mean()
        nv = self.critic(obs).view(-1)
        if a.value_clip:
            cl = 0.5 * torch.max((nv - ret) ** 2, (val + torch.clamp(nv - val, -a.ratio_clip, a.ratio_clip) - ret) ** 2).mean()
        else:
            cl = 0.5 * ((nv - ret) ** 2).mean()
        al = al - a.lambda_entropy * dist.entropy().mean()
        for opt, loss in ((self.aopt, al), (self.copt, cl)):
            opt.zero_grad(set_to_none=True)
            loss.backward()
            nn.utils.clip_grad_norm_(opt.param_groups[0]["params"], a.max_grad_norm)
            opt.step()
        return al.item(), cl.item()


@pytest.mark.parametrize("value_clip,lam", [(True, 0.0), (False, 0.01)])
def test_update_net_trace_against_torch(dev, value_clip, lam):
    """T*N = 64 rows, batch 24 (a short last minibatch of 16), 2 epochs: per-minibatch losses and the parameters after the update."""
    from pql_amd.algo.ppo import AgentPPO
    from pql_amd.envs.synthetic import create_task_env
    O, A, rows = 8, 2, 64
    cfg = _ppo_cfg(["algo.batch_size=24", "algo.update_times=2", f"algo.value_clip={value_clip}", f"algo.lambda_entropy={lam}"])
    agent = AgentPPO(create_task_env(cfg), cfg)
    asd = {k: T(v) for k, v in dd.mlp_state(O, A, 41).items()}
    asd["logstd"] = T(dd.uniform((A,), 42, -0.7, 0.2))
    csd = {k: T(v) for k, v in dd.mlp_state(O, 1, 43, prefix="critic.net.").items()}
    agent.actor.load_state_dict(asd)
    agent.critic.load_state_dict(csd)
    mean, var = T(dd.uniform((O,), 44, -0.5, 0.5)).to(dev), T(dd.uniform((O,), 45, 0.5, 2.0)).to(dev)
    agent.obs_rms.mean, agent.obs_rms.var = mean.clone(), var.clone()
    data = _trajectory(rows, O, A, 500, dev)
    ref = _RefPPO(O, A, asd, csd, cfg.algo, dev)
    # log-probs near the current policy's, so the ratios straddle the clip range
    with torch.no_grad():
        x = (data[0] - mean) / torch.sqrt(var + 1e-4)
        m = ref.net(x)
        lp = Independent(Normal(m, torch.exp(ref.logstd.expand_as(m))), 1).log_prob(data[1])
        data = (data[0], data[1], lp + T(dd.uniform((rows,), 510, -0.3, 0.3)).to(dev), *data[3:])
    perms = [np.random.RandomState(7 + e).permutation(rows) for e in range(2)]
    info = agent.update_net(data, perms=perms)
    want = []
    for p in perms:
        for s in range(0, rows, 24):
            i = torch.from_numpy(p[s:s + 24]).to(dev)
            want.append(ref.minibatch(((data[0][i] - mean) / torch.sqrt(var + 1e-4)), data[1][i], data[2][i], data[3][i], data[4][i],
                                      data[5][i]))
    got_a, got_c = agent.loss_history()
    want = np.array(want)
    np.testing.assert_allclose(got_a, want[:, 0], rtol=2e-5, atol=1e-6)
    np.testing.assert_allclose(got_c, want[:, 1], rtol=2e-5, atol=1e-6)
    assert abs(info["train/actor_loss"] - want[:, 0].mean()) < 1e-5 and abs(info["train/critic_loss"] - want[:, 1].mean()) < 1e-5
    sd = agent.actor.state_dict()
    np.testing.assert_allclose(sd["logstd"].cpu().numpy(), ref.logstd.detach().cpu().numpy(), rtol=5e-5, atol=5e-7)
    np.testing.assert_allclose(sd["net.6.weight"].cpu().numpy(), ref.net[6].weight.detach().cpu().numpy(), rtol=5e-5, atol=5e-7)
    np.testing.assert_allclose(agent.critic.state_dict()["critic.net.6.weight"].cpu().numpy(),
                               ref.critic[6].weight.detach().cpu().numpy(), rtol=5e-5, atol=5e-7)


@pytest.mark.parametrize("value_norm", [False, True])
def test_explore_env_against_torch(dev, value_norm):
    """5 env steps x 37 envs with injected draws, then compute_adv: the 6-tuple against a torch restatement of ppo.py:30-139."""
    from pql_amd.algo.ppo import AgentPPO
    from pql_amd.envs.synthetic import create_task_env
    O, A, n, Tn = 8, 2, 37, 5
    cfg = _ppo_cfg([f"num_envs={n}", f"algo.value_norm={value_norm}", "task.episode_length=4"])
    env, env_r = create_task_env(cfg), create_task_env(cfg)
    agent = AgentPPO(env, cfg)
    asd = {k: T(v) for k, v in dd.mlp_state(O, A, 51).items()}
    asd["logstd"] = T(dd.uniform((A,), 52, -0.7, 0.2))
    csd = {k: T(v) for k, v in dd.mlp_state(O, 1, 53, prefix="critic.net.").items()}
    agent.actor.load_state_dict(asd)
    agent.critic.load_state_dict(csd)
    ref = _RefPPO(O, A, asd, csd, cfg.algo, dev)
    draws = T(dd.uniform((Tn, n, A), 54, -2, 2)).to(dev)
    agent.reset_agent()
    data, steps = agent.explore_env(env, Tn, draws=draws)
    assert steps == Tn * n

    class RMS:   # torch_util.py:68-103
        def __init__(self, shape):
            self.mean, self.var, self.count = torch.zeros(shape, device=dev), torch.ones(shape, device=dev), 1e-4

        def update(self, x):
            bm, bv, bc = x.mean(dim=0), x.var(dim=0), x.shape[0]
            d, tot = bm - self.mean, self.count + bc
            m2 = self.var * self.count + bv * bc + d ** 2 * self.count * bc / tot
            self.mean, self.var, self.count = self.mean + d * bc / tot, m2 / tot, tot

        def norm(self, x):
            return (x - self.mean) / torch.sqrt(self.var + 1e-4)

    orms, vrms = RMS((O,)), RMS((1,))
    ob, dones = env_r.reset(), torch.zeros(n, device=dev)
    tr = {k: [] for k in ("obs", "act", "logp", "rew", "done", "val", "tmo")}
    with torch.no_grad():
        for t in range(Tn):
            orms.update(ob)
            x = orms.norm(ob)
            m = ref.net(x)
            act = m + draws[t] * torch.exp(ref.logstd)
            lp = Independent(Normal(m, torch.exp(ref.logstd.expand_as(m))), 1).log_prob(act)
            v = ref.critic(x)
            if value_norm:
                vrms.update(v)
                v = v * torch.sqrt(vrms.var + 1e-4) + vrms.mean
            nob, rew, done, info = env_r.step(act)
            for k, val in zip(tr, (ob, act, lp, rew, dones, v.flatten(), info["TimeLimit.truncated"])):
                tr[k].append(val.clone())
            ob, dones = nob, done.float()
        nv = ref.critic(orms.norm(ob))
        if value_norm:
            vrms.update(nv)
            nv = nv * torch.sqrt(vrms.var + 1e-4) + vrms.mean
        S = {k: torch.stack(v) for k, v in tr.items()}
        adv, ret = _gae_torch(S["rew"], S["done"], S["val"], nv.flatten(), dones, 0.99, 0.95, True, S["tmo"])
        b_ret, b_val = ret.reshape(-1), S["val"].reshape(-1)
        if value_norm:
            vrms.update(b_ret); b_ret = (b_ret - vrms.mean) / torch.sqrt(vrms.var + 1e-4)
            vrms.update(b_val); b_val = (b_val - vrms.mean) / torch.sqrt(vrms.var + 1e-4)
    want = (S["obs"].reshape(-1, O), S["act"].reshape(-1, A), S["logp"].reshape(-1), adv.reshape(-1), b_ret, b_val)
    for name, g, w in zip(("obs", "act", "logp", "adv", "ret", "val"), data, want):
        np.testing.assert_allclose(g.cpu().numpy(), w.cpu().numpy(), rtol=1e-4, atol=1e-4, err_msg=name)
    assert torch.equal(agent.dones, dones)
    # a second call continues from the carried obs / dones and fills the same slabs
    data2, _ = agent.explore_env(env, Tn, draws=draws)
    assert torch.equal(data2[0][:n], ob)


def test_train_baselines_ppo_runs(dev):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "train_baselines.py"), "algo=ppo_algo", "task.name=Toy",
                          "num_envs=64", "max_step=20000"], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-3000:]
    last = out.stdout.strip().splitlines()[-1]
    info = eval(last, {"nan": float("nan"), "inf": float("inf")})   # the script prints its final log dict
    assert info["global_steps"] > 20000
    assert math.isfinite(info["train/critic_loss"]) and math.isfinite(info["train/actor_loss"])
