"""The TQC agent (algo=tqc_algo, pql_amd/algo/tqc.py) on the GPU, (obs, act) = (8, 2), hidden [64, 64], batch 256, at N = 8 with d = 2
and N = 33 with d = 5 (a padded head, an odd pool).

Yardsticks: the CPU torch-autograd agent of tests/tqc_sac_cases.py (the oracle's SACRef with the literal shift-sort-truncate law and
the mean-of-critics actor term) on identical weights, replay rows, injected indices and both eps draws, at the tolerances of
tests/test_learners_gpu.py's SAC comparison against the oracle (losses at rtol 5e-5, the actor's with atol 1e-6; log_alpha at rtol
1e-5; parameters at rtol 1e-5 with atol 1e-5; |TD| at the parameters' bar, as in tests/test_tqc_learners_gpu.py); the entries a step
goes through and the soft entry called directly on the step's own heads; a second agent from the same seed; and the uninterrupted run
for a resumed one (the pattern of tests/test_resume_gpu.py for the baselines).
"""
import os

import numpy as np
import pytest
import torch

import detdata as dd
import tqc_sac_cases as TS
from learner_harness import _compare_nets, _sd
from quantile_cases import A, B, HID, O, _cfg, _fill
from resume_cases import BASELINE_KEYS, BASELINES, TOY, child, same
from support import T, dev  # noqa: F401

pytestmark = pytest.mark.gpu

SETUPS = [(8, 2), (33, 5)]   # (N, d)
PER_STEP = ("algo.per.enabled=True", "algo.per.alpha=0.5", "algo.per.eps=1.0e-3")
CAP, ROWS = 4096, 3000
WATCHED = ("pqlk_sac_entropy_shift", "pqlk_dpg_loss_quantile", "pqlk_dpg_loss", "pqlk_td_mse_loss", "pqlk_td_mse_loss_per", "pqlk_qr_huber_loss",
           "pqlk_qr_huber_loss_per", "pqlk_tqc_huber_loss", "pqlk_tqc_huber_loss_per", "pqlk_tqc_huber_loss_soft", "pqlk_tqc_huber_loss_soft_per",
           "pqlk_dpg_loss_quantile_mean", "pqlk_sac_alpha_terms", "pqlk_sg_head_forward", "pqlk_sg_head_backward")


def _tqc_cfg(N, d, *extra):
    return _cfg(N, f"algo.qr_drop={d}", *extra, algo="tqc_algo", memory=CAP)


def _weights(N):
    return dd.doubleq_state(O, A, N, 21 + N, HID), dd.mlp_state(O, 2 * A, 11, HID)


def _agent(dev, N, d, *extra, per=False, load=True):
    from pql_amd.algo.tqc import AgentTQC
    from pql_amd.envs.synthetic import create_task_env
    from pql_amd.replay.prioritized_replay import PrioritizedReplayBuffer
    from pql_amd.replay.simple_replay import ReplayBuffer
    cfg = _tqc_cfg(N, d, *(PER_STEP if per else ()), *extra)
    agent = AgentTQC(create_task_env(cfg), cfg)
    assert agent.critic.head == "quantile" and agent.critic.num_quantiles == N and agent.actor.layout.dims[-1] == 2 * A
    mean, var = T(dd.uniform((O,), 801, -0.5, 0.5)), T(dd.uniform((O,), 802, 0.5, 2.0))
    if load:
        cst, ast = _weights(N)
        agent.critic.load_state_dict(_sd(cst)); agent.critic_target.arena.data.copy_(agent.critic.arena.data)
        agent.actor.load_state_dict(_sd(ast))
        agent.obs_rms.mean, agent.obs_rms.var = mean.to(dev), var.to(dev)
    data = _fill(ROWS, 77)
    memory = PrioritizedReplayBuffer(CAP, (O,), A, device=dev, alpha=0.5, eps=1.0e-3) if per else ReplayBuffer(CAP, (O,), A, device=dev)
    memory.add_to_buffer(tuple(t.to(dev) for t in data))
    return agent, memory, data, (mean, var, 1e-4)


def _draws(s):
    return T(dd.integers((B,), 40 + s, ROWS)), T(dd.uniform((B, A), 50 + s, -2, 2)), T(dd.uniform((B, A), 60 + s, -2, 2))


# ------------------------------------------------------------------------------------------------ against the autograd agent
@pytest.mark.parametrize("per", [False, True])
@pytest.mark.parametrize("fixed", [None, 0.2])
@pytest.mark.parametrize("N,d", SETUPS)
def test_update_once_vs_autograd(dev, N, d, fixed, per):
    """Three update_once calls on injected indices and both eps draws; learned and fixed temperature, uniform and prioritized
    (refresh=step: the reference takes the importance weights the agent's tree gave the injected rows)."""
    from oracle import pql_ref_cpu as ref
    agent, memory, data, norm = _agent(dev, N, d, *((f"algo.alpha={fixed}",) if fixed else ()), per=per)
    cst, ast = _weights(N)
    orc = TS.make_tqc_sac_ref(O, A, ref.HyperRef(batch_size=B), CAP, ref.params_from_state(ast), ref.params_from_state(cst, "net_q1.net."),
                              ref.params_from_state(cst, "net_q2.net."), d, alpha_lr=agent.cfg.algo.alpha_lr, alpha=fixed)
    orc.ring.insert(*data); orc.norm = norm
    spread = 0
    for s in range(3):
        idx, e1, e2 = _draws(s)
        agent.update_once(memory, indices=idx, eps_next=e1, eps_cur=e2)
        wh = None
        if per:
            w = agent._ws["w"].cpu()
            wh = w / agent._ws["wmax"].cpu()
            spread = max(spread, int(torch.unique(w).numel()))
        cl, al_, _ = orc.update_once(idx, e1, e2, wh)
        print(f"N={N} d={d} alpha={fixed} per={per} step {s}: closs {agent.closs[s % 5].item():.9g} vs {cl:.9g}; aloss {agent.aloss[s % 5].item():.9g} "
              f"vs {al_:.9g}; log_alpha {agent.log_alpha.item():.9g} vs {float(orc.log_alpha.detach()):.9g}")
        np.testing.assert_allclose(agent.closs[s % 5].item(), cl, rtol=5e-5)
        np.testing.assert_allclose(agent.aloss[s % 5].item(), al_, rtol=5e-5, atol=1e-6)
        if fixed is None:
            np.testing.assert_allclose(agent.log_alpha.item(), float(orc.log_alpha.detach()), rtol=1e-5)
        if per:   # |TD| of the step, and the leaves it wrote back: (|TD| + eps)^alpha, the largest candidate of a row drawn twice
            td = orc.abs_td.numpy()
            np.testing.assert_allclose(agent._ws["abs_td"].cpu().numpy(), td, rtol=1e-5, atol=1e-5)
            want = np.zeros(CAP)
            np.maximum.at(want, idx.numpy(), np.sqrt(td.astype(np.float64) + 1.0e-3))
            rows = np.unique(idx.numpy())
            np.testing.assert_allclose(memory.leaves.cpu().numpy()[rows], want[rows], rtol=1e-5, atol=1e-5)
    if fixed is None:
        assert abs(agent.log_alpha.item()) > 1e-3   # the temperature moved
    else:
        assert abs(agent.get_alpha(scalar=True) - fixed) < 1e-7
    assert not per or spread > 10
    _compare_nets(agent.critic, (orc.q1, orc.q2), "critic")
    _compare_nets(agent.critic_target, (orc.t1, orc.t2), "target")
    _compare_nets(agent.actor, (orc.actor,), "actor")


# ------------------------------------------------------------------------------------------------ which launches a step issues
@pytest.fixture
def entries(monkeypatch):
    """Records, in order, which of the watched entries a step goes through, with their arguments."""
    from pql_amd import _lib as L
    seen = []
    for name in WATCHED:
        inner = getattr(L.lib, name)

        def spy(*a, _inner=inner, _name=name):
            seen.append((_name, a))
            return _inner(*a)

        monkeypatch.setattr(L.lib, name, spy)
    return seen


@pytest.mark.parametrize("per", [False, True])
@pytest.mark.parametrize("N,d", SETUPS)
def test_a_step_issues_the_soft_and_the_mean_entry_and_no_shift(dev, entries, N, d, per):
    """No pqlk_sac_entropy_shift and no pqlk_dpg_loss_quantile launch; SAC's other launches in SAC's order.  The dy the critic step
    used and the loss it wrote are the bits of the soft entry called directly on the step's own heads."""
    from pql_amd import _lib as L
    from pql_amd.models.mlp import mlp_forward_raw, output_view
    agent, memory, _, _ = _agent(dev, N, d, per=per)
    kept = {}
    soft = "pqlk_tqc_huber_loss_soft" + ("_per" if per else "")
    inner = getattr(L.lib, soft)   # (the spy of `entries`)

    def keep_dy(*a):   # the critic's dy is overwritten by the actor step: copy it as the loss launch leaves it
        rc = inner(*a)
        kept["dy"] = agent._ws["dy"].clone()
        kept["w"] = None if not per else (agent._ws["w"].clone(), agent._ws["wmax"].clone())
        return rc

    arena0, la0 = agent.critic.arena.data.clone(), agent.log_alpha.clone()   # the critic and log_alpha as the step's loss launch read them
    setattr(L.lib, soft, keep_dy)
    try:
        idx, e1, e2 = _draws(0)
        agent.update_once(memory, indices=idx, eps_next=e1, eps_cur=e2)
        torch.cuda.synchronize(dev)
    finally:
        setattr(L.lib, soft, inner)
    names = [n for n, _ in entries]
    assert names == ["pqlk_sg_head_forward", soft, "pqlk_sg_head_forward", "pqlk_dpg_loss_quantile_mean", "pqlk_sac_alpha_terms",
                     "pqlk_sg_head_backward"], names
    # the soft entry on the heads the step read, into fresh buffers.  The target's stash is as the step left it (no in-place shift);
    # the critic's was overwritten by the actor step's forward, so the pre-step critic is run again on the step's own batch.
    ws, cl = agent._ws, agent.critic.layout
    qt = output_view(cl, ws["acts_t"], B)
    xq = torch.empty_like(ws["acts_c"])
    with torch.cuda.device(dev):
        mlp_forward_raw(cl, arena0, ws["x_sa"], L.ACT_NONE, acts=xq)
        q = output_view(cl, xq, B)
        dy = torch.full_like(ws["dy"], float("nan"))
        ring, step = torch.zeros(5, dtype=torch.float32, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
        scratch, abs_td = torch.empty(1024, dtype=torch.float32, device=dev), torch.zeros(B, dtype=torch.float32, device=dev)
        gamma_n = float(agent.cfg.algo.gamma) ** int(agent.cfg.algo.nstep)
        head = (L.ptr(q), L.ptr(qt), cl.ld_out, N, L.ptr(ws["rew"]), L.ptr(ws["done"]), gamma_n, 1.0, B, L.ptr(dy), L.ptr(ring), L.ptr(step), 5,
                L.ptr(scratch))
        pw = (L.ptr(kept["w"][0]), L.ptr(kept["w"][1]), L.ptr(abs_td)) if per else ()
        L.check(inner(*head, *pw, L.ptr(ws["logp_next"]), L.ptr(la0), d, L.stream(dev)))
        torch.cuda.synchronize(dev)
    assert torch.equal(dy, kept["dy"]) and bool((dy[:, :, N:] == 0).all())
    assert ring[0].item() == agent.closs[0].item() and ring[0].item() > 0
    if per:
        assert torch.equal(abs_td, ws["abs_td"])
    assert bool((ws["logp_next"] != 0).all())   # (the shift was not trivially absent)


def test_sac_keeps_its_own_sequence(dev, entries):
    """The hooks AgentTQC overrides leave AgentSAC on the shift launch, the twin MSE and the min-Q actor loss."""
    from pql_amd.algo.sac import AgentSAC
    from pql_amd.envs.synthetic import create_task_env
    from pql_amd.replay.simple_replay import ReplayBuffer
    from pql_amd.utils.cfg import load_cfg
    cfg = load_cfg(["algo=sac_algo", "task.name=Toy", "num_envs=64", f"algo.batch_size={B}", f"algo.memory_size={CAP}", "device=cuda:0",
                    "sim_device=cuda:0"])
    agent = AgentSAC(create_task_env(cfg), cfg)
    memory = ReplayBuffer(CAP, (O,), A, device=dev)
    memory.add_to_buffer(tuple(t.to(dev) for t in _fill(ROWS, 77)))
    idx, e1, e2 = _draws(0)
    agent.update_once(memory, indices=idx, eps_next=e1, eps_cur=e2)
    torch.cuda.synchronize(dev)
    assert [n for n, _ in entries] == ["pqlk_sg_head_forward", "pqlk_sac_entropy_shift", "pqlk_td_mse_loss", "pqlk_sg_head_forward", "pqlk_dpg_loss",
                                       "pqlk_sac_alpha_terms", "pqlk_sg_head_backward"]


# ------------------------------------------------------------------------------------------------ determinism, resume
@pytest.mark.parametrize("per", [False, True])
def test_two_agents_from_one_seed_give_the_same_bits(dev, per):
    """Three update_net calls (update_times = 2 each) drawing their own indices and eps: arenas, moments, rings, temperature."""
    N, d = SETUPS[1]
    ends = []
    for _ in range(2):
        torch.manual_seed(1234)
        torch.cuda.manual_seed_all(1234)
        agent, memory, _, _ = _agent(dev, N, d, "algo.update_times=2", per=per, load=False)
        for _ in range(3):
            out = agent.update_net(memory)
        torch.cuda.synchronize(dev)
        assert np.isfinite(out["train/critic_loss"]) and np.isfinite(out["train/actor_loss"]) and 0 < out["train/alpha"] != 1.0
        st = {k: v.clone() for k, v in agent._state_tensors().items()}
        if per:
            st["tree"], st["pmax"] = memory.tree.clone(), memory.pmax.clone()
        ends.append(st)
    assert set(ends[0]) == set(ends[1]) and {"log_alpha", "alpha_loss", "alpha_opt.m", "alpha_opt.v", "alpha_opt.step", "critic_target"} <= set(ends[0])
    for k in ends[0]:
        assert torch.equal(ends[0][k], ends[1][k]), k
    assert int(ends[0]["copt.step"]) == 6 and int(ends[0]["alpha_opt.step"]) == 6


def test_resume_is_bit_exact(tmp_path):
    """scripts/train_baselines.py with algo=tqc_algo: 6000 steps uninterrupted == 3000 steps, checkpoint, a fresh process, to 6000."""
    base = TOY + ["algo=tqc_algo", "algo.num_quantiles=8", "algo.qr_drop=2"]
    a = child(BASELINES, base + ["max_step=6000"], tmp_path)
    ck = tmp_path / "ck"
    b1 = child(BASELINES, base + ["max_step=3000", f"checkpoint.dir={ck}"], tmp_path)
    assert b1["actor_sha"] != a["actor_sha"] and sorted(os.listdir(ck / f"step-{b1['global_steps']}")) == ["ring.bin", "state.pt"]
    b2 = child(BASELINES, base + ["max_step=6000", f"resume={ck}"], tmp_path)
    assert b2["resumed_from"]["global_steps"] == b1["global_steps"]
    same(b2["resumed_from"], b1, ("actor_sha", "critic_sha"))
    same(a, b2, BASELINE_KEYS)
    assert np.isfinite(a["train/critic_loss"]) and np.isfinite(a["train/actor_loss"])
