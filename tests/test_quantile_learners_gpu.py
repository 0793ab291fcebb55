"""The quantile-regression critic in the PQL learners and in DDPG on the GPU (algo.cri_class=QuantileDoubleQ).

Yardsticks: the CPU torch-autograd learners of tests/quantile_cases.py (the oracle's learners with the quantile laws in place of
the twin MSE / min Q) on identical weights, replay rows, injected indices and draws; the learner's own other modes (eager, per-slot
graphs, one run graph); the uninterrupted run for a resumed one; and, for the priorities, the float64 law on the heads the step
itself produced.

Tolerances of the comparisons against the autograd learners are those of tests/test_learners_gpu.py for the same comparison
(`test_full_size_step_vs_oracle`): losses at rtol 1e-5; parameters at rtol 1e-5 with atol 1e-5 = 2 % of one Adam step (lr 5e-4) --
Adam divides by sqrt(v), so an entry whose gradient is ~0 turns a 1e-9 gradient difference (fp32 summation order) into a visible
fraction of lr.
"""
import numpy as np
import pytest
import torch

import detdata as dd
import quantile_cases as Q
from learner_harness import PER, _compare_nets, _same_state, _sd, _state
from quantile_cases import A, B, K, O, _cfg, _fill, _learner, _rows, _run, _weights
from support import T, dev  # noqa: F401

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------ against the autograd learners
@pytest.mark.parametrize("N", [8, 33])   # 33: a padded head (ld 64)
def test_pql_learners_vs_autograd(dev, N):
    """Three V steps and two P steps on injected rows and draws."""
    from oracle import pql_ref_cpu as ref
    from pql_amd.algo.pql_p_learner import PQLPLearner
    from pql_amd.algo.pql_v_learner import PQLVLearner
    cfg, cap, rows = _cfg(N), 4096, 3000
    v, p = PQLVLearner((O,), A, cfg), PQLPLearner((O,), A, cfg)
    assert v.critic.head == "quantile" and v.critic.num_quantiles == N and v.critic.layout.dims[-1] == N
    cst, ast = _weights(N)
    v.critic.load_state_dict(_sd(cst)); v.critic_target.arena.data.copy_(v.critic.arena.data)
    p.actor.load_state_dict(_sd(ast))
    data = _fill(rows, 77)
    mean, var = T(dd.uniform((O,), 801, -0.5, 0.5)), T(dd.uniform((O,), 802, 0.5, 2.0))
    hp = ref.HyperRef(batch_size=B)
    vr = Q.make_v_ref(O, A, hp, cap, ref.params_from_state(cst, "net_q1.net."), ref.params_from_state(cst, "net_q2.net."))
    pr = Q.make_p_ref(O, A, hp, cap, ref.params_from_state(ast))
    vr.update(ref.params_from_state(ast), data, (mean, var, 1e-4))
    pr.update(vr.q1, vr.q2, data[0], (mean, var, 1e-4))
    norm = (mean.to(dev), var.to(dev), 1e-4)
    v.update(p.actor, tuple(t.to(dev) for t in data), norm, 0)
    p.update(v.critic, data[0].to(dev), norm, 0)
    assert p.critic.head == "quantile" and p.critic.num_quantiles == N
    for s in range(3):
        idx, draw = T(dd.integers((B,), 900 + s, rows)), T(dd.uniform((B, A), 950 + s, -2, 2))
        lv = vr.learn(idx=idx, draw=draw)
        v.learn(indices=idx, noise=draw)
        v.synchronize()
        print(f"N={N} V step {s}: loss {v.loss_ring[s % 5].item():.9g} vs {lv:.9g}")
        np.testing.assert_allclose(v.loss_ring[s % 5].item(), lv, rtol=1e-5)
        if s < 2:
            lp = pr.learn(idx=idx)
            p.learn(indices=idx)
            p.synchronize()
            print(f"N={N} P step {s}: loss {p.loss_ring[s % 5].item():.9g} vs {lp:.9g}")
            np.testing.assert_allclose(p.loss_ring[s % 5].item(), lp, rtol=1e-5, atol=1e-7)
    ws = v._ws
    assert ws["td_parts"] == 0 and ws["td_fwd"] == 0 and not p._ws["dpg_fused"] and not p._ws["split_in"]   # the scalar-only fusions are off
    _compare_nets(v.critic, (vr.q1, vr.q2), "critic")
    _compare_nets(v.critic_target, (vr.t1, vr.t2), "target")
    _compare_nets(p.actor, (pr.actor,), "actor")


@pytest.mark.parametrize("per", [False, True])
def test_ddpg_vs_autograd(dev, per):
    """Three inner iterations of update_net (update_once on injected rows and draws), uniform and prioritized.  Prioritized: the
    reference takes the importance weights the agent's tree gave the injected rows; from the second iteration on they differ."""
    from oracle import pql_ref_cpu as ref
    from pql_amd.algo.ddpg import AgentDDPG
    from pql_amd.envs.synthetic import create_task_env
    from pql_amd.replay.prioritized_replay import PrioritizedReplayBuffer
    from pql_amd.replay.simple_replay import ReplayBuffer
    N, cap, rows = 8, 4096, 3000
    cfg = _cfg(N, *(("algo.per.enabled=True", "algo.per.alpha=0.5", "algo.per.eps=1.0e-3") if per else ()), algo="ddpg_algo", memory=cap)
    agent = AgentDDPG(create_task_env(cfg), cfg)
    assert agent.critic.head == "quantile" and agent.critic.num_quantiles == N
    cst, ast = _weights(N)
    agent.critic.load_state_dict(_sd(cst)); agent.critic_target.arena.data.copy_(agent.critic.arena.data)
    agent.actor.load_state_dict(_sd(ast))
    mean, var = T(dd.uniform((O,), 801, -0.5, 0.5)), T(dd.uniform((O,), 802, 0.5, 2.0))
    agent.obs_rms.mean, agent.obs_rms.var = mean.to(dev), var.to(dev)
    data = _fill(rows, 77)
    memory = PrioritizedReplayBuffer(cap, (O,), A, device=dev, alpha=0.5, eps=1.0e-3) if per else ReplayBuffer(cap, (O,), A, device=dev)
    memory.add_to_buffer(tuple(t.to(dev) for t in data))
    orc = Q.make_ddpg_ref(O, A, ref.HyperRef(batch_size=B), cap, ref.params_from_state(ast), ref.params_from_state(cst, "net_q1.net."),
                          ref.params_from_state(cst, "net_q2.net."))
    orc.ring.insert(*data); orc.norm = (mean, var, 1e-4)
    spread = 0
    for s in range(3):
        idx, draw = T(dd.integers((B,), 40 + s, rows)), T(dd.uniform((B, A), 50 + s, -2, 2))
        agent.update_once(memory, indices=idx, noise=draw)
        wh = None
        if per:
            w = agent._ws["w"].cpu()
            wh = w / agent._ws["wmax"].cpu()
            spread = max(spread, int(torch.unique(w).numel()))
        cl, al_ = orc.update_once(idx, draw, wh)
        print(f"per={per} step {s}: closs {agent.closs[s % 5].item():.9g} vs {cl:.9g}; aloss {agent.aloss[s % 5].item():.9g} vs {al_:.9g}")
        np.testing.assert_allclose(agent.closs[s % 5].item(), cl, rtol=1e-5)
        np.testing.assert_allclose(agent.aloss[s % 5].item(), al_, rtol=1e-5, atol=1e-7)
        if per:   # |TD| of the step (fp32 on both sides: the bar of the parameters)
            np.testing.assert_allclose(agent._ws["abs_td"].cpu().numpy(), orc.abs_td.numpy(), rtol=1e-5, atol=1e-5)
    assert not per or spread > 10
    _compare_nets(agent.critic, (orc.q1, orc.q2), "critic")
    _compare_nets(agent.critic_target, (orc.t1, orc.t2), "target")
    _compare_nets(agent.actor, (orc.actor,), "actor")


# ------------------------------------------------------------------------------------------------ modes, resume, priorities
@pytest.mark.parametrize("N,extra", [(8, ()), (33, ()), (8, PER)])
def test_modes_agree(dev, N, extra):
    """Eager learn() x K, per-slot graphs and one run graph: two runs with an `update()` between leave the same arenas, Adam state
    and loss ring -- and, prioritized, the same tree and pmax."""
    ends = {}
    for mode in ("eager", "slots", "run"):
        v, actor, norm = _learner(N, *extra, graph=mode != "eager")
        for rnd in range(2):
            _run(v, mode)
            if rnd == 0:
                v.update(actor, _rows(300, 30, dev), norm, 0)
        assert v.rng == "philox" and v.update_count == 2 * K
        assert (len(v._slot_graphs), v._run_graph is not None) == {"eager": (0, False), "slots": (K, False), "run": (0, True)}[mode]
        ends[mode] = _state(v)
    _same_state(ends["eager"], ends["slots"])
    _same_state(ends["eager"], ends["run"])
    e = ends["eager"]
    assert bool(torch.isfinite(e["loss_ring"]).all()) and bool((e["loss_ring"] > 0).all()) and int(e["adam_step"]) == 2 * K
    assert not torch.equal(e["critic"], e["target"])
    if extra:
        assert e["tree"][:1800].unique().numel() > 100


@pytest.mark.parametrize("extra", [(), PER])
def test_resume_continues_bit_exactly(dev, extra):
    """One run, save, one more run -- against a fresh learner that loads the saved state (and the ring's rows) and takes that run."""
    a, actor, norm = _learner(8, *extra, graph=True)
    _run(a, "run")
    a.synchronize()
    st, rows = a.training_state(), a.memory.rows().clone()
    _run(a, "run")
    b, _, _ = _learner(8, *extra, graph=True, seed=12)   # other weights, other rows, another generator state
    b.load_training_state(st)
    b.memory.rows().copy_(rows)
    _run(b, "run")
    assert a.update_count == b.update_count == 2 * K
    _same_state(_state(a), _state(b))


def test_priorities_are_the_law_applied_to_the_steps_own_heads(dev):
    """A prioritized run, eager: the |TD| slab of the run's last step against the float64 law on the heads, rewards, done flags and
    weights that step itself read (still in the workspace), within the kernel test's bound (quantile_cases.qr_bounds) -- and so is that
    step's dy.  Then the write-back: every sampled row's leaf is (max over its occurrences of |TD| + eps)^0.5 from the slabs, bit for
    bit (alpha = 0.5: sqrtf is correctly rounded)."""
    from pql_amd.models.mlp import output_view
    N = 8
    v, actor, norm = _learner(N, *PER, graph=False)
    _run(v, "eager")   # a first run on the fresh tree (every priority 1, every weight 1); the second samples from its |TD|s
    _run(v, "eager")
    torch.cuda.synchronize()
    assert v._per_pending == K
    ws, cl = v._ws, v.critic.layout
    slot = ws["slots"][K - 1]
    theta = output_view(cl, ws["acts_c"], B)[:, :, :N].cpu().numpy()
    theta_t = output_view(cl, ws["acts_t"], B)[:, :, :N].cpu().numpy()
    gamma_n = float(v.cfg.algo.gamma) ** int(v.cfg.algo.nstep)
    ref = Q.qr_huber_ref(theta, theta_t, slot["rew"].cpu().numpy(), slot["done"].cpu().numpy(), gamma_n, 1.0, slot["w"].cpu().numpy(),
                         slot["wmax"].cpu().numpy())
    dy_b, _, td_b = Q.qr_bounds(ref, int((B + 3) // 4))
    assert np.unique(slot["w"].cpu().numpy()).size > 10   # (weights that weigh)
    assert (np.abs(ws["dy"][:, :, :N].cpu().numpy().astype(np.float64) - ref["dy"]) <= dy_b).all() and bool((ws["dy"][:, :, N:] == 0).all())
    td = slot["abs_td"].cpu().numpy()
    assert (np.abs(td.astype(np.float64) - ref["abs_td"]) <= td_b).all() and (td > 0).any()
    idx, td_all = ws["per_idx_all"].cpu().numpy().reshape(-1), ws["abs_td_all"].cpu().numpy().reshape(-1)
    before = v.memory.leaves.cpu().numpy().copy()
    v.flush_priorities()
    torch.cuda.synchronize()
    want = before.copy()
    want[idx] = 0
    np.maximum.at(want, idx, np.sqrt(td_all + np.float32(1.0e-3)))
    assert np.array_equal(v.memory.leaves.cpu().numpy().view(np.int32), want.view(np.int32))


def test_bf16_targets_are_refused_on_a_built_learner_too(dev):
    """`check_critic_class` refuses the config key; `set_target_dtype` on a quantile learner refuses the call, and changes nothing."""
    v, _, _ = _learner(8, graph=False)
    with pytest.raises(ValueError, match=r"algo\.target_dtype=bfloat16 is not supported with algo\.cri_class=QuantileDoubleQ"):
        v.set_target_dtype("bfloat16")
    assert not v._bf16 and v.pk_target_bf16 is None
    v.learn()
    v.synchronize()
    assert v.update_count == 1
