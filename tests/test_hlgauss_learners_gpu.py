"""The HL-Gauss loss (algo.distl=True algo.distl_loss=hl_gauss) in the PQL learners and in DDPG on the GPU.

Yardsticks: the CPU torch-autograd learners of tests/hlgauss_cases.py (the oracle's learners with the soft-target cross-entropy in
place of C51's loss) on identical weights, replay rows, injected indices and draws; the learner's own other modes (eager, per-slot
graphs, one run graph); a learner built without the key for the C51 path; a second run from the same seed; the uninterrupted run for
a resumed one.  Bars against the autograd learners: those of the C51 learner at 101 atoms (tests/test_c51_wide_gpu.py): losses at
rtol 2e-5, parameters through `_compare_nets`' defaults.  Shapes: O = 8, A = 2, B = 64, hidden [64, 64], K = 51 and 101.
"""
import functools
import os

import numpy as np
import pytest
import torch

import agent_harness as ah
import detdata as dd
import hlgauss_cases as hc
import learner_harness as lh
from hlgauss_cases import A, B, CAP, HID, HL, O, STEPS, learner_cfg
from learner_harness import PER, _compare_nets, _same_state, _sd, _state
from resume_cases import PQL, PQL_KEYS, PQL_TOY, child, same
from support import T, dev  # noqa: F401

pytestmark = pytest.mark.gpu

LOSSES = ("pqlk_hlgauss_ce_loss", "pqlk_hlgauss_ce_loss_per", "pqlk_c51_bce_loss", "pqlk_td_mse_loss")
_fill = functools.partial(lh._fill, O, A, rew=0.5)
_rows = functools.partial(lh._rows, O, A)
_run = functools.partial(lh._run, n=STEPS)


def _learner(K, *extra, graph, rows=600, seed=11, drop_key=False):
    def cfg_of():
        cfg = learner_cfg(K, *extra, graph=graph)
        if drop_key:   # a configuration from before the key existed
            cfg.algo.pop("distl_loss"); cfg.algo.pop("hl_sigma")
        return cfg
    return lh._learner(cfg_of, O, A, rows, seed)


@pytest.fixture
def counts(monkeypatch):
    """Call counters in front of the real entries."""
    from pql_amd import _lib as L
    seen = {}
    for name in LOSSES + ("pqlk_per_update",):
        real = getattr(L.lib, name)
        seen[name] = 0

        def spy(*a, _n=name, _real=real):
            seen[_n] += 1
            return _real(*a)
        monkeypatch.setattr(L.lib, name, spy)
    return seen


def _weights(K):
    return dd.doubleq_state(O, A, K, 21 + K, HID), dd.mlp_state(O, A, 11, HID)


# ------------------------------------------------------------------------------------------------ against the autograd learners
@pytest.mark.parametrize("K", [51, 101])
def test_pql_learners_vs_autograd(dev, counts, K):
    """Three V steps on injected rows and draws, and one P step (unchanged code) on the critic the V-learner hands out."""
    from oracle import pql_ref_cpu as ref
    from pql_amd.algo.pql_p_learner import PQLPLearner
    from pql_amd.algo.pql_v_learner import PQLVLearner
    cfg, rows = learner_cfg(K, HL[1]), 600
    v, p = PQLVLearner((O,), A, cfg), PQLPLearner((O,), A, cfg)
    assert v.critic.head == "categorical" and v.critic.num_atoms == K and v.head.hl_gauss
    cst, ast = _weights(K)
    v.critic.load_state_dict(_sd(cst)); v.critic_target.arena.data.copy_(v.critic.arena.data)
    p.actor.load_state_dict(_sd(ast))
    data = _fill(rows, 77)
    mean, var = T(dd.uniform((O,), 801, -0.5, 0.5)), T(dd.uniform((O,), 802, 0.5, 2.0))
    hp = ref.HyperRef(batch_size=B, distl=True, num_atoms=K)
    vr = hc.make_v_ref(O, A, hp, CAP, ref.params_from_state(cst, "net_q1.net."), ref.params_from_state(cst, "net_q2.net."))
    pr = ref.PLearnerRef(O, A, hp, CAP, ref.params_from_state(ast))
    vr.update(ref.params_from_state(ast), data, (mean, var, 1e-4))
    norm = (mean.to(dev), var.to(dev), 1e-4)
    v.update(p.actor, tuple(t.to(dev) for t in data), norm, 0)
    for s in range(3):
        idx, draw = T(dd.integers((B,), 900 + s, rows)), T(dd.uniform((B, A), 950 + s, -2, 2))
        lv = vr.learn(idx=idx, draw=draw)
        v.learn(indices=idx, noise=draw)
        v.synchronize()
        print(f"K={K} V step {s}: loss {v.loss_ring[s % 5].item():.9g} vs {lv:.9g}")
        np.testing.assert_allclose(v.loss_ring[s % 5].item(), lv, rtol=2e-5)
    assert v._ws["td_parts"] == 0 and v._ws["td_fwd"] == 0    # the generic head.critic_loss path
    assert counts["pqlk_hlgauss_ce_loss"] == 3 and counts["pqlk_c51_bce_loss"] == counts["pqlk_td_mse_loss"] == 0
    _compare_nets(v.critic, (vr.q1, vr.q2), "critic")
    _compare_nets(v.critic_target, (vr.t1, vr.t2), "target")
    critic, _, _ = v.update(p.actor, _rows(8, 5, dev), norm, 0)
    pr.update(vr.q1, vr.q2, data[0], (mean, var, 1e-4))
    p.update(critic, data[0].to(dev), norm, 0)
    idx = T(dd.integers((B,), 990, rows))
    lp = pr.learn(idx=idx)
    p.learn(indices=idx)
    p.synchronize()
    print(f"K={K} P step: loss {p.loss_ring[0].item():.9g} vs {lp:.9g}")
    np.testing.assert_allclose(p.loss_ring[0].item(), lp, rtol=2e-5, atol=1e-6)
    _compare_nets(p.actor, (pr.actor,), "actor")


@pytest.mark.parametrize("per", [False, True])
def test_ddpg_vs_autograd(dev, per):
    """Three update_once on injected rows and draws, uniform and prioritized (the reference takes the importance weights the agent's
    tree gave the injected rows)."""
    from oracle import pql_ref_cpu as ref
    from pql_amd.algo.ddpg import AgentDDPG
    from pql_amd.envs.synthetic import create_task_env
    from pql_amd.replay.prioritized_replay import PrioritizedReplayBuffer
    from pql_amd.replay.simple_replay import ReplayBuffer
    K, rows = 51, 600
    cfg = learner_cfg(K, HL[1], *(("algo.per.enabled=True", "algo.per.alpha=0.5", "algo.per.eps=1.0e-3") if per else ()), algo="ddpg_algo")
    agent = AgentDDPG(create_task_env(cfg), cfg)
    assert agent.critic.head == "categorical" and agent.critic.num_atoms == K
    cst, ast = _weights(K)
    agent.critic.load_state_dict(_sd(cst)); agent.critic_target.arena.data.copy_(agent.critic.arena.data)
    agent.actor.load_state_dict(_sd(ast))
    mean, var = T(dd.uniform((O,), 801, -0.5, 0.5)), T(dd.uniform((O,), 802, 0.5, 2.0))
    agent.obs_rms.mean, agent.obs_rms.var = mean.to(dev), var.to(dev)
    data = _fill(rows, 77)
    memory = PrioritizedReplayBuffer(CAP, (O,), A, device=dev, alpha=0.5, eps=1.0e-3) if per else ReplayBuffer(CAP, (O,), A, device=dev)
    memory.add_to_buffer(tuple(t.to(dev) for t in data))
    orc = hc.make_ddpg_ref(O, A, ref.HyperRef(batch_size=B, distl=True, num_atoms=K), CAP, ref.params_from_state(ast),
                           ref.params_from_state(cst, "net_q1.net."), ref.params_from_state(cst, "net_q2.net."))
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
        np.testing.assert_allclose(agent.closs[s % 5].item(), cl, rtol=2e-5)
        np.testing.assert_allclose(agent.aloss[s % 5].item(), al_, rtol=2e-5, atol=1e-6)
        if per:
            np.testing.assert_allclose(agent._ws["abs_td"].cpu().numpy(), orc.abs_td.numpy(), rtol=1e-5, atol=1e-5)
    assert not per or spread > 10
    _compare_nets(agent.critic, (orc.q1, orc.q2), "critic")
    _compare_nets(agent.critic_target, (orc.t1, orc.t2), "target")
    _compare_nets(agent.actor, (orc.actor,), "actor")


def test_ddpg_prioritized_is_reproducible(dev):
    """Two agents from one seed (tests/agent_harness.py), three prioritized updates each: the same bits, and priorities that moved."""
    shape = ["task=pointmass", f"task.obs_dim={O}", f"task.act_dim={A}", "num_envs=16", f"algo.batch_size={B}", "algo.memory_size=1024"]
    ends = []
    for _ in range(2):
        agent, memory = ah._agent("ddpg_algo", *HL, "algo.hidden_layers=[64, 64]", "algo.per.enabled=True", shape=shape)
        assert agent.critic.head == "categorical"
        ah._updates(agent, memory, range(3), B=B, A=A)
        ends.append((ah._state(agent), memory.tree.detach().cpu().clone()))
    assert ah._same(ends[0][0], ends[1][0]) and torch.equal(ends[0][1], ends[1][1])
    assert bool(torch.isfinite(ends[0][0]["closs"]).all()) and ends[0][1][:256].unique().numel() > 10


# ------------------------------------------------------------------------------------------------ modes, dispatch, priorities
@pytest.mark.parametrize("K,extra", [(51, ()), (101, ()), (51, PER)])
def test_modes_agree(dev, K, extra):
    """Eager learn() x STEPS, per-slot graphs and one run graph: two runs with an `update()` between leave the same arenas, Adam
    state and loss ring -- and, prioritized, the same tree and pmax."""
    ends = {}
    for mode in ("eager", "slots", "run"):
        v, actor, norm = _learner(K, HL[1], *extra, graph=mode != "eager")
        for rnd in range(2):
            _run(v, mode)
            if rnd == 0:
                v.update(actor, _rows(100, 30, dev), norm, 0)
        assert v.update_count == 2 * STEPS
        assert (len(v._slot_graphs), v._run_graph is not None) == {"eager": (0, False), "slots": (STEPS, False), "run": (0, True)}[mode]
        ends[mode] = _state(v)
    _same_state(ends["eager"], ends["slots"])
    _same_state(ends["eager"], ends["run"])
    e = ends["eager"]
    assert bool(torch.isfinite(e["loss_ring"]).all()) and bool((e["loss_ring"] > 0).all()) and int(e["adam_step"]) == 2 * STEPS
    assert not torch.equal(e["critic"], e["target"])
    if extra:
        assert e["tree"][:600].unique().numel() > 50


def test_the_key_selects_the_entry_and_c51_keeps_its_bits(dev, counts):
    """hl_gauss: pqlk_hlgauss_ce_loss and never pqlk_c51_bce_loss.  The key absent, and distl_loss=c51: the reverse, and after three
    steps the state of a learner built without the key, bit for bit."""
    ends = {}
    for name, extra, drop in (("hl", (HL[1],), False), ("c51", ("algo.distl_loss=c51",), False), ("absent", (), True)):
        before = dict(counts)
        v, _, _ = _learner(51, *extra, graph=False, drop_key=drop)
        assert v.head.hl_gauss == (name == "hl")
        for _ in range(3):
            v.learn()
        ends[name] = _state(v)
        took = {k: counts[k] - before[k] for k in LOSSES}
        want = "pqlk_hlgauss_ce_loss" if name == "hl" else "pqlk_c51_bce_loss"
        assert took == {k: (3 if k == want else 0) for k in LOSSES}, (name, took)
    _same_state(ends["c51"], ends["absent"])
    assert not torch.equal(ends["hl"]["critic"], ends["c51"]["critic"])


def test_prioritized_run_writes_td_back_once_per_run(dev, counts):
    """algo.per.enabled=True algo.per.refresh=run: the weighted entry, one write-back per run, a second learner from the same seed
    ends on the same bits; the same configuration under C51 is still refused with today's message."""
    from pql_amd.algo.pql_v_learner import PQLVLearner
    ends = []
    for _ in range(2):
        before = dict(counts)
        v, actor, norm = _learner(51, HL[1], *PER, graph=True)
        for rnd in range(3):
            _run(v, "run")
        ends.append(_state(v))     # (flushes the last run's |TD|)
        took = {k: counts[k] - before[k] for k in counts}
        assert took["pqlk_per_update"] == 3 and took["pqlk_hlgauss_ce_loss"] == took["pqlk_c51_bce_loss"] == 0
        assert took["pqlk_hlgauss_ce_loss_per"] >= 1       # (captured once into the run graph, replayed afterwards)
    _same_state(*ends)
    assert ends[0]["tree"][:600].unique().numel() > 50 and bool(torch.isfinite(ends[0]["loss_ring"]).all())
    with pytest.raises(ValueError, match="there is no weighted C51 loss"):
        PQLVLearner((O,), A, learner_cfg(51, "algo.distl_loss=c51", *PER))


def test_priorities_are_the_law_applied_to_the_steps_own_heads(dev):
    """A prioritized eager run: the last step's |TD| slab and dy against the float64 law on the heads, rewards, done flags and weights
    that step itself read, within the kernel test's bound (hlgauss_cases.hl_bounds)."""
    from pql_amd.models.mlp import output_view
    K = 51
    v, actor, norm = _learner(K, HL[1], *PER, graph=False)
    _run(v, "eager")
    _run(v, "eager")
    torch.cuda.synchronize()
    ws, cl = v._ws, v.critic.layout
    slot = ws["slots"][STEPS - 1]
    x = output_view(cl, ws["acts_c"], B)[:, :, :K].cpu().numpy()
    xt = output_view(cl, ws["acts_t"], B)[:, :, :K].cpu().numpy()
    algo = v.cfg.algo
    ref = hc.hl_ref(x, xt, slot["rew"].cpu().numpy(), slot["done"].cpu().numpy(), v.critic.z_atoms.cpu().numpy(), float(algo.gamma) ** int(algo.nstep),
                    float(algo.v_min), float(algo.v_max), float(algo.hl_sigma), slot["w"].cpu().numpy(), slot["wmax"].cpu().numpy())
    bound = hc.hl_bounds(ref, hc.loss_blocks(B))
    assert np.unique(slot["w"].cpu().numpy()).size > 10   # (weights that weigh)
    assert (np.abs(ws["dy"][:, :, :K].cpu().numpy().astype(np.float64) - ref["dy"]) <= bound["dy"]).all() and bool((ws["dy"][:, :, K:] == 0).all())
    td = slot["abs_td"].cpu().numpy()
    assert (np.abs(td.astype(np.float64) - ref["abs_td"]) <= bound["abs_td"]).all() and (td > 0).any()


def test_bf16_targets_run_where_c51_takes_them(dev):
    v, _, _ = _learner(51, HL[1], "algo.target_dtype=bfloat16", graph=False)
    assert v._bf16 and v.head.hl_gauss
    for _ in range(2):
        v.learn()
    v.synchronize()
    assert v.update_count == 2 and bool(torch.isfinite(v.loss_ring[:2]).all()) and bool((v.loss_ring[:2] > 0).all())


# ------------------------------------------------------------------------------------------------ resume
def test_resume_is_bit_exact(tmp_path):
    """scripts/train_pql.py under hl_gauss: 6000 steps uninterrupted == 3000 steps, checkpoint, a fresh process, to 6000."""
    base = PQL_TOY + ["algo.graph=True", *HL]
    a = child(PQL, base + ["max_step=6000"], tmp_path)
    ck = tmp_path / "ck"
    b1 = child(PQL, base + ["max_step=3000", f"checkpoint.dir={ck}"], tmp_path)
    assert b1["critic_sha"] != a["critic_sha"] and os.listdir(ck)
    b2 = child(PQL, base + ["max_step=6000", f"resume={ck}"], tmp_path)
    assert b2["resumed_from"]["global_steps"] == b1["global_steps"]
    same(b2["resumed_from"], b1, ("critic_sha", "critic_target_sha", "actor_sha"))
    same(a, b2, PQL_KEYS)
    assert np.isfinite(a["critic_loss"]) and np.isfinite(a["actor_loss"])


def test_a_c51_checkpoint_resumes_under_hl_gauss(tmp_path):
    """The law is no part of a checkpoint's structure: a checkpoint written under c51 loads into a run under hl_gauss, which starts
    from the C51 run's nets and goes on."""
    base = PQL_TOY + ["algo.graph=True", *HL]
    ck51 = tmp_path / "ck51"
    c1 = child(PQL, PQL_TOY + ["algo.graph=True", "algo.distl=True", "max_step=3000", f"checkpoint.dir={ck51}"], tmp_path)
    c2 = child(PQL, base + ["max_step=4000", f"resume={ck51}"], tmp_path)
    same(c2["resumed_from"], c1, ("critic_sha", "critic_target_sha", "actor_sha"))
    assert c2["global_steps"] > c1["global_steps"] and np.isfinite(c2["critic_loss"]) and c2["critic_sha"] != c1["critic_sha"]
