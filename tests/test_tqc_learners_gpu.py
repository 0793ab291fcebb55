"""The truncated pooled target (algo.qr_drop) in the PQL V-learner and in DDPG on the GPU.

Yardsticks: the CPU torch-autograd learners of tests/tqc_cases.py (the oracle's learners with the literal sort-and-truncate law) on
identical weights, replay rows, injected indices and draws, at the tolerances of tests/test_learners_gpu.py for the same comparison
(losses at rtol 1e-5; parameters at rtol 1e-5 with atol 1e-5 = 2 % of one Adam step); the learner's own other modes (eager, per-slot
graphs, one run graph); the uninterrupted run for a resumed one; and the loss entries called directly on the heads a step produced.
Helpers and sizes are those of tests/test_quantile_learners_gpu.py (tests/quantile_cases.py, tests/learner_harness.py).
"""
import numpy as np
import pytest
import torch

import detdata as dd
import tqc_cases as TQ
from learner_harness import PER, _compare_nets, _same_state, _sd, _state
from quantile_cases import A, B, K, O, _cfg, _fill, _learner, _rows, _run, _weights
from support import T, dev  # noqa: F401

pytestmark = pytest.mark.gpu

SETUPS = [(8, 2), (33, 5)]   # (N, d); 33: a padded head (ld 64), an odd pool
ENTRIES = ("pqlk_qr_huber_loss", "pqlk_qr_huber_loss_per", "pqlk_tqc_huber_loss", "pqlk_tqc_huber_loss_per")


def _drop(d):
    return f"algo.qr_drop={d}"


# ------------------------------------------------------------------------------------------------ against the autograd learners
@pytest.mark.parametrize("per", [False, True])
@pytest.mark.parametrize("N,d", SETUPS)
def test_v_learner_vs_autograd(dev, N, d, per):
    """Three V steps on injected rows and draws, uniform and prioritized.  Prioritized: the reference takes the importance weights
    the learner's tree gave the injected rows (from the second step on they differ from row to row)."""
    from oracle import pql_ref_cpu as ref
    from pql_amd.algo.pql_v_learner import PQLVLearner
    from pql_amd.algo.learner import make_actor
    cfg, cap, rows = _cfg(N, _drop(d), *(PER if per else ())), 4096, 3000
    v = PQLVLearner((O,), A, cfg)
    actor = make_actor(cfg, (O,), A, v.device)
    cst, ast = _weights(N)
    v.critic.load_state_dict(_sd(cst)); v.critic_target.arena.data.copy_(v.critic.arena.data)
    actor.load_state_dict(_sd(ast))
    data = _fill(rows, 77)
    mean, var = T(dd.uniform((O,), 801, -0.5, 0.5)), T(dd.uniform((O,), 802, 0.5, 2.0))
    vr = TQ.make_v_ref(O, A, ref.HyperRef(batch_size=B), cap, ref.params_from_state(cst, "net_q1.net."), ref.params_from_state(cst, "net_q2.net."), d)
    vr.update(ref.params_from_state(ast), data, (mean, var, 1e-4))
    v.update(actor, tuple(t.to(dev) for t in data), (mean.to(dev), var.to(dev), 1e-4), 0)
    spread = 0
    for s in range(3):
        idx, draw = T(dd.integers((B,), 900 + s, rows)), T(dd.uniform((B, A), 950 + s, -2, 2))
        v.learn(indices=idx, noise=draw)
        v.synchronize()
        if per:
            w = v._ws["w_all"][0].cpu()
            vr.wh = w / v._ws["wmax_all"][0].cpu()
            spread = max(spread, int(torch.unique(w).numel()))
        lv = vr.learn(idx=idx, draw=draw)
        print(f"N={N} d={d} per={per} V step {s}: loss {v.loss_ring[s % 5].item():.9g} vs {lv:.9g}")
        np.testing.assert_allclose(v.loss_ring[s % 5].item(), lv, rtol=1e-5)
        if per:   # |TD| of the step (fp32 on both sides: the bar of the parameters)
            np.testing.assert_allclose(v._ws["abs_td_all"][0].cpu().numpy(), vr.abs_td.numpy(), rtol=1e-5, atol=1e-5)
    assert not per or spread > 10
    assert v._ws["td_parts"] == 0 and v._ws["td_fwd"] == 0
    _compare_nets(v.critic, (vr.q1, vr.q2), "critic")
    _compare_nets(v.critic_target, (vr.t1, vr.t2), "target")


@pytest.mark.parametrize("per", [False, True])
@pytest.mark.parametrize("N,d", SETUPS)
def test_ddpg_vs_autograd(dev, N, d, per):
    """Three inner iterations of update_net (update_once on injected rows and draws), uniform and prioritized (refresh=step)."""
    from oracle import pql_ref_cpu as ref
    from pql_amd.algo.ddpg import AgentDDPG
    from pql_amd.envs.synthetic import create_task_env
    from pql_amd.replay.prioritized_replay import PrioritizedReplayBuffer
    from pql_amd.replay.simple_replay import ReplayBuffer
    cap, rows = 4096, 3000
    cfg = _cfg(N, _drop(d), *(("algo.per.enabled=True", "algo.per.alpha=0.5", "algo.per.eps=1.0e-3") if per else ()), algo="ddpg_algo", memory=cap)
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
    orc = TQ.make_ddpg_ref(O, A, ref.HyperRef(batch_size=B), cap, ref.params_from_state(ast), ref.params_from_state(cst, "net_q1.net."),
                           ref.params_from_state(cst, "net_q2.net."), d)
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
        print(f"N={N} d={d} per={per} step {s}: closs {agent.closs[s % 5].item():.9g} vs {cl:.9g}; aloss {agent.aloss[s % 5].item():.9g} vs {al_:.9g}")
        np.testing.assert_allclose(agent.closs[s % 5].item(), cl, rtol=1e-5)
        np.testing.assert_allclose(agent.aloss[s % 5].item(), al_, rtol=1e-5, atol=1e-7)
        if per:
            np.testing.assert_allclose(agent._ws["abs_td"].cpu().numpy(), orc.abs_td.numpy(), rtol=1e-5, atol=1e-5)
    assert not per or spread > 10
    _compare_nets(agent.critic, (orc.q1, orc.q2), "critic")
    _compare_nets(agent.critic_target, (orc.t1, orc.t2), "target")
    _compare_nets(agent.actor, (orc.actor,), "actor")


# ------------------------------------------------------------------------------------------------ modes, resume
@pytest.mark.parametrize("extra", [(), PER])
@pytest.mark.parametrize("N,d", SETUPS)
def test_modes_agree(dev, N, d, extra):
    """Eager learn() x K, per-slot graphs and one run graph: two runs with an `update()` between leave the same arenas, Adam state
    and loss ring -- and, prioritized (refresh=run), the same tree and pmax."""
    ends = {}
    for mode in ("eager", "slots", "run"):
        v, actor, norm = _learner(N, _drop(d), *extra, graph=mode != "eager")
        for rnd in range(2):
            _run(v, mode)
            if rnd == 0:
                v.update(actor, _rows(300, 30, dev), norm, 0)
        assert v.update_count == 2 * K
        assert (len(v._slot_graphs), v._run_graph is not None) == {"eager": (0, False), "slots": (K, False), "run": (0, True)}[mode]
        ends[mode] = _state(v)
    _same_state(ends["eager"], ends["slots"])
    _same_state(ends["eager"], ends["run"])
    e = ends["eager"]
    assert bool(torch.isfinite(e["loss_ring"]).all()) and bool((e["loss_ring"] > 0).all()) and int(e["adam_step"]) == 2 * K
    if extra:
        assert e["tree"][:1800].unique().numel() > 100


@pytest.mark.parametrize("extra", [(), PER])
def test_resume_continues_bit_exactly(dev, extra):
    """One run, save, one more run -- against a fresh learner that loads the saved state (and the ring's rows) and takes that run."""
    N, d = SETUPS[0]
    a, actor, norm = _learner(N, _drop(d), *extra, graph=True)
    _run(a, "run")
    a.synchronize()
    st, rows = a.training_state(), a.memory.rows().clone()
    _run(a, "run")
    b, _, _ = _learner(N, _drop(d), *extra, graph=True, seed=12)   # other weights, other rows, another generator state
    b.load_training_state(st)
    b.memory.rows().copy_(rows)
    _run(b, "run")
    assert a.update_count == b.update_count == 2 * K
    _same_state(_state(a), _state(b))


# ------------------------------------------------------------------------------------------------ which entry a step takes
@pytest.fixture
def entries(monkeypatch):
    """Records which of the four quantile loss entries a step goes through."""
    from pql_amd import _lib as L
    seen = []
    for name in ENTRIES:
        inner = getattr(L.lib, name)

        def spy(*a, _inner=inner, _name=name):
            seen.append(_name)
            return _inner(*a)

        monkeypatch.setattr(L.lib, name, spy)
    return seen


def _direct(dev, v, N, drop, per):
    """The loss entry (`drop` None: the entry without the key) called on the heads, rewards, done flags and weights the learner's last
    eager step read, into fresh buffers -> (dy, the loss, |TD|)."""
    from pql_amd import _lib as L
    from pql_amd.models.mlp import output_view
    ws, cl = v._ws, v.critic.layout
    slot = ws["slots"][0]
    q, qt = output_view(cl, ws["acts_c"], B), output_view(cl, ws["acts_t"], B)
    dy = torch.full_like(ws["dy"], float("nan"))
    ring, step = torch.zeros(5, dtype=torch.float32, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
    scratch, abs_td = torch.empty(1024, dtype=torch.float32, device=dev), torch.zeros(B, dtype=torch.float32, device=dev)
    gamma_n = float(v.cfg.algo.gamma) ** int(v.cfg.algo.nstep)
    head = (L.ptr(q), L.ptr(qt), cl.ld_out, N, L.ptr(slot["rew"]), L.ptr(slot["done"]), gamma_n, 1.0, B, L.ptr(dy), L.ptr(ring), L.ptr(step), 5,
            L.ptr(scratch))
    tail = (L.ptr(slot["w"]), L.ptr(slot["wmax"]), L.ptr(abs_td)) if per else ()
    name = ("pqlk_qr_huber_loss" if drop is None else "pqlk_tqc_huber_loss") + ("_per" if per else "")
    with torch.cuda.device(dev):
        L.check(getattr(L.lib, name)(*head, *tail, *(() if drop is None else (drop,)), L.stream(dev)))
        torch.cuda.synchronize(dev)
    return dy, ring[0].item(), abs_td


@pytest.mark.parametrize("per", [False, True])
@pytest.mark.parametrize("N,d", [(8, None), (33, None), (8, 2), (33, 5), (8, 0)])
def test_a_step_takes_the_entry_its_key_names_and_folds_with_its_divisor(dev, entries, N, d, per):
    """qr_drop=null: the step goes through the entry without the key, and its dy, loss and |TD| are that entry's bits on the step's own
    heads.  qr_drop=d (0 included): through the truncated entry; the loss the optimiser launch folded (scale 1 / (B M) on
    pqlk_loss_parts(B, N) partials) is the bits of the entry's own fold."""
    v, _, _ = _learner(N, *(() if d is None else (_drop(d),)), *(PER if per else ()), graph=False)
    v.learn()
    v.synchronize()
    want = ("pqlk_qr_huber_loss" if d is None else "pqlk_tqc_huber_loss") + ("_per" if per else "")
    assert entries == [want]
    del entries[:]
    dy, loss, abs_td = _direct(dev, v, N, d, per)
    assert torch.equal(dy, v._ws["dy"]) and bool((dy[:, :, N:] == 0).all())
    assert loss == v.loss_ring[0].item() and loss > 0
    if per:
        assert torch.equal(abs_td, v._ws["slots"][0]["abs_td"])


@pytest.mark.parametrize("d", [None, 2])
def test_ddpg_takes_the_entry_its_key_names(dev, entries, d):
    from pql_amd.algo.ddpg import AgentDDPG
    from pql_amd.envs.synthetic import create_task_env
    from pql_amd.replay.simple_replay import ReplayBuffer
    cfg = _cfg(8, *(() if d is None else (_drop(d),)), algo="ddpg_algo", memory=4096)
    agent = AgentDDPG(create_task_env(cfg), cfg)
    memory = ReplayBuffer(4096, (O,), A, device=dev)
    memory.add_to_buffer(tuple(t.to(dev) for t in _fill(1000, 77)))
    agent.update_once(memory, indices=T(dd.integers((B,), 40, 1000)), noise=T(dd.uniform((B, A), 50, -2, 2)))
    torch.cuda.synchronize(dev)
    assert entries == ["pqlk_qr_huber_loss" if d is None else "pqlk_tqc_huber_loss"]
    assert np.isfinite(agent.closs[0].item()) and agent.closs[0].item() > 0
