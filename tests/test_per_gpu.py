"""Prioritized replay on the GPU (pql_amd/csrc/per.hip, include/pqlk.h "Prioritized experience replay").

Every reference here is NumPy written in this file: float64 cumulative sums for the sampler, the documented fp32 butterfly for the
tree's sums, float64 `pow` for the two powf paths, float64 of the loss formula.  Nothing is compared with the code under test
except where the statement IS "two paths give the same bits" (incremental maintenance against rebuild, the weighted loss with unit
weights against the plain loss, two runs from one seed, a resumed run against the uninterrupted one).
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from per_cases import Tree, level_sizes, model_tree
from support import T, dev  # noqa: F401

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ a tree and its NumPy model: tests/per_cases.py
def ulps(a, b):
    """Distance in units of the last place between positive fp32 arrays."""
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


# ------------------------------------------------------------------------------------------------ sampling, exact data
CAPS = (1, 63, 64, 65, 4096, 4097, 262_145)
BATCHES = (1, 64, 257)


def exact_leaves(tree, model, rows, B, rng):
    """Raise some of `rows` (through pqlk_per_update, alpha 1, eps 0) until the total is B * 2^s: then seg = total / B is a power of
    two and t_k = (k + u_k) * seg, with u on a grid of 2^-10 and k < 2^9, is exact in fp32.  Integers below 2^24 throughout, so every
    sum in the tree is exact whatever its order."""
    total = int(model.sum())
    target = B
    while target < max(total, 1):
        target *= 2
    deficit = target - total
    if deficit:
        pick = rng.permutation(rows)[: min(len(rows), 97)]
        add = np.full(len(pick), deficit // len(pick), dtype=np.int64)
        add[: deficit % len(pick)] += 1
        new = model[pick].astype(np.int64) + add
        tree.update(pick, new.astype(np.float32))
        model[pick] = new
    assert int(model.sum()) == target < 2 ** 24
    return target


@pytest.mark.parametrize("variant", ["full", "partly_filled", "wrapped_insert", "one_row"])
@pytest.mark.parametrize("capacity", CAPS)
def test_sampling_is_exact_on_exactly_summable_priorities(dev, capacity, variant):
    rng = np.random.default_rng(1000 * CAPS.index(capacity) + len(variant))
    tree = Tree(capacity, dev)
    model = np.zeros(capacity, dtype=np.float64)
    n_valid = capacity if variant != "partly_filled" else max(1, (2 * capacity) // 3)
    if variant == "one_row":
        rows = np.array([int(rng.integers(capacity))])
    else:
        rows = np.arange(n_valid)
        vals = rng.integers(0, 9, size=n_valid)
        vals[int(rng.integers(n_valid))] = 8            # (at least one non-zero row)
        tree.update(rows, vals.astype(np.float32))
        model[rows] = vals
        if variant == "wrapped_insert" and capacity >= 8:   # the ring's last insert wrapped: a head segment and a tail segment
            head, tail = min(3, capacity // 4), min(5, capacity // 4)
            tree.insert(capacity - head, head)
            tree.insert(0, tail)
            model[capacity - head:] = model[:tail] = model.max()   # pmax (alpha 1): the largest priority assigned so far
            assert float(tree.pmax.item()) == model.max() == 8.0
    for B in BATCHES:
        total = exact_leaves(tree, model, rows, B, rng)
        assert np.array_equal(tree.leaves().astype(np.float64), model)
        u = rng.integers(0, 1024, size=B) / 1024.0
        t = (np.arange(B) + u) * (total / B)
        assert np.array_equal(t.astype(np.float32).astype(np.float64), t)        # exact in fp32, as promised
        got = tree.sample(u)
        want = np.searchsorted(np.cumsum(model), t, side="right")
        assert np.array_equal(got, want), (capacity, variant, B, np.flatnonzero(got != want)[:5])
        assert got.max() < n_valid and got.min() >= 0 and np.all(model[got] > 0)
        # stratification: B equal segments of the mass, one draw from each -> a row's count is within one of its share, either side
        share = B * model / total
        count = np.bincount(got, minlength=capacity)
        assert np.all(count >= np.floor(share) - 1) and np.all(count <= np.ceil(share) + 1)
    torch.cuda.synchronize()


def test_sampling_on_random_priorities(dev):
    """fp32 priorities over six orders of magnitude, capacity 262 145 (4 levels).  Every returned row i must hold t_k up to the slack
    s = 16 * levels * 2^-24 * total: at most 13 roundings per level (6 in a node's sum, 6 in the prefix, 1 in the subtraction), each at
    most 2^-24 of a quantity that is at most the total."""
    capacity, B = 262_145, 4096
    rng = np.random.default_rng(7)
    tree = Tree(capacity, dev)
    tree.update(np.arange(capacity), (10.0 ** rng.uniform(-3, 3, size=capacity)).astype(np.float32))
    leaves = tree.leaves()
    assert leaves.min() > 0 and leaves.max() / leaves.min() > 1e5
    cum = np.cumsum(leaves.astype(np.float64))
    total = cum[-1]
    u = rng.random(B).astype(np.float32)
    t = (np.arange(B) + u.astype(np.float64)) * (total / B)
    got = tree.sample(u)
    assert got.min() >= 0 and got.max() < capacity
    s = 16 * len(level_sizes(capacity)) * 2.0 ** -24 * total
    below = np.where(got > 0, cum[np.maximum(got - 1, 0)], 0.0)
    bad = np.flatnonzero((below - s > t) | (t > cum[got] + s))
    assert bad.size == 0, (bad[:5], got[bad[:5]], t[bad[:5]], below[bad[:5]], cum[got[bad[:5]]])
    count = np.bincount(got, minlength=capacity)
    share = B * leaves.astype(np.float64) / total
    assert np.all(count >= np.floor(share) - 1) and np.all(count <= np.ceil(share) + 1)


# ------------------------------------------------------------------------------------------------ maintenance
@pytest.mark.parametrize("capacity", [65, 4097, 70_000])
def test_incremental_maintenance_equals_rebuild(dev, capacity):
    """A random interleaving of ring inserts (wrapping included) and updates with duplicated rows, alpha = 0.5 (sqrtf: correctly
    rounded, so NumPy gives the leaves' bits).  The tree kept incrementally == pqlk_per_rebuild of its leaves == the documented
    butterfly in NumPy, bit for bit; a duplicated row holds the largest of its candidates; pmax is the running maximum."""
    from pql_amd.replay.simple_replay import ring_plan
    rng = np.random.default_rng(capacity)
    tree = Tree(capacity, dev)
    alpha, eps = 0.5, np.float32(1e-3)
    leaves, pmax = np.zeros(capacity, dtype=np.float32), np.float32(1.0)
    next_p, full, cur, wraps = 0, False, 0, 0
    for step in range(14):
        m = int(rng.integers(1, max(2, capacity // 3)))
        segs, next_p, full, cur = ring_plan(next_p, full, capacity, m)
        wraps += len(segs) == 2
        for dst, _, n in segs:
            tree.insert(dst, n, alpha)
            leaves[dst: dst + n] = np.sqrt(pmax)
        b = 300
        idx = rng.integers(0, cur, size=b)
        idx[b // 2:] = idx[: b - b // 2]                       # every row of the first half is drawn at least twice
        td = (10.0 ** rng.uniform(-3, 1.5, size=b)).astype(np.float32)
        tree.update(idx, td, alpha, float(eps))
        p = td + eps                                            # fp32
        cand = np.sqrt(p)
        leaves[idx] = 0
        np.maximum.at(leaves, idx, cand)
        pmax = max(pmax, p.max())
    assert wraps >= 1 and full
    kept = tree.buffer()
    assert np.array_equal(kept[:capacity].view(np.int32), leaves.view(np.int32))
    assert np.float32(tree.pmax.item()) == pmax
    want, _ = model_tree(leaves)
    assert np.array_equal(kept.view(np.int32), want.view(np.int32))
    tree.rebuild()
    assert np.array_equal(tree.buffer().view(np.int32), kept.view(np.int32))


# ------------------------------------------------------------------------------------------------ weights and the two powf paths
# Largest distances from float64 `pow` rounded to fp32, measured on an MI355X on the first run of this file: 2 ulp for
# powf(x, -0.4) over the 1000 weights below, 4 ulp for powf(p, 0.6) over the 4097 leaves below.  The bounds are those + 2.  OpenCL
# allows pow 16 ulp; a larger value is a finding, not a constant to raise.
POWF_ULP_BETA = 2 + 2
POWF_ULP_ALPHA = 4 + 2


def _weights_case(dev):
    capacity, B = 4097, 1000
    rng = np.random.default_rng(11)
    tree = Tree(capacity, dev)
    tree.update(np.arange(capacity), (10.0 ** rng.uniform(-3, 3, size=capacity)).astype(np.float32))
    leaves = tree.leaves()
    _, total = model_tree(leaves)
    idx = rng.integers(0, capacity, size=B)
    x = (np.float32(capacity) * leaves[idx]) / total             # fp32: one multiplication, one division
    assert x.dtype == np.float32
    return tree, capacity, idx, x


def test_weights_beta_zero_and_one_are_exact(dev):
    tree, capacity, idx, x = _weights_case(dev)
    w, wmax = tree.weights(idx, capacity, 0.0)
    assert np.all(w == 1.0) and wmax == 1.0
    w, wmax = tree.weights(idx, capacity, 1.0)
    want = np.float32(1.0) / x
    assert np.array_equal(w.view(np.int32), want.view(np.int32)) and np.float32(wmax) == want.max()


def test_weights_powf_path(dev):
    tree, capacity, idx, x = _weights_case(dev)
    w, wmax = tree.weights(idx, capacity, 0.4)
    want = np.power(x.astype(np.float64), -0.4).astype(np.float32)
    d = ulps(w, want)
    print(f"powf(x, -0.4): largest distance {d.max()} ulp over {d.size} weights")
    assert np.float32(wmax) == w.max()
    assert d.max() <= POWF_ULP_BETA <= 16


def test_priority_powf_path(dev):
    capacity = 4097
    rng = np.random.default_rng(12)
    tree = Tree(capacity, dev)
    td = (10.0 ** rng.uniform(-4, 3, size=capacity)).astype(np.float32)
    eps = np.float32(1e-6)
    tree.update(np.arange(capacity), td, 0.6, float(eps))
    want = np.power((td + eps).astype(np.float64), 0.6).astype(np.float32)
    d = ulps(tree.leaves(), want)
    print(f"powf(p, 0.6): largest distance {d.max()} ulp over {d.size} leaves")
    assert np.float32(tree.pmax.item()) == (td + eps).max()
    assert d.max() <= POWF_ULP_ALPHA <= 16


# ------------------------------------------------------------------------------------------------ the weighted loss
def _loss_inputs(B, dev, seed):
    """Multiples of 2^-6 in [-4, 4], done in {0, 1}, gamma^n = 0.5: y and q - y are exact in fp32."""
    rng = np.random.default_rng(seed)
    grid = lambda shape: (rng.integers(-256, 257, size=shape) / 64.0).astype(np.float32)  # noqa: E731
    q, qt = np.zeros((2, B, 32), dtype=np.float32), np.zeros((2, B, 32), dtype=np.float32)
    q[:, :, 0], qt[:, :, 0] = grid((2, B)), grid((2, B))
    rew, done = grid(B), (rng.random(B) < 0.2).astype(np.float32)
    return q, qt, rew, done


def _run_loss(dev, q, qt, rew, done, w=None, wmax=None, slot=None):
    from pql_amd import _lib as L
    B = q.shape[1]
    d = lambda a: T(a).to(dev)  # noqa: E731
    qd, qtd, rd, dd_ = d(q), d(qt), d(rew), d(done)
    dy, ring, scratch = torch.full((2, B, 32), 9.0, device=dev), torch.full((5,), -3.0, device=dev), torch.zeros(2048, device=dev)
    slot_dev = None if slot is None else torch.tensor([slot], dtype=torch.int32, device=dev)
    head = (L.ptr(qd), L.ptr(qtd), 32, L.ptr(rd), L.ptr(dd_), 0.5, B, L.ptr(dy), L.ptr(ring), L.ptr(slot_dev), 5, L.ptr(scratch))
    if w is None:
        L.check(L.lib.pqlk_td_mse_loss(*head, L.stream(dev)))
        return dy.cpu().numpy(), ring.cpu().numpy(), None
    wd, wm, td = d(w), d(np.array([wmax], dtype=np.float32)), torch.full((B,), -1.0, device=dev)
    L.check(L.lib.pqlk_td_mse_loss_per(*head, L.ptr(wd), L.ptr(wm), L.ptr(td), L.stream(dev)))
    return dy.cpu().numpy(), ring.cpu().numpy(), td.cpu().numpy()


@pytest.mark.parametrize("B", [1, 255, 256, 257, 256 * 1024 + 1])
def test_weighted_loss_with_unit_weights_is_the_plain_loss(dev, B):
    q, qt, rew, done = _loss_inputs(B, dev, B)
    q[:, :, 0] += (np.random.default_rng(B + 1).random((2, B)).astype(np.float32) - 0.5)   # inexact differences too
    slot = 3 if B % 2 else None
    dy0, ring0, _ = _run_loss(dev, q, qt, rew, done, slot=slot)
    dy1, ring1, td = _run_loss(dev, q, qt, rew, done, w=np.ones(B, dtype=np.float32), wmax=1.0, slot=slot)
    assert np.array_equal(dy0.view(np.int32), dy1.view(np.int32))
    assert np.array_equal(ring0.view(np.int32), ring1.view(np.int32)) and ring0[3 if slot else 0] != -3.0
    y = rew + ((np.float32(1) - done) * np.float32(0.5)) * np.minimum(qt[0, :, 0], qt[1, :, 0])
    assert np.array_equal(td, np.maximum(np.abs(q[0, :, 0] - y), np.abs(q[1, :, 0] - y)))


def test_weighted_loss_against_float64(dev):
    """dy = (2 / B) (w / wmax) (q - y) with q - y exact: the division, 2 / B and two multiplications round, half an ulp each: 2 ulp."""
    B = 257
    q, qt, rew, done = _loss_inputs(B, dev, 5)
    w = np.random.default_rng(6).uniform(0.05, 1.0, size=B).astype(np.float32)
    wmax = float(w.max())
    dy, ring, td = _run_loss(dev, q, qt, rew, done, w=w, wmax=wmax)
    f = lambda a: a.astype(np.float64)  # noqa: E731
    y = f(rew) + (1.0 - f(done)) * 0.5 * np.minimum(f(qt[0, :, 0]), f(qt[1, :, 0]))
    d1, d2 = f(q[0, :, 0]) - y, f(q[1, :, 0]) - y
    assert np.array_equal(d1.astype(np.float32).astype(np.float64), d1)                    # exact, as promised
    wh = f(w) / np.float64(np.float32(wmax))
    for n, dn in enumerate((d1, d2)):
        want = ((2.0 / B) * wh * dn).astype(np.float32)
        got = dy[n, :, 0]
        nz = want != 0
        assert np.all(got[~nz] == 0) and np.all(np.sign(got[nz]) == np.sign(want[nz]))
        assert ulps(np.abs(got[nz]), np.abs(want[nz])).max() <= 2
    assert np.array_equal(td.astype(np.float64), np.maximum(np.abs(d1), np.abs(d2)))        # abs_td: exact
    loss = np.mean(wh * d1 * d1) + np.mean(wh * d2 * d2)
    assert abs(ring[0] - loss) <= 1e-5 * loss
    assert np.all(dy[:, :, 1:] == 9.0)                                                     # only column 0 is written, as the plain loss


# ------------------------------------------------------------------------------------------------ agents
O, A, B_AGENT, RING = 8, 2, 256, 4096
AGENTS = {"ddpg_algo": ("pql_amd.algo.ddpg", "AgentDDPG"), "sac_algo": ("pql_amd.algo.sac", "AgentSAC"),
          "crossq_algo": ("pql_amd.algo.crossq", "AgentCrossQ")}
SHAPE = ["task=pointmass", "num_envs=64", f"algo.batch_size={B_AGENT}", f"algo.memory_size={RING}", "algo.hidden_layers=[64,64]"]


def _agent(algo, *extra, prioritized=True, seed=3):
    """Agent, PointMass env and a ring filled by the warm-up rollout (1920 rows), all from `seed`."""
    import importlib
    from pql_amd.envs.synthetic import create_task_env
    from pql_amd.replay.prioritized_replay import PrioritizedReplayBuffer
    from pql_amd.replay.simple_replay import ReplayBuffer
    from pql_amd.utils.cfg import load_cfg
    from pql_amd.utils.common import preprocess_cfg, set_random_seed
    cfg = load_cfg([f"algo={algo}", *SHAPE, "device=cuda:0", "sim_device=cuda:0", "rl_device=cuda:0", f"seed={seed}", *extra])
    set_random_seed(cfg.seed)
    cfg.algo.v_learner_gpu = cfg.algo.p_learner_gpu = 0
    preprocess_cfg(cfg)
    env = create_task_env(cfg)
    mod, cls = AGENTS[algo]
    agent = getattr(importlib.import_module(mod), cls)(env=env, cfg=cfg)
    agent.reset_agent()
    if prioritized:
        memory = PrioritizedReplayBuffer(RING, agent.obs_dim, agent.action_dim, device=agent.device, alpha=float(cfg.algo.per.alpha),
                                         eps=float(cfg.algo.per.eps))
    else:
        memory = ReplayBuffer(RING, agent.obs_dim, agent.action_dim, device=agent.device)
    trajectory, _ = agent.explore_env(env, cfg.algo.warm_up, random=True)
    memory.add_to_buffer(trajectory)
    assert memory.cur_capacity == 1920
    return agent, memory


def _arenas(agent):
    torch.cuda.synchronize()
    return {k: v.detach().cpu().clone() for k, v in agent._state_tensors().items()}


@pytest.mark.parametrize("algo", ["ddpg_algo", "sac_algo"])
def test_prioritized_agents_are_bitwise_reproducible(algo):
    runs = []
    for _ in range(2):
        agent, memory = _agent(algo, "algo.per.enabled=True")
        assert agent.per is not None and agent.beta() == 0.4
        for _ in range(6):
            agent.update_once(memory)
        runs.append((_arenas(agent), memory.tree.cpu().clone(), memory.pmax.cpu().clone()))
    (a, ta, pa), (b, tb, pb) = runs
    assert set(a) == set(b) and {"critic", "copt.m", "closs"} <= set(a)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    assert torch.equal(ta.view(torch.int32), tb.view(torch.int32)) and torch.equal(pa, pb)
    leaves = ta[:1920]
    assert bool((leaves > 0).all()) and bool((ta[1920:RING] == 0).all()) and leaves.unique().numel() > 100   # priorities did move
    assert float(pa) > 0 and bool(torch.isfinite(a["closs"]).all())


def test_hooks_change_nothing_else():
    """alpha = 0 (every priority 1), beta0 = 1: every weight is exactly 1, so the prioritized path must leave the bits the plain path
    leaves when both are given the same indices and noise."""
    ends = []
    for prioritized in (True, False):
        agent, memory = _agent("ddpg_algo", "algo.per.enabled=True", "algo.per.alpha=0.0", "algo.per.beta0=1.0", prioritized=prioritized)
        g = torch.Generator().manual_seed(5)
        for _ in range(3):
            idx = torch.randint(0, 1920, (B_AGENT,), generator=g)
            agent.update_once(memory, indices=idx, noise=torch.randn((B_AGENT, A), generator=g))
        ends.append(_arenas(agent))
        if prioritized:
            assert bool((memory.tree[:1920] == 1.0).all()) and float(memory.wmax) == 1.0 and bool((memory.w == 1.0).all())
    for k in ends[0]:
        assert torch.equal(ends[0][k], ends[1][k]), k


def test_crossq_runs_prioritized():
    agent, memory = _agent("crossq_algo", "algo.per.enabled=True")
    for _ in range(3):
        agent.update_once(memory)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(agent.closs[:3]).all()) and bool(torch.isfinite(agent.aloss[:3]).all())
    assert bool(torch.isfinite(memory.tree).all()) and memory.tree[:1920].unique().numel() > 100


CHILD = """
import importlib.util, json, sys
spec = importlib.util.spec_from_file_location("entry", sys.argv[1])
mod = importlib.util.module_from_spec(spec)
spec.loader.exec_module(mod)
from pql_amd.utils.cfg import load_cfg
out = mod.main(load_cfg(sys.argv[2:]))
sys.stdout.flush()
print("CHILD_RESULT " + json.dumps(out), flush=True)
"""


def _child(overrides, cwd, timeout=120):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    r = subprocess.run([sys.executable, "-c", CHILD, os.path.join(ROOT, "scripts", "train_baselines.py"), *overrides], env=env, cwd=str(cwd),
                       capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, f"{overrides}\n{r.stderr[-4000:]}"
    lines = [l for l in r.stdout.splitlines() if l.startswith("CHILD_RESULT ")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0][len("CHILD_RESULT "):])


def test_prioritized_ddpg_resumes_bit_exact(tmp_path):
    """6 iterations uninterrupted == 3 iterations, checkpoint, a fresh process, 3 more: arenas, ring, tree leaves, pmax.  beta_iters=4,
    so the schedule's position has to survive too.  Each child is its own process with its own time limit; a failing one ends the test."""
    base = ["algo=ddpg_algo", *SHAPE, "algo.per.enabled=True", "algo.per.beta_iters=4"]
    warm = 64 * 32
    a = _child(base + [f"max_step={warm + 6 * 64 - 1}"], tmp_path)
    assert a["iters"] == 6 and a["per_sha"] and a["per_pmax"] > 0
    ck = tmp_path / "ck"
    b1 = _child(base + [f"max_step={warm + 3 * 64 - 1}", f"checkpoint.dir={ck}"], tmp_path)
    assert b1["iters"] == 3 and b1["per_sha"] != a["per_sha"]
    b2 = _child(base + [f"max_step={warm + 6 * 64 - 1}", f"resume={ck}"], tmp_path)
    assert b2["resumed_from"]["global_steps"] == b1["global_steps"]
    for k in ("actor_sha", "critic_sha", "replay_sha", "per_sha", "per_pmax", "global_steps", "iters", "train/critic_loss", "train/actor_loss"):
        assert a[k] == b2[k], (k, a[k], b2[k])
    with pytest.raises(AssertionError, match=r"algo\.per\.enabled=False.*algo\.per\.enabled=True"):
        _child(["algo=ddpg_algo", *SHAPE, f"max_step={warm + 6 * 64 - 1}", f"resume={ck}"], tmp_path)
