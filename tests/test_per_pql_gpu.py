"""Prioritized replay in the PQL V-learner, frozen per run of prefetched steps (`algo.per.refresh=run`; pql_amd/csrc/per.hip
`pqlk_per_sample_steps`, pql_amd/algo/pql_v_learner.py), on the GPU.

The kernel's yardsticks are the per-step entries it restates (`pqlk_per_sample` fed u = r 2^-24, `pqlk_per_weights`: the statement IS
"the same bits on the same device") and, on exactly summable priorities, NumPy's searchsorted over a float64 cumulative sum.  The
learner's are those same entries applied to a clone of the tree taken before the run, NumPy's correctly rounded sqrt for the
write-back (alpha = 0.5), its own other modes (eager, per-slot graphs, one run graph), a plain learner when every weight is 1, and the
uninterrupted run for a resumed one.
"""
import functools
import json
import os

import numpy as np
import pytest
import torch

import learner_harness as lh
from learner_harness import PER, _same_state, _state
from per_cases import Tree, model_tree
from resume_cases import PQL, PQL_KEYS, PQL_TOY, child, same
from support import T, dev  # noqa: F401

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R24 = 1 << 24


@pytest.fixture(autouse=True)
def _keep_sigint():
    """The entry points' `main` installs a Ctrl+C handler (capture_keyboard_interrupt); here one runs inside pytest's process."""
    import signal
    old = signal.getsignal(signal.SIGINT)
    yield
    signal.signal(signal.SIGINT, old)


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32)).view(np.int32)


# ------------------------------------------------------------------------------------------------ the kernel
B_K, STEPS = 96, 3                     # 96: no multiple of the 64 lanes, nor of a block's 4 samples x 64; 24 blocks per step, 3 rows of blocks
CAPS = (50, 4096, 4097)                # one level; two levels of full nodes; three levels (4097 / 65 / 2 nodes, ragged tails)


def sample_steps(tree, r, n_valid, beta):
    """pqlk_per_sample_steps on `tree` (a per_cases.Tree) -> (idx (steps, b), w (steps, b), wmax (steps)) as NumPy, outputs poisoned first."""
    L = tree.L
    steps, b = r.shape
    rd = T(np.asarray(r, dtype=np.int64)).to(tree.dev)
    idx = torch.full((steps, b), -7, dtype=torch.int64, device=tree.dev)
    w, wmax = torch.full((steps, b), -1.0, device=tree.dev), torch.full((steps,), 123.0, device=tree.dev)
    L.check(L.lib.pqlk_per_sample_steps(L.ptr(tree.tree), tree.cap, L.ptr(rd), b, steps, n_valid, beta, L.ptr(idx), L.ptr(w), L.ptr(wmax),
                                        L.stream(tree.dev)))
    return idx.cpu().numpy(), w.cpu().numpy(), wmax.cpu().numpy()


def draws(rng):
    r = rng.integers(0, R24, size=(STEPS, B_K))
    r[0, 0], r[0, 7], r[1, 5], r[2, B_K - 1], r[2, 0] = 0, R24 - 1, R24 - 1, R24 - 1, 0   # both ends of the range, last stratum included
    return r


def kernel_tree(dev, capacity, alpha, rng):
    """Priorities over six orders of magnitude on the first two thirds of the rows (n_valid < capacity: the rest are zero leaves), a
    tenth of the valid rows zeroed as well; the upper levels rebuilt from those leaves."""
    tree = Tree(capacity, dev)
    n_valid = max(3, (2 * capacity) // 3)
    tree.update(np.arange(n_valid), (10.0 ** rng.uniform(-3, 3, size=n_valid)).astype(np.float32), alpha, 1e-3)
    zero = rng.permutation(n_valid)[: max(1, n_valid // 10)]
    tree.tree[T(zero).to(dev)] = 0.0
    tree.rebuild()
    leaves = tree.leaves()
    assert np.all(leaves[n_valid:] == 0) and np.count_nonzero(leaves[:n_valid] == 0) == len(zero) and np.count_nonzero(leaves) > 0
    return tree, n_valid


@pytest.mark.parametrize("alpha", [0.0, 0.5, 0.6, 1.0])
@pytest.mark.parametrize("capacity", CAPS)
def test_sample_steps_equals_the_per_step_entries(dev, capacity, alpha):
    rng = np.random.default_rng(100 * CAPS.index(capacity) + int(10 * alpha))
    tree, n_valid = kernel_tree(dev, capacity, alpha, rng)
    leaves, r = tree.leaves(), draws(rng)
    before = tree.buffer().copy()
    for beta in (0.0, 0.4, 1.0):
        idx, w, wmax = sample_steps(tree, r, n_valid, beta)
        for s in range(STEPS):
            u = (r[s].astype(np.float32) * np.float32(2.0 ** -24))
            assert np.all(u < 1.0) and u.astype(np.float64).tolist() == (r[s] / R24).tolist()          # exact
            want_idx = tree.sample(u)
            want_w, want_max = tree.weights(want_idx, n_valid, beta)
            assert np.array_equal(idx[s], want_idx), (capacity, alpha, beta, s, np.flatnonzero(idx[s] != want_idx)[:5])
            assert np.array_equal(bits(w[s]), bits(want_w)), (capacity, alpha, beta, s)
            assert bits(wmax[s]) == bits(want_max) and wmax[s] == w[s].max()
        assert idx.min() >= 0 and idx.max() < n_valid and np.all(leaves[idx] > 0)                       # never a row with a zero leaf
        if beta == 0.0:
            assert np.all(w == 1.0) and np.all(wmax == 1.0)
        else:
            assert np.all(w > 0) and np.all(np.isfinite(w))
        again = sample_steps(tree, r, n_valid, beta)                                                    # a second call: the same bits
        assert np.array_equal(again[0], idx) and np.array_equal(bits(again[1]), bits(w)) and np.array_equal(bits(again[2]), bits(wmax))
    assert np.array_equal(bits(tree.buffer()), bits(before))                                            # the tree is only read


@pytest.mark.parametrize("capacity", CAPS)
def test_sample_steps_on_exactly_summable_priorities(dev, capacity):
    """alpha = 1, priorities k / 8 with k in 0..16 (zeros inside the valid range): every sum in the tree and every prefix is exact, and
    so is residual - prefix (both lie on t's own grid and the difference is no larger than t).  The row is then NumPy's
    searchsorted(cumsum, t, side="right") with t formed in fp32 by the written operations; where rounding pushes (k + u) seg to the
    total or past it -- k = b - 1 with u = 1 - 2^-24 gives (float)k + u = b -- no prefix exceeds it and the law's other branch, the
    last non-zero child at every level, gives the last row with a non-zero leaf."""
    rng = np.random.default_rng(capacity)
    tree = Tree(capacity, dev)
    n_valid = max(3, (2 * capacity) // 3)
    k8 = rng.integers(0, 17, size=n_valid)
    k8[0], k8[1] = 16, 0
    tree.update(np.arange(n_valid), (k8 / 8.0).astype(np.float32), 1.0, 0.0)
    model = np.zeros(capacity, dtype=np.float64)
    model[:n_valid] = k8 / 8.0
    assert np.array_equal(tree.leaves().astype(np.float64), model) and np.any(model[:n_valid] == 0)
    cum, total = np.cumsum(model), np.float32(model.sum())
    assert float(total) == model.sum()
    r = draws(rng)
    idx, w, wmax = sample_steps(tree, r, n_valid, 1.0)
    seg = total / np.float32(B_K)
    last = int(np.flatnonzero(model)[-1])
    hit_total = 0
    for s in range(STEPS):
        u = r[s].astype(np.float32) * np.float32(2.0 ** -24)
        t = (np.arange(B_K, dtype=np.float32) + u) * seg
        assert t.dtype == np.float32
        want = np.searchsorted(cum, t.astype(np.float64), side="right")
        hit_total += int(np.count_nonzero(want >= capacity))
        want = np.where(want >= capacity, last, want)
        assert np.array_equal(idx[s], want), (capacity, s, np.flatnonzero(idx[s] != want)[:5])
        x = (np.float32(n_valid) * model[idx[s]].astype(np.float32)) / total                          # fp32: one product, one division
        assert np.array_equal(bits(w[s]), bits(np.float32(1.0) / x)) and wmax[s] == w[s].max()
    assert np.all(model[idx] > 0)
    print(f"capacity {capacity}: {hit_total} of {STEPS * B_K} samples had t >= total")


# ------------------------------------------------------------------------------------------------ the learner
O, A, B, K = 8, 2, 256, 4
_rows = functools.partial(lh._rows, O, A)


def _learner(*extra, graph, cap, rows, seed=11):
    """A V-learner at the toy shape (obs 8, act 2, batch 256, K = 4 steps per run), a policy, statistics and `rows` rows in the ring."""
    from pql_amd.utils.cfg import load_cfg
    return lh._learner(lambda: load_cfg(["task.name=Toy", f"algo.batch_size={B}", f"algo.memory_size={cap}", "algo.v_learner_gpu=0", "algo.p_learner_gpu=0",
                                         "algo.num_gpus=1", f"algo.prefetch_steps={K}", f"algo.graph={graph}", *extra]), O, A, rows, seed)


def test_a_run_samples_from_the_tree_as_it_stood(dev):
    """One run graph of K = 4 steps: its rows and weights are the per-step entries applied to a clone of the tree taken before the
    run, with u = r 2^-24 of the draws made ahead and beta of the schedule at the run's first step; the tree keeps its bits until
    the flush."""
    from pql_amd.replay.prioritized_replay import PrioritizedReplayBuffer, per_beta
    v, actor, norm = _learner(*PER, "algo.per.beta_iters=16", graph=True, cap=4096, rows=1500)
    assert v.rng is not None and isinstance(v.memory, PrioritizedReplayBuffer) and v.memory.alpha == 0.5
    v.learn_many(K)                                     # a first run and a hand-off: the priorities are |TD|s and pmax now, not all 1
    assert v.rng == "philox" and v._run_graph is not None
    v.update(actor, _rows(300, 5, dev), norm, 0)
    torch.cuda.synchronize()
    n_valid = v.memory.cur_capacity
    assert n_valid == 1800 and v._per_pending == 0 and v.update_count == K
    before = Tree(4096, dev)
    before.tree.copy_(v.memory.tree)
    assert np.unique(before.leaves()[:n_valid]).size > 100 and np.all(before.leaves()[n_valid:] == 0)
    v.learn_many(K)
    torch.cuda.synchronize()
    assert v._per_pending == K and v.update_count == 2 * K
    assert torch.equal(v.memory.tree.view(torch.int32), before.tree.view(torch.int32))                 # frozen: nothing written back yet
    ws, r = v._ws, v._ahead.idx.cpu().numpy()
    assert r.shape == (K, B) and r.min() >= 0 and r.max() < R24 and r.max() > 1800
    beta = per_beta(0.4, 16, K)
    assert 0.4 < beta < 1.0
    for s in range(K):
        idx = before.sample(r[s].astype(np.float32) * np.float32(2.0 ** -24))
        w, wmax = before.weights(idx, n_valid, beta)
        assert np.array_equal(ws["per_idx_all"][s].cpu().numpy(), idx), s
        assert np.array_equal(bits(ws["w_all"][s].cpu().numpy()), bits(w)), s
        assert bits(ws["wmax_all"][s].item()) == bits(wmax)
        assert np.unique(w).size > 10
    assert bool((ws["abs_td_all"] > 0).any())
    v.flush_priorities()
    torch.cuda.synchronize()
    assert v._per_pending == 0 and not torch.equal(v.memory.tree, before.tree)


@pytest.mark.parametrize("graph", [False, True])
def test_write_back_then_insert(dev, graph):
    """A full ring of 2048 rows, so every insert overwrites: two runs, each followed by `update()` with 300 new rows.  After each the
    leaves are, bit for bit: the new rows pmax^alpha (rows sampled in the run among them: the flush comes before the insert), every
    other sampled row (max over its occurrences of |TD| + eps)^alpha from the slabs, the rest unchanged; pmax is the running maximum
    of |TD| + eps; and the upper levels are those of a rebuild.  alpha = 0.5: sqrtf is correctly rounded, so NumPy gives the bits."""
    cap, m = 2048, 300
    v, actor, norm = _learner(*PER, graph=graph, cap=cap, rows=cap)
    torch.cuda.synchronize()
    assert v.memory.cur_capacity == cap and v.memory.next_p == cap        # every row written, the pointer at the end: the next insert wraps to row 0
    leaves, pmax, eps = np.ones(cap, dtype=np.float32), np.float32(1.0), np.float32(1.0e-3)
    assert np.array_equal(v.memory.leaves.cpu().numpy(), leaves)
    for rnd in range(2):
        if graph:
            v.learn_many(K)
        else:
            for _ in range(K):
                v.learn()
        torch.cuda.synchronize()
        assert v.rng == "philox" and v._per_pending == K
        assert np.array_equal(bits(v.memory.leaves.cpu().numpy()), bits(leaves))                       # frozen until the flush
        idx, td = v._ws["per_idx_all"].cpu().numpy().reshape(-1), v._ws["abs_td_all"].cpu().numpy().reshape(-1)
        lo = rnd * m
        overwritten = np.count_nonzero((idx >= lo) & (idx < lo + m))
        assert overwritten > 0 and np.unique(idx).size < idx.size                                      # both cases are in the data
        v.update(actor, _rows(m, 20 + rnd, dev), norm, 0)
        torch.cuda.synchronize()
        p = td + eps
        leaves[idx] = 0
        np.maximum.at(leaves, idx, np.sqrt(p))
        pmax = max(pmax, p.max())
        leaves[lo: lo + m] = np.sqrt(pmax)
        assert np.float32(v.memory.pmax.item()) == pmax
        got = v.memory.tree.cpu().numpy()
        assert np.array_equal(bits(got[:cap]), bits(leaves)), (rnd, np.flatnonzero(got[:cap] != leaves)[:5])
        assert np.array_equal(bits(got), bits(model_tree(leaves)[0]))
        clone = Tree(cap, dev)
        clone.tree.copy_(v.memory.tree)
        clone.rebuild()
        assert np.array_equal(bits(clone.buffer()), bits(got))
    assert pmax > 1.0 or np.unique(leaves).size > 100


def test_modes_agree(dev):
    """Eager learn() x K, per-slot graphs and one run graph: two runs with an `update()` between leave the same arenas, Adam state,
    loss ring, tree and pmax."""
    ends = {}
    for mode in ("eager", "slots", "run"):
        v, actor, norm = _learner(*PER, graph=mode != "eager", cap=4096, rows=1500)
        for rnd in range(2):
            if mode == "run":
                v.learn_many(K)
            else:
                for _ in range(K):
                    v.learn()
            if rnd == 0:
                v.update(actor, _rows(300, 30, dev), norm, 0)
        assert v.rng == "philox" and v.update_count == 2 * K
        assert (len(v._slot_graphs), v._run_graph is not None) == {"eager": (0, False), "slots": (K, False), "run": (0, True)}[mode]
        ends[mode] = _state(v)
    _same_state(ends["eager"], ends["slots"])
    _same_state(ends["eager"], ends["run"])
    e = ends["eager"]
    assert e["tree"][:1800].unique().numel() > 100 and bool(torch.isfinite(e["loss_ring"]).all()) and int(e["adam_step"]) == 2 * K


def test_per_step_path_agrees_with_itself_under_a_graph(dev):
    """algo.rng=torch: one randint(2^24) + one sample launch in front of every step, the write-back behind it; eager == per-step graph."""
    ends = []
    for graph in (False, True):
        v, actor, norm = _learner(*PER, "algo.rng=torch", graph=graph, cap=4096, rows=1500)
        for _ in range(3):
            v.learn()
            assert v._per_pending == 0
        assert v.rng == "torch"
        ends.append(_state(v))
    _same_state(*ends)
    assert ends[0]["tree"][:1500].unique().numel() > 100


def test_hooks_change_nothing_else(dev):
    """alpha = 0 (every priority 1) and beta0 = 1: every weight is exactly 1, so on injected indices and noise the prioritized learner
    must leave the bits of a plain learner that takes the separate-loss sequence (td_in_head=False, td_in_forward=False)."""
    ends = []
    for extra in (("algo.per.enabled=True", "algo.per.refresh=run", "algo.per.alpha=0.0", "algo.per.beta0=1.0"),
                  ("algo.td_in_head=False", "algo.td_in_forward=False")):
        v, actor, norm = _learner(*extra, graph=False, cap=4096, rows=1500)
        g = torch.Generator().manual_seed(5)
        for _ in range(3):
            v.learn(indices=torch.randint(0, 1500, (B,), generator=g), noise=torch.randn((B, A), generator=g))
        st = _state(v)
        if "tree" in st:
            assert bool((st["tree"][:1500] == 1.0).all()) and bool((v._ws["w_all"][0] == 1.0).all()) and float(v._ws["wmax_all"][0]) == 1.0
            assert v._ws["td_parts"] == 0 and v._ws["td_fwd"] == 0
            st = {k: t for k, t in st.items() if k not in ("tree", "pmax")}
        ends.append(st)
    _same_state(*ends)
    assert int(ends[0]["adam_step"]) == 3


def test_resume_is_bit_exact_and_two_processes_agree(tmp_path):
    """scripts/train_pql.py with prioritized replay, a ring of 2500 rows (it wraps around iteration 10: inserts overwrite sampled
    rows).  A: 6000 steps; A2: the same in another process; B1: 3000 steps, checkpoint at stop; B2 (new process): resume, to 6000.
    A == A2 == B2, leaves and pmax included.  Each child runs under its own time limit; a failing one ends the test."""
    base = PQL_TOY + ["algo.graph=True", "algo.memory_size=2500", "algo.per.enabled=True", "algo.per.refresh=run", "algo.per.beta_iters=300"]
    keys = PQL_KEYS + ("per_sha", "per_pmax")
    a = child(PQL, base + ["max_step=6000"], tmp_path, timeout=120)
    assert a["per_sha"] and a["per_pmax"] > 0 and a["rollout_iterations"] == 62 and a["critic_updates"] == 8 * 62
    a2 = child(PQL, base + ["max_step=6000"], tmp_path, timeout=120)
    same(a, a2, keys)
    ck = tmp_path / "ck"
    b1 = child(PQL, base + ["max_step=3000", f"checkpoint.dir={ck}"], tmp_path, timeout=120)
    assert b1["rollout_iterations"] == 15 and b1["per_sha"] != a["per_sha"]
    b2 = child(PQL, base + ["max_step=6000", f"resume={ck}"], tmp_path, timeout=120)
    assert b2["resumed_from"]["global_steps"] == b1["global_steps"]
    same(a, b2, keys)


# ------------------------------------------------------------------------------------------------ it learns
def learning_bar():
    """(iterations, F_MIN) from the committed record profiles/per_pql_learning.json (tools/learn_pointmass.py --task swingup --algos pql
    --shapes small with the two overrides, seeds 0-4, on an MI355X): the smallest iteration count at which all five seeds reached
    f >= 0.2, and half of the lowest f recorded at that count -- the rule of the other learning tests (the yardsticks, zero action and
    energy controller, depend on no learner kernel; the half covers seed-to-seed and box-to-box spread)."""
    rec = json.load(open(os.path.join(ROOT, "profiles", "per_pql_learning.json")))
    by_iters = {}
    for r in rec["runs"] + rec["curve"]:
        if r["algo"] == "pql" and r["shape"] == "small" and r.get("task") == "swingup" and "algo.per.enabled=True" in r.get("overrides", []):
            by_iters.setdefault(int(r["iters"]), {})[int(r["seed"])] = float(r["f"])
    ok = sorted(n for n, f in by_iters.items() if set(f) >= {0, 1, 2, 3, 4} and min(f.values()) >= 0.2)
    assert ok, f"no iteration count in the record at which all five seeds have f >= 0.2: {by_iters}"
    return ok[0], 0.5 * min(by_iters[ok[0]].values())


def test_pql_with_prioritized_replay_learns_swingup():
    import task_cases as tc
    iters, f_min = learning_bar()
    lp = tc.load_script("tools/learn_pointmass.py", "learn_pointmass_per_pql")
    r = lp.run("pql", "small", 0, iters, ("algo.per.enabled=True", "algo.per.refresh=run"), task="swingup")
    print(f"swingup pql + prioritized replay, seed 0, {iters} iterations: R={r['R']:.3f} R_zero={r['R_zero']:.3f} R_ctrl={r['R_ctrl']:.3f} "
          f"f={r['f']:.4f} (bar {f_min:.4f}) wall={r['wall_s']}s")
    assert r["R_ctrl"] > r["R_zero"] and r["critic_updates"] == 8 * iters
    assert r["f"] >= f_min, r
