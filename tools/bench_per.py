#!/usr/bin/env python3
"""Timing of prioritized replay (pql_amd/csrc/per.hip) beside uniform replay, on one MI355X.

ONE call, variants alternating inside every round (differences come from the same process and the same minutes):

  calls     us per call, HIP events around `--launches` back-to-back calls, median and min over the rounds, at B = 8192 over rings of
            1 M and 5 M rows whose priorities are (|td| + eps)^0.6 of random |td|:
              insert          pqlk_per_insert of 4096 rows (1 + levels - 1 launches)
              sample_weights  torch.rand + pqlk_per_sample + pqlk_per_weights (what PrioritizedReplayBuffer.draw_indices issues)
              loss_per        pqlk_td_mse_loss_per (2 launches)
              update          pqlk_per_update (2 + levels - 1 launches)
              randint         torch.randint (what ReplayBuffer.draw_indices issues)
              loss            pqlk_td_mse_loss (2 launches)
            `added_us` = sample_weights + loss_per + update - randint - loss: what a learner step pays for priorities.
  update    `AgentDDPG.update_once` at (obs 88, act 16), B = 8192, default hidden layers, ring of 1 M rows, with `ReplayBuffer` and
            with `PrioritizedReplayBuffer`: host clock around `--updates` updates that end in a device synchronise.

    python tools/bench_per.py --out profiles/per_bench.json

`--pql`: prioritized replay in the PQL V-learner (`algo.per.refresh=run`) instead, measured the same way:

  calls     at 8 steps x B = 8192 over the same rings: `sample_steps` (ONE pqlk_per_sample_steps) against `per_step_pairs`
            (8 x (pqlk_per_sample + pqlk_per_weights) on given u).
  learn_many  `PQLVLearner.learn_many(8)` at BASELINE configs[1] (obs 88, act 16, B = 8192, hidden [512, 512, 256], ring of 1 M rows,
            hipGraph per run), us per step, host clock around `--updates` runs that end in a device synchronise, three learners:
              uniform           the shipped configuration
              uniform_separate  uniform with algo.td_in_head=False algo.td_in_forward=False: the launch sequence the prioritized step takes
              prioritized       algo.per.enabled=True algo.per.refresh=run (one flush + one sample launch per run ride in the figure)
            uniform_separate - uniform is what leaving the fused TD head costs, prioritized - uniform_separate what the priorities cost.

    python tools/bench_per.py --pql --out profiles/per_pql_bench.json
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

from pql_amd import _lib as L  # noqa: E402

RINGS = [1_000_000, 5_000_000]
ALPHA, BETA, EPS, INSERT_ROWS = 0.6, 0.4, 1.0e-6, 4096


def call_variants(capacity, B, dev):
    f = dict(dtype=torch.float32, device=dev)
    lib, st = L.lib, L.stream(dev)
    tree = torch.zeros(int(lib.pqlk_per_tree_floats(capacity)), **f)
    pmax = torch.ones(1, **f)
    L.check(lib.pqlk_per_insert(L.ptr(tree), capacity, L.ptr(pmax), 0, capacity, ALPHA, st))
    rows, td0 = torch.arange(capacity, device=dev), torch.rand(capacity, **f).pow_(4) * 10
    L.check(lib.pqlk_per_update(L.ptr(tree), capacity, L.ptr(pmax), L.ptr(rows), L.ptr(td0), capacity, EPS, ALPHA, st))
    idx, w, wmax, td = torch.empty(B, dtype=torch.int64, device=dev), torch.empty(B, **f), torch.zeros(1, **f), torch.empty(B, **f)
    q, qt, dy = torch.randn((2, B, 32), **f), torch.randn((2, B, 32), **f), torch.zeros((2, B, 32), **f)
    rew, done = torch.randn(B, **f), (torch.rand(B, **f) < 0.1).float()
    ring, scratch = torch.zeros(5, **f), torch.zeros(2048, **f)
    head = (L.ptr(q), L.ptr(qt), 32, L.ptr(rew), L.ptr(done), 0.97, B, L.ptr(dy), L.ptr(ring), None, 5, L.ptr(scratch))
    state = {"p": 0}

    def insert():
        p = state["p"]
        L.check(lib.pqlk_per_insert(L.ptr(tree), capacity, L.ptr(pmax), p, INSERT_ROWS, ALPHA, st))
        state["p"] = (p + INSERT_ROWS) % (capacity - INSERT_ROWS)

    def sample_weights():
        u = torch.rand(B, device=dev)
        L.check(lib.pqlk_per_sample(L.ptr(tree), capacity, L.ptr(u), B, L.ptr(idx), st))
        L.check(lib.pqlk_per_weights(L.ptr(tree), capacity, L.ptr(idx), B, capacity, BETA, L.ptr(w), L.ptr(wmax), st))

    def loss_per():
        L.check(lib.pqlk_td_mse_loss_per(*head, L.ptr(w), L.ptr(wmax), L.ptr(td), st))

    def update():
        L.check(lib.pqlk_per_update(L.ptr(tree), capacity, L.ptr(pmax), L.ptr(idx), L.ptr(td), B, EPS, ALPHA, st))

    def randint():
        torch.randint(capacity, size=(B,), device=dev)

    def loss():
        L.check(lib.pqlk_td_mse_loss(*head, st))

    sample_weights(); loss_per()   # idx, w and td hold real values before anything is timed
    keep = (tree, pmax, rows, td0, idx, w, wmax, td, q, qt, dy, rew, done, ring, scratch)
    return dict(insert=insert, sample_weights=sample_weights, loss_per=loss_per, update=update, randint=randint, loss=loss), keep


def steps_variants(capacity, B, steps, dev):
    """One launch for `steps` batches against `steps` pairs of the per-step entries, on the same tree and the same draws."""
    f = dict(dtype=torch.float32, device=dev)
    lib, st = L.lib, L.stream(dev)
    tree = torch.zeros(int(lib.pqlk_per_tree_floats(capacity)), **f)
    pmax = torch.ones(1, **f)
    rows, td0 = torch.arange(capacity, device=dev), torch.rand(capacity, **f).pow_(4) * 10
    L.check(lib.pqlk_per_update(L.ptr(tree), capacity, L.ptr(pmax), L.ptr(rows), L.ptr(td0), capacity, EPS, ALPHA, st))
    r = torch.randint(1 << 24, (steps, B), device=dev)
    u = r.float() * 2.0 ** -24
    idx, w = torch.empty((steps, B), dtype=torch.int64, device=dev), torch.empty((steps, B), **f)
    wmax = torch.zeros(steps, **f)

    def sample_steps():
        L.check(lib.pqlk_per_sample_steps(L.ptr(tree), capacity, L.ptr(r), B, steps, capacity, BETA, L.ptr(idx), L.ptr(w), L.ptr(wmax), st))

    def per_step_pairs():
        for s in range(steps):
            L.check(lib.pqlk_per_sample(L.ptr(tree), capacity, L.ptr(u[s]), B, L.ptr(idx[s]), st))
            L.check(lib.pqlk_per_weights(L.ptr(tree), capacity, L.ptr(idx[s]), B, capacity, BETA, L.ptr(w[s]), L.ptr(wmax[s:s + 1]), st))

    return dict(sample_steps=sample_steps, per_step_pairs=per_step_pairs), (tree, pmax, rows, td0, r, u, idx, w, wmax)


V_VARIANTS = {"uniform": (), "uniform_separate": ("algo.td_in_head=False", "algo.td_in_forward=False"),
              "prioritized": ("algo.per.enabled=True", "algo.per.refresh=run")}


def make_v_learner(extra, batch, rows, steps):
    from pql_amd.algo.learner import make_actor
    from pql_amd.algo.pql_v_learner import PQLVLearner
    from pql_amd.utils.cfg import load_cfg
    O, A = 88, 16
    cfg = load_cfg(["task.name=AllegroHand", "num_envs=64", f"algo.batch_size={batch}", f"algo.memory_size={rows}", "algo.v_learner_gpu=0",
                    "algo.p_learner_gpu=0", "algo.num_gpus=1", "algo.graph=True", f"algo.prefetch_steps={steps}",
                    "algo.hidden_layers=[512,512,256]", *extra])
    v = PQLVLearner((O,), A, cfg)
    dev = v.device
    actor = make_actor(cfg, (O,), A, dev)
    norm = (torch.zeros(O, device=dev), torch.ones(O, device=dev), 1e-4)
    chunk = 250_000
    for _ in range(rows // chunk):
        v.update(actor, (torch.randn((chunk, O), device=dev), torch.rand((chunk, A), device=dev) * 2 - 1, torch.randn((chunk, 1), device=dev) * 0.05,
                         torch.randn((chunk, O), device=dev), (torch.rand((chunk, 1), device=dev) < 0.1).float()), norm, 0)
    v.prepare()
    return v


def time_runs(v, steps, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        v.learn_many(steps)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / (n * steps) * 1e6   # us per step


def main_pql(a):
    steps, dev = 8, torch.device("cuda:0")
    variants, keep = {}, []
    for cap in RINGS:
        fns, k = steps_variants(cap, a.batch, steps, dev)
        keep.append(k)
        variants.update({(cap, name): fn for name, fn in fns.items()})
    learners = {name: make_v_learner(extra, a.batch, RINGS[0], steps) for name, extra in V_VARIANTS.items()}
    ctimes, vtimes = {k: [] for k in variants}, {k: [] for k in learners}
    for r in range(a.rounds + 1):     # round 0 warms up (and gives the prioritized learner's tree real |TD|s)
        for k, fn in variants.items():
            t = time_launches(fn, a.launches)
            if r:
                ctimes[k].append(t)
        for k, v in learners.items():
            t = time_runs(v, steps, a.updates)
            if r:
                vtimes[k].append(t)
    res = dict(device=torch.cuda.get_device_name(0), torch=torch.__version__, rounds=a.rounds, launches=a.launches, runs=a.updates, steps=steps,
               batch=a.batch, alpha=ALPHA, beta=BETA, calls=[], learn_many=[])
    for (cap, name), ts in ctimes.items():
        rec = dict(ring_rows=cap, levels=int(L.lib.pqlk_per_levels(cap)), what=name, us_median=round(statistics.median(ts), 2), us_min=round(min(ts), 2))
        res["calls"].append(rec)
        print(json.dumps(rec), flush=True)
    for k, ts in vtimes.items():
        rec = dict(variant=k, overrides=list(V_VARIANTS[k]), rng=learners[k].rng, ring_rows=RINGS[0], obs_dim=88, act_dim=16, batch=a.batch,
                   us_per_step_median=round(statistics.median(ts), 1), us_per_step_min=round(min(ts), 1))
        res["learn_many"].append(rec)
        print(json.dumps(rec), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


def time_launches(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / n * 1e3   # us per call


def make_agent(prioritized, batch, rows):
    from pql_amd.algo.ddpg import AgentDDPG
    from pql_amd.envs.synthetic import create_task_env
    from pql_amd.replay.prioritized_replay import PrioritizedReplayBuffer
    from pql_amd.replay.simple_replay import ReplayBuffer
    from pql_amd.utils.cfg import load_cfg
    O, A = 88, 16
    cfg = load_cfg(["algo=ddpg_algo", "task.name=AllegroHand", "num_envs=64", f"algo.batch_size={batch}", f"algo.memory_size={rows}",
                    "device=cuda:0", "sim_device=cuda:0", f"algo.per.enabled={prioritized}"])
    agent = AgentDDPG(create_task_env(cfg), cfg)
    dev = agent.device
    memory = PrioritizedReplayBuffer(rows, (O,), A, device=dev, alpha=ALPHA, eps=EPS) if prioritized else ReplayBuffer(rows, (O,), A, device=dev)
    chunk = 250_000
    for _ in range(rows // chunk):
        memory.add_to_buffer((torch.randn((chunk, O), device=dev), torch.rand((chunk, A), device=dev) * 2 - 1, torch.randn((chunk, 1), device=dev) * 0.05,
                              torch.randn((chunk, O), device=dev), (torch.rand((chunk, 1), device=dev) < 0.1).float()))
    return agent, memory


def time_updates(agent, memory, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        agent.update_once(memory)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--updates", type=int, default=50)
    ap.add_argument("--batch", type=int, default=8192)
    ap.add_argument("--pql", action="store_true", help="the PQL V-learner's run-frozen prioritized replay instead (see the module's text)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_per needs a GPU"
    torch.manual_seed(0)
    if a.pql:
        return main_pql(a)
    dev = torch.device("cuda:0")
    variants = {}
    keep = []
    for cap in RINGS:
        fns, k = call_variants(cap, a.batch, dev)
        keep.append(k)
        variants.update({(cap, name): fn for name, fn in fns.items()})
    agents = {name: make_agent(name == "prioritized", a.batch, RINGS[0]) for name in ("uniform", "prioritized")}
    ctimes, utimes = {k: [] for k in variants}, {k: [] for k in agents}
    for r in range(a.rounds + 1):     # round 0 warms up
        for k, fn in variants.items():
            t = time_launches(fn, a.launches)
            if r:
                ctimes[k].append(t)
        for k, (agent, memory) in agents.items():
            t = time_updates(agent, memory, a.updates)
            if r:
                utimes[k].append(t)
    res = dict(device=torch.cuda.get_device_name(0), torch=torch.__version__, rounds=a.rounds, launches=a.launches, updates=a.updates,
               batch=a.batch, alpha=ALPHA, beta=BETA, insert_rows=INSERT_ROWS, calls=[], added=[], update_once=[])
    med = {}
    for (cap, name), ts in ctimes.items():
        med[(cap, name)] = statistics.median(ts)
        rec = dict(ring_rows=cap, levels=int(L.lib.pqlk_per_levels(cap)), what=name, us_median=round(med[(cap, name)], 2), us_min=round(min(ts), 2))
        res["calls"].append(rec)
        print(json.dumps(rec), flush=True)
    for cap in RINGS:
        m = lambda name: med[(cap, name)]  # noqa: E731
        rec = dict(ring_rows=cap, prioritized_us=round(m("sample_weights") + m("loss_per") + m("update"), 2), uniform_us=round(m("randint") + m("loss"), 2),
                   added_us=round(m("sample_weights") + m("loss_per") + m("update") - m("randint") - m("loss"), 2), insert_us=round(m("insert"), 2))
        res["added"].append(rec)
        print(json.dumps(rec), flush=True)
    for k, ts in utimes.items():
        rec = dict(replay=k, ring_rows=RINGS[0], obs_dim=88, act_dim=16, batch=a.batch, us_median=round(statistics.median(ts), 1), us_min=round(min(ts), 1))
        res["update_once"].append(rec)
        print(json.dumps(rec), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
