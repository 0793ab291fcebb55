#!/usr/bin/env python3
"""Timing of the exploration-noise launches (pql_amd/csrc/rollout.hip, pql_amd/csrc/noise.hip) and of a rollout iteration, on one
MI355X.

ONE call, variants alternating inside every round (deltas between variants come from the same process and the same minutes):

  kernels   per-launch time of pqlk_action_noise (white) and of pqlk_action_noise_colored with R = 1, 6 and 8 AR(1) states per action
            on the same act / sigma / out buffers, at 4096 x 16 and 16384 x 21: HIP events around `--launches` back-to-back launches,
            median and min over the rounds, and the algorithmic bytes of one launch (act in, out out, the draw in, the state in and
            out, one sigma and one flag per row).  Launches this small are bound by launch latency, not by bytes.
  draw      the `normal_` that feeds each of them, (rows, R * cols), timed the same way: pink's cost beyond the launch.
  rollout   `PQLActor.explore_env(env, 1, random=False)` on PointMass at (obs 88, act 16), 4096 envs, with algo.noise.color = white,
            ar1 and pink: host clock around `--iters` iterations that end in a device synchronise.  The white line is the figure to
            hold against the same command on another commit.

    python tools/bench_noise.py --out profiles/noise_bench.json
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

KERNEL_SHAPES = [(4096, 16), (16384, 21)]
OCTAVES = (1, 6, 8)
COLORS = ("white", "ar1", "pink")


def kernel_variants(dev):
    """{(rows, cols, name): (launch, algorithmic bytes)} and {(rows, cols, R): the draw of that shape}."""
    f = dict(dtype=torch.float32, device=dev)
    out, draws = {}, {}
    st = L.stream(dev)
    colored = getattr(L.lib, "pqlk_action_noise_colored", None)   # (absent on a commit before the entry: the white lines still run)
    for rows, cols in KERNEL_SHAPES:
        act, res = torch.rand((rows, cols), **f) * 2 - 1, torch.empty((rows, cols), **f)
        std = torch.linspace(0.05, 0.8, rows).to(dev)
        fresh = (torch.rand(rows, device=dev) < 0.02).to(torch.uint8)
        d1 = torch.randn((rows, cols), **f)

        def white(act=act, d1=d1, std=std, res=res, rows=rows, cols=cols):
            L.check(L.lib.pqlk_action_noise(L.ptr(act), L.ptr(d1), L.ptr(std), 0.0, rows, cols, -1.0, 1.0, L.ptr(res), st))

        out[(rows, cols, "white")] = (white, 4 * (3 * rows * cols + rows))
        for R in OCTAVES:
            G = 8 if R == 1 else 1
            rho, draw = torch.rand((G, R), **f) * 0.95, torch.randn((rows, R * cols), **f)
            coef = torch.sqrt(1 - rho.double() ** 2).float()
            state = torch.randn((rows, R, cols), **f)
            w = float(torch.tensor(R ** -0.5, dtype=torch.float32))

            def colour(act=act, draw=draw, std=std, rho=rho, coef=coef, G=G, R=R, fresh=fresh, state=state, w=w, res=res, rows=rows, cols=cols):
                L.check(colored(L.ptr(act), L.ptr(draw), L.ptr(std), 0.0, L.ptr(rho), L.ptr(coef), G, R, 0, L.ptr(fresh), L.ptr(state), rows,
                                cols, w, -1.0, 1.0, L.ptr(res), st))

            if colored is not None:
                out[(rows, cols, f"colored_R{R}")] = (colour, 4 * (2 * rows * cols + 3 * R * rows * cols + rows) + rows)
            draws[(rows, cols, R)] = torch.empty((rows, R * cols), **f)
    for fn, _ in out.values():
        fn()
    return out, draws


def time_launches(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / n * 1e3   # us per call


def make_rollout(color, num_envs):
    from pql_amd.algo.learner import make_actor
    from pql_amd.algo.pql_actor import PQLActor
    from pql_amd.envs.synthetic import create_task_env
    from pql_amd.utils.cfg import load_cfg
    from pql_amd.utils.common import set_random_seed
    extra = [] if color == "white" else [f"algo.noise.color={color}"]   # (white: the command also runs on a commit before the key)
    cfg = load_cfg(["task=pointmass", "task.obs_dim=88", "task.act_dim=16", f"num_envs={num_envs}", "algo.v_learner_gpu=0", "algo.p_learner_gpu=0",
                    "algo.num_gpus=1", "sim_device=cuda:0", "device=cuda:0", *extra])
    set_random_seed(0)
    env = create_task_env(cfg)
    actor = PQLActor(env, cfg)
    actor.set_actor(make_actor(cfg, env.observation_space.shape, env.action_space.shape[0], actor.sim_device))
    actor.reset_agent()
    actor.explore_env(env, cfg.algo.warm_up, random=True)   # as the training loop: fills the n-step window
    return actor, env


def time_rollout(actor, env, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        actor.explore_env(env, 1, random=False)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--launches", type=int, default=500)
    ap.add_argument("--iters", type=int, default=300)
    ap.add_argument("--num-envs", type=int, default=4096)
    ap.add_argument("--colors", default=",".join(COLORS), help="the rollout variants (white alone runs on any commit)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_noise needs a GPU"
    torch.manual_seed(0)
    dev = torch.device("cuda:0")
    kv, draws = kernel_variants(dev)
    rollouts = {c: make_rollout(c, a.num_envs) for c in a.colors.split(",")}
    ktimes, dtimes, rtimes = {k: [] for k in kv}, {k: [] for k in draws}, {c: [] for c in rollouts}
    for r in range(a.rounds + 1):     # round 0 warms up
        for k, (fn, _) in kv.items():
            t = time_launches(fn, a.launches)
            if r:
                ktimes[k].append(t)
        for k, buf in draws.items():
            t = time_launches(buf.normal_, a.launches)
            if r:
                dtimes[k].append(t)
        for c, (actor, env) in rollouts.items():
            t = time_rollout(actor, env, a.iters)
            if r:
                rtimes[c].append(t)
    res = dict(device=torch.cuda.get_device_name(0), torch=torch.__version__, rounds=a.rounds, launches=a.launches, iters=a.iters, kernels=[],
               draws=[], rollout_iteration=[])
    for (rows, cols, name), ts in ktimes.items():
        rec = dict(rows=rows, cols=cols, launch=name, us_median=round(statistics.median(ts), 2), us_min=round(min(ts), 2),
                   algorithmic_bytes=kv[(rows, cols, name)][1])
        res["kernels"].append(rec)
        print(json.dumps(rec), flush=True)
    for (rows, cols, R), ts in dtimes.items():
        rec = dict(rows=rows, cols=R * cols, octaves=R, us_median=round(statistics.median(ts), 2), us_min=round(min(ts), 2))
        res["draws"].append(rec)
        print(json.dumps(rec), flush=True)
    for c, ts in rtimes.items():
        rec = dict(color=c, task="pointmass", obs_dim=88, act_dim=16, num_envs=a.num_envs, us_median=round(statistics.median(ts), 1),
                   us_min=round(min(ts), 1), us_all=[round(t, 1) for t in ts])
        res["rollout_iteration"].append(rec)
        print(json.dumps(rec), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
