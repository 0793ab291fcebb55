#!/usr/bin/env python3
"""Per-step time of the V- and the P-learner with each of the three twin critics on one MI355X, at bench.py's shape (cfg #2):
`DoubleQ` (scalar heads: TD in the forward launch, fused DPG backward), C51 with 51 atoms (`algo.distl=True`) and
`QuantileDoubleQ` with 32 quantiles.  tools/kbench.py's variants switch settings of ONE learner pair; a critic class is a different
learner pair, so this builds the three systems in one process and times them in turn, ROUNDS times (cdna_hip_programming.md rule
24: deltas come from interleaved rounds in one process).  A point is kbench's `rate`: free-running `learn()` calls on the learner's
own stream (hipGraph replay), wall clock around a full device synchronise, best of three windows of --steps steps; the table and
the JSON hold median and min over the rounds.  Recorded, not gated.  GPU only.
--drop d [d ...] times the quantile critic alone: without `algo.qr_drop` and with each d (the truncated pooled target), in turn.

    python tools/bench_quantile.py [--out profiles/quantile_bench.json] [--rounds 5] [--steps 200] [bench.py flags ...]
    python tools/bench_quantile.py --drop 0 2 --out profiles/tqc_bench.json"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import bench  # noqa: E402

VARIANTS = {"DoubleQ": [], "C51 (51 atoms)": ["algo.distl=True", "algo.num_atoms=51"],
            "QuantileDoubleQ (N = 32)": ["algo.cri_class=QuantileDoubleQ", "algo.num_quantiles=32"]}


def rate(fn, n):
    """us per call of `fn` (kbench's): warmed, best of three windows of n calls, each ended by a device synchronise."""
    for _ in range(8):
        fn()
    torch.cuda.synchronize()
    best = 1e30
    for _ in range(3):
        t0 = time.perf_counter()
        for _ in range(n):
            fn()
        torch.cuda.synchronize()
        best = min(best, (time.perf_counter() - t0) / n * 1e6)
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--drop", type=int, nargs="+", default=None, help="time QuantileDoubleQ without algo.qr_drop and with each of these values")
    ns, rest = ap.parse_known_args()
    variants = VARIANTS
    if ns.drop is not None:
        name, qr = "QuantileDoubleQ (N = 32)", VARIANTS["QuantileDoubleQ (N = 32)"]
        variants = {name: qr, **{f"{name}, qr_drop = {d}": [*qr, f"algo.qr_drop={d}"] for d in ns.drop}}
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_quantile.py needs an MI355X (no CPU path)")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    systems = {}
    for name, override in variants.items():
        sys.argv = ["bench.py", "--no-cpu-baseline", *rest, *[x for o in override for x in ("--override", o)]]
        args = bench.parse()
        torch.manual_seed(42)
        cfg, env, actor, v, p = bench.build_system(args, 0, 1, dev, None)
        bench.prefill(actor, v, p, env, cfg, args, dev)
        v.learn(); p.learn()
        torch.cuda.synchronize()
        systems[name] = (cfg, v, p, actor, env)
        print(f"built {name}: head {v.critic.head}, out {v.critic.layout.dims[-1]}, td_fwd {v._ws['td_fwd']}, dpg_fused {p._ws['dpg_fused']}",
              file=sys.stderr, flush=True)
    res = {name: {"vstep": [], "pstep": []} for name in systems}
    for r in range(ns.rounds):
        for name, (cfg, v, p, _, _) in systems.items():
            res[name]["vstep"].append(rate(v.learn, ns.steps))
            res[name]["pstep"].append(rate(p.learn, ns.steps))
        print(f"round {r} done", file=sys.stderr, flush=True)
    cfg = next(iter(systems.values()))[0]
    print(f"{'critic':42s} {'vstep us (median / min)':>26s} {'pstep us (median / min)':>26s}")
    out = {"device": torch.cuda.get_device_name(dev), "batch": int(cfg.algo.batch_size), "hidden": list(cfg.algo.hidden_layers),
           "rounds": ns.rounds, "steps": ns.steps, "argv": rest, "unit": "us per learner step", "critics": {}}
    for name, r in res.items():
        row = {k: {"median": statistics.median(x), "min": min(x), "all": x} for k, x in r.items()}
        _, v, p, _, _ = systems[name]
        row["td_in_forward"], row["dpg_fused"] = bool(v._ws["td_fwd"] > 0), bool(p._ws["dpg_fused"])
        out["critics"][name] = row
        print(f"{name:42s} {row['vstep']['median']:14.1f} /{row['vstep']['min']:9.1f} {row['pstep']['median']:14.1f} /{row['pstep']['min']:9.1f}")
    if ns.out:
        with open(ns.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
