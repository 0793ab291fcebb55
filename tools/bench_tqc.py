#!/usr/bin/env python3
"""Per-update time of the TQC agent against SAC on one MI355X, at bench.py's shape (cfg #2: AllegroHand, batch 8192, hidden
512-512-256): `AgentSAC` with `DoubleQ` and `AgentTQC` with N = 25, d = 2 (the config's values) and with N = 32, d = 2 live in one
process and are timed in turn, ROUNDS times (cdna_hip_programming.md rule 24: deltas come from interleaved rounds in one process).
A point is tools/bench_quantile.py's `rate`: `update_once` calls drawing their own indices and eps, wall clock around a full device
synchronise, best of three windows of --steps calls; the table and the JSON hold median and min over the rounds.

In the same call: what fusing the entropy shift into the loss launch is worth.  `pqlk_tqc_huber_loss_soft` against "shift the
(2, B, N) target heads in torch, then `pqlk_tqc_huber_loss`" on the same buffers, at both N.  Recorded, not gated.  GPU only.
And `entries`: us per call of each of the eight quantile loss entries at B = 8192, N in (25, 32), d = 2 -- the point to compare two
builds of the library on (`PQLK_LIB=...`, a fresh process each).

    python tools/bench_tqc.py [--out profiles/tqc_sac_bench.json] [--rounds 5] [--steps 200] [--sections agents fusion entries]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch  # noqa: E402

from bench_quantile import rate  # noqa: E402

O, A, B, HIDDEN, ROWS = 88, 16, 8192, [512, 512, 256], 200_000
VARIANTS = {"SAC, DoubleQ": ["algo=sac_algo"],
            "TQC, N = 25, d = 2": ["algo=tqc_algo", "algo.num_quantiles=25", "algo.qr_drop=2"],
            "TQC, N = 32, d = 2": ["algo=tqc_algo", "algo.num_quantiles=32", "algo.qr_drop=2"]}


def build(override, dev):
    from pql_amd.algo import alg_name_to_path
    from pql_amd.envs.synthetic import create_task_env
    from pql_amd.replay.simple_replay import ReplayBuffer
    from pql_amd.utils.cfg import load_cfg
    from pql_amd.utils.common import load_class_from_path
    cfg = load_cfg([*override, "task.name=AllegroHand", "num_envs=64", f"algo.batch_size={B}", f"algo.memory_size={ROWS}", "device=cuda:0",
                    "sim_device=cuda:0"])
    cfg.algo.hidden_layers = list(HIDDEN)
    torch.manual_seed(42)
    name = "Agent" + cfg.algo.name
    agent = load_class_from_path(name, alg_name_to_path[name])(env=create_task_env(cfg), cfg=cfg)
    g = torch.Generator(device=dev).manual_seed(7)
    r = lambda *s: torch.rand(s, device=dev, generator=g) * 2.0 - 1.0   # noqa: E731
    memory = ReplayBuffer(ROWS, (O,), A, device=dev)
    memory.add_to_buffer((r(ROWS, O), r(ROWS, A), 0.05 * r(ROWS, 1), r(ROWS, O), (torch.rand((ROWS, 1), device=dev, generator=g) < 0.05).float()))
    return cfg, agent, memory


def fusion(dev, N, d, steps):
    """us per call: the soft loss launch vs an in-place torch shift of the target heads followed by the entry without the shift."""
    from pql_amd import _lib as L
    ld = L.ld(N)
    g = torch.Generator(device=dev).manual_seed(11)
    n = lambda *s: torch.randn(s, device=dev, generator=g)   # noqa: E731
    th, tt, rew, logp = n(2, B, ld), n(2, B, ld), n(B), n(B) - 1.0
    done = (torch.rand(B, device=dev, generator=g) < 0.1).float()
    la = torch.full((1,), -1.6, device=dev)
    dy, ring, step, scratch = torch.zeros(2, B, ld, device=dev), torch.zeros(5, device=dev), torch.zeros(1, dtype=torch.int32, device=dev), torch.zeros(2048, device=dev)
    head = (L.ptr(th), L.ptr(tt), ld, N, L.ptr(rew), L.ptr(done), 0.97, 1.0, B, L.ptr(dy), L.ptr(ring), L.ptr(step), 5, L.ptr(scratch))
    st = L.stream(dev)

    def fused():
        L.check(L.lib.pqlk_tqc_huber_loss_soft(*head, L.ptr(logp), L.ptr(la), d, st))

    def split():
        tt[:, :, :N].sub_((la.exp() * logp)[None, :, None])
        L.check(L.lib.pqlk_tqc_huber_loss(*head, d, st))

    def hard():
        L.check(L.lib.pqlk_tqc_huber_loss(*head, d, st))

    return {"N": N, "d": d, "soft_entry_us": rate(fused, steps), "torch_shift_then_plain_entry_us": rate(split, steps), "plain_entry_us": rate(hard, steps)}


def entries(dev, N, d, steps):
    """us per call of every quantile loss entry, each with a loss slot, on one set of buffers."""
    from pql_amd import _lib as L
    ld = L.ld(N)
    g = torch.Generator(device=dev).manual_seed(13)
    n = lambda *s: torch.randn(s, device=dev, generator=g)   # noqa: E731
    th, tt, rew, logp = n(2, B, ld), n(2, B, ld), n(B), n(B) - 1.0
    done = (torch.rand(B, device=dev, generator=g) < 0.1).float()
    w = torch.rand(B, device=dev, generator=g) * 0.95 + 0.05
    wmax, la, td = w.max().reshape(1), torch.full((1,), -1.6, device=dev), torch.zeros(B, device=dev)
    dy, ring, step, scratch = torch.zeros(2, B, ld, device=dev), torch.zeros(5, device=dev), torch.zeros(1, dtype=torch.int32, device=dev), torch.zeros(2048, device=dev)
    out = (B, L.ptr(dy), L.ptr(ring), L.ptr(step), 5, L.ptr(scratch))
    head = (L.ptr(th), L.ptr(tt), ld, N, L.ptr(rew), L.ptr(done), 0.97, 1.0, *out)
    per, soft, st = (L.ptr(w), L.ptr(wmax), L.ptr(td)), (L.ptr(logp), L.ptr(la)), L.stream(dev)
    calls = {"pqlk_qr_huber_loss": (*head, st), "pqlk_qr_huber_loss_per": (*head, *per, st), "pqlk_tqc_huber_loss": (*head, d, st),
             "pqlk_tqc_huber_loss_per": (*head, *per, d, st), "pqlk_tqc_huber_loss_soft": (*head, *soft, d, st),
             "pqlk_tqc_huber_loss_soft_per": (*head, *per, *soft, d, st), "pqlk_dpg_loss_quantile": (L.ptr(th), ld, N, *out, st),
             "pqlk_dpg_loss_quantile_mean": (L.ptr(th), ld, N, *out, st)}
    return {"N": N, "d": d, **{name: rate(lambda: L.check(getattr(L.lib, name)(*args)), steps) for name, args in calls.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sections", nargs="+", default=["agents", "fusion", "entries"], choices=["agents", "fusion", "entries"])
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=200)
    ns = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_tqc.py needs an MI355X (no CPU path)")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    systems = {name: build(ov, dev) for name, ov in VARIANTS.items()} if "agents" in ns.sections else {}
    res = {name: [] for name in systems}
    for r in range(ns.rounds):
        for name, (_, agent, memory) in systems.items():
            res[name].append(rate(lambda: agent.update_once(memory), ns.steps))
        print(f"round {r} done", file=sys.stderr, flush=True)
    out = {"device": torch.cuda.get_device_name(dev), "task": "AllegroHand", "batch": B, "hidden": HIDDEN, "rounds": ns.rounds, "steps": ns.steps,
           "unit": "us per update_once", "agents": {}, "fusion": [], "entries": []}
    if systems:
        print(f"{'agent':24s} {'update_once us (median / min)':>32s}")
    for name, x in res.items():
        out["agents"][name] = {"median": statistics.median(x), "min": min(x), "all": x}
        print(f"{name:24s} {statistics.median(x):20.1f} /{min(x):9.1f}")
    for N in (25, 32) if "fusion" in ns.sections else ():
        rows = [fusion(dev, N, 2, ns.steps) for _ in range(ns.rounds)]
        row = {"N": N, "d": 2, **{k: {"median": statistics.median(r[k] for r in rows), "min": min(r[k] for r in rows)}
                                  for k in ("soft_entry_us", "torch_shift_then_plain_entry_us", "plain_entry_us")}}
        out["fusion"].append(row)
        print(json.dumps(row))
    for N in (25, 32) if "entries" in ns.sections else ():   # us per call
        rows = [entries(dev, N, 2, ns.steps) for _ in range(ns.rounds)]
        row = {"N": N, "d": 2, **{k: {"median": statistics.median(r[k] for r in rows), "min": min(r[k] for r in rows)} for k in rows[0] if k.startswith("pqlk_")}}
        out["entries"].append(row)
        print(json.dumps(row))
    if ns.out:
        with open(ns.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
