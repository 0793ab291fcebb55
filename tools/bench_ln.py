#!/usr/bin/env python3
"""Timing of the LayerNorm + ELU pair (pql_amd/csrc/ln.hip) and of a DDPG update with the LayerNorm critic, on one MI355X.

ONE call, variants alternating inside every round (deltas between variants come from the same process and the same minutes):

  kernels   per-launch time of pqlk_ln_elu_forward and pqlk_ln_elu_backward (with parameter gradients: two launches) at
            8192 x {128, 256, 512} and 32768 x 512: HIP events around `--launches` back-to-back launches, median and min over the
            rounds; the fraction of the 8 TB/s HBM peak from ALGORITHMIC bytes (forward 2 M w 4 B: z in, y out; backward 4 M w 4 B:
            dy, y, z in, dz out).  At these sizes the tiles fit the 256 MB last-level cache, so a fraction above what HBM alone
            would allow is possible: it is a yardstick, not a traffic measurement.
  update    `AgentDDPG.update_once` at (obs 88, act 16), B = 8192, default hidden layers, with `DoubleQ` and with
            `DoubleQLayerNorm`: host clock around `--updates` updates that end in a device synchronise.

    python tools/bench_ln.py --out profiles/ln_bench.json
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

HBM_PEAK = 8.0e12
KERNEL_SHAPES = [(8192, 128), (8192, 256), (8192, 512), (32768, 512)]


def kernel_variants(dev):
    out = {}
    for m, w in KERNEL_SHAPES:
        f = dict(dtype=torch.float32, device=dev)
        z, dy = torch.randn((m, w), **f), torch.randn((m, w), **f)
        y, dz = torch.empty((m, w), **f), torch.empty((m, w), **f)
        gamma, beta = torch.rand(w, **f) + 0.5, torch.rand(w, **f) - 0.5
        mean, rstd = torch.empty(m, **f), torch.empty(m, **f)
        dg, db = torch.empty(w, **f), torch.empty(w, **f)
        scratch = torch.empty(int(L.lib.pqlk_ln_scratch_floats(w)), **f)
        st = L.stream(dev)
        keep = (z, dy, y, dz, gamma, beta, mean, rstd, dg, db, scratch)

        def fwd(z=z, y=y, gamma=gamma, beta=beta, mean=mean, rstd=rstd, m=m, w=w, st=st, keep=keep):
            L.check(L.lib.pqlk_ln_elu_forward(L.ptr(z), w, m, w, L.ptr(gamma), L.ptr(beta), 1e-5, L.ptr(y), L.ptr(mean), L.ptr(rstd), st))

        def bwd(z=z, y=y, dy=dy, dz=dz, gamma=gamma, mean=mean, rstd=rstd, dg=dg, db=db, scratch=scratch, m=m, w=w, st=st):
            L.check(L.lib.pqlk_ln_elu_backward(L.ptr(dy), L.ptr(y), L.ptr(z), w, m, w, L.ptr(mean), L.ptr(rstd), L.ptr(gamma), L.ptr(dz),
                                               L.ptr(dg), L.ptr(db), L.ptr(scratch), st))

        def bwd_frozen(z=z, y=y, dy=dy, dz=dz, gamma=gamma, mean=mean, rstd=rstd, m=m, w=w, st=st):
            L.check(L.lib.pqlk_ln_elu_backward(L.ptr(dy), L.ptr(y), L.ptr(z), w, m, w, L.ptr(mean), L.ptr(rstd), L.ptr(gamma), L.ptr(dz),
                                               None, None, None, st))

        fwd()
        out[(m, w, "forward")] = (fwd, 2 * m * w * 4)
        out[(m, w, "backward")] = (bwd, 4 * m * w * 4)
        out[(m, w, "backward_frozen")] = (bwd_frozen, 4 * m * w * 4)
    return out


def time_launches(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / n * 1e3   # us per call


def make_agent(cri_class, batch):
    from pql_amd.algo.ddpg import AgentDDPG
    from pql_amd.envs.synthetic import create_task_env
    from pql_amd.replay.simple_replay import ReplayBuffer
    from pql_amd.utils.cfg import load_cfg
    O, A, rows = 88, 16, 4 * batch
    cfg = load_cfg(["algo=ddpg_algo", "task.name=AllegroHand", "num_envs=64", f"algo.batch_size={batch}", f"algo.memory_size={rows}",
                    "device=cuda:0", "sim_device=cuda:0", f"algo.cri_class={cri_class}"])
    agent = AgentDDPG(create_task_env(cfg), cfg)
    dev = agent.device
    memory = ReplayBuffer(rows, (O,), A, device=dev)
    memory.add_to_buffer((torch.randn((rows, O), device=dev), torch.rand((rows, A), device=dev) * 2 - 1, torch.randn((rows, 1), device=dev) * 0.05,
                          torch.randn((rows, O), device=dev), (torch.rand((rows, 1), device=dev) < 0.1).float()))
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
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_ln needs a GPU"
    torch.manual_seed(0)
    dev = torch.device("cuda:0")
    kv = kernel_variants(dev)
    agents = {c: make_agent(c, a.batch) for c in ("DoubleQ", "DoubleQLayerNorm")}
    ktimes, utimes = {k: [] for k in kv}, {c: [] for c in agents}
    for r in range(a.rounds + 1):     # round 0 warms up
        for k, (fn, _) in kv.items():
            t = time_launches(fn, a.launches)
            if r:
                ktimes[k].append(t)
        for c, (agent, memory) in agents.items():
            t = time_updates(agent, memory, a.updates)
            if r:
                utimes[c].append(t)
    res = dict(device=torch.cuda.get_device_name(0), torch=torch.__version__, rounds=a.rounds, launches=a.launches, updates=a.updates,
               hbm_peak_bytes_per_s=HBM_PEAK, kernels=[], update_once=[])
    for (m, w, what), ts in ktimes.items():
        med, nbytes = statistics.median(ts), kv[(m, w, what)][1]
        rec = dict(m=m, cols=w, what=what, launches_per_call=2 if what == "backward" else 1, us_median=round(med, 2), us_min=round(min(ts), 2),
                   algorithmic_bytes=nbytes, hbm_time_us=round(nbytes / HBM_PEAK * 1e6, 2), fraction_of_hbm_peak=round(nbytes / (med * 1e-6) / HBM_PEAK, 3))
        res["kernels"].append(rec)
        print(json.dumps(rec), flush=True)
    for c, ts in utimes.items():
        rec = dict(cri_class=c, obs_dim=88, act_dim=16, batch=a.batch, us_median=round(statistics.median(ts), 1), us_min=round(min(ts), 1))
        res["update_once"].append(rec)
        print(json.dumps(rec), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
