#!/usr/bin/env python3
"""Timing of the skip-connection row kernels (pqlk_ln_res_forward / pqlk_ln_sum_backward, pql_amd/csrc/ln.hip) against their unfused
compositions, and of a DDPG update with the residual LayerNorm critic, on one MI355X.

ONE call, variants alternating inside every round (deltas between variants come from the same process and the same minutes):

  kernels   per-launch time at 8192 x {256, 512, 1024} and 32768 x 512: HIP events around `--launches` back-to-back calls, median and
            min over the rounds.
              res_forward            pqlk_ln_res_forward                                     (z, res in, y out: 3 M w 4 B)
              res_unfused            a LayerNorm row launch into a temporary plus a torch add (the row launch is
                                     pqlk_ln_elu_forward: the library has no activation-free LayerNorm entry of its own, and the
                                     traffic is the same)                                    (5 M w 4 B: z in, t out; res, t in, y out)
              elu_forward            pqlk_ln_elu_forward, the floor: one input row fewer     (2 M w 4 B)
              sum_backward           pqlk_ln_sum_backward(dy, dy2, y = NULL) -> dsum in place of dy2, dz in place of dy, with
                                     parameter gradients (two launches)                      (5 M w 4 B: dy, dy2, z in, dsum, dz out)
              sum_unfused            torch add into dy2, then the call without dy2 / dsum    (7 M w 4 B)
            The fraction of the 8 TB/s HBM peak comes from these ALGORITHMIC bytes.  At these sizes the tiles fit the 256 MB
            last-level cache, so a fraction above what HBM alone would allow is possible: a yardstick, not a traffic measurement.
  update    `AgentDDPG.update_once` at (obs 88, act 16), B = 8192, with `DoubleQ`, `DoubleQLayerNorm` (default hidden layers) and
            `DoubleQBroNet` (critic_width 512, critic_blocks 2): host clock around `--updates` updates that end in a device synchronise.

    python tools/bench_bro.py --out profiles/bro_bench.json
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import torch  # noqa: E402

from bench_ln import HBM_PEAK, make_agent, time_launches, time_updates  # noqa: E402
from pql_amd import _lib as L  # noqa: E402

KERNEL_SHAPES = [(8192, 256), (8192, 512), (8192, 1024), (32768, 512)]
CRITICS = ("DoubleQ", "DoubleQLayerNorm", "DoubleQBroNet")


def kernel_variants(dev):
    out = {}
    for m, w in KERNEL_SHAPES:
        f = dict(dtype=torch.float32, device=dev)
        z, res, dy, dy2 = (torch.randn((m, w), **f) for _ in range(4))
        y, tmp = torch.empty((m, w), **f), torch.empty((m, w), **f)
        gamma, beta = torch.rand(w, **f) + 0.5, torch.rand(w, **f) - 0.5
        mean, rstd = torch.empty(m, **f), torch.empty(m, **f)
        dg, db = torch.empty(w, **f), torch.empty(w, **f)
        scratch = torch.empty(int(L.lib.pqlk_ln_scratch_floats(w)), **f)
        st = L.stream(dev)
        p = L.ptr

        def res_forward(m=m, w=w, z=z, res=res, y=y, gamma=gamma, beta=beta, mean=mean, rstd=rstd, st=st):
            L.check(L.lib.pqlk_ln_res_forward(p(z), w, m, w, p(gamma), p(beta), 1e-5, p(res), p(y), p(mean), p(rstd), st))

        def elu_forward(dst=y, m=m, w=w, z=z, gamma=gamma, beta=beta, mean=mean, rstd=rstd, st=st):
            L.check(L.lib.pqlk_ln_elu_forward(p(z), w, m, w, p(gamma), p(beta), 1e-5, p(dst), p(mean), p(rstd), st))

        def res_unfused(res=res, y=y, tmp=tmp, row=elu_forward):
            row(dst=tmp)
            torch.add(res, tmp, out=y)

        def sum_backward(second=dy2, m=m, w=w, z=z, dy=dy, gamma=gamma, mean=mean, rstd=rstd, dg=dg, db=db, scratch=scratch, st=st):
            L.check(L.lib.pqlk_ln_sum_backward(p(dy), p(second), None, p(z), w, m, w, p(mean), p(rstd), p(gamma), p(second), p(dy), p(dg), p(db),
                                               p(scratch), st))

        def sum_unfused(dy=dy, dy2=dy2, m=m, w=w, z=z, gamma=gamma, mean=mean, rstd=rstd, dg=dg, db=db, scratch=scratch, st=st):
            torch.add(dy, dy2, out=dy2)
            L.check(L.lib.pqlk_ln_sum_backward(p(dy2), None, None, p(z), w, m, w, p(mean), p(rstd), p(gamma), None, p(dy), p(dg), p(db),
                                               p(scratch), st))

        def reset(dy=dy, dy2=dy2):   # the in-place variants feed their outputs back in: keep the values finite between rounds
            dy.normal_(); dy2.normal_()

        res_forward()
        n = m * w * 4
        out[(m, w, "res_forward")] = (res_forward, 3 * n, 1, reset)
        out[(m, w, "res_unfused")] = (res_unfused, 5 * n, 2, reset)
        out[(m, w, "elu_forward")] = (elu_forward, 2 * n, 1, reset)
        out[(m, w, "sum_backward")] = (sum_backward, 5 * n, 2, reset)
        out[(m, w, "sum_unfused")] = (sum_unfused, 7 * n, 3, reset)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--launches", type=int, default=100)
    ap.add_argument("--updates", type=int, default=30)
    ap.add_argument("--batch", type=int, default=8192)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_bro needs a GPU"
    torch.manual_seed(0)
    dev = torch.device("cuda:0")
    kv = kernel_variants(dev)
    agents = {c: make_agent(c, a.batch) for c in CRITICS}
    ktimes, utimes = {k: [] for k in kv}, {c: [] for c in agents}
    for r in range(a.rounds + 1):     # round 0 warms up
        for k, (fn, _, _, reset) in kv.items():
            reset()
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
        med, (_, nbytes, launches, _) = statistics.median(ts), kv[(m, w, what)]
        rec = dict(m=m, cols=w, what=what, launches_per_call=launches, us_median=round(med, 2), us_min=round(min(ts), 2),
                   algorithmic_bytes=nbytes, hbm_time_us=round(nbytes / HBM_PEAK * 1e6, 2), fraction_of_hbm_peak=round(nbytes / (med * 1e-6) / HBM_PEAK, 3))
        res["kernels"].append(rec)
        print(json.dumps(rec), flush=True)
    for c, ts in utimes.items():
        agent = agents[c][0]
        rec = dict(cri_class=c, obs_dim=88, act_dim=16, batch=a.batch, critic_params=int(agent.critic.num_params()) if hasattr(agent.critic, "num_params") else None,
                   us_median=round(statistics.median(ts), 1), us_min=round(min(ts), 1))
        res["update_once"].append(rec)
        print(json.dumps(rec), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
