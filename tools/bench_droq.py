#!/usr/bin/env python3
"""What the in-kernel dropout mask costs: pqlk_drop_ln_elu_forward / _backward (pql_amd/csrc/ln.hip) at p = 0.01 against the plain
pqlk_ln_elu_forward / _backward launches ON THE SAME BUFFERS, on one MI355X.

ONE call, the variants alternating inside every round (a ratio comes from the same process and the same minutes), timed as
tools/bench_ln.py times its launches: HIP events around `--launches` back-to-back launches, median and min over the rounds.
Shapes (8192, 512), (8192, 256) -- the register paths of the default critic widths -- and (8192, 1025), the strided path, which
re-forms the mask once per pass over the row.  forward; backward with parameter gradients (two launches); backward without.
The yardstick is the plain LayerNorm launch; the ratio drop / plain is recorded, not gated.

    python tools/bench_droq.py --out profiles/droq_bench.json
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

from pql_amd import _lib as L  # noqa: E402

SHAPES = [(8192, 512), (8192, 256), (8192, 1025)]
P, SEED, TAG = 0.01, 0x9E3779B97F4A7C15, (3 << 8) | (1 << 4) | 1


def variants(dev):
    out = {}
    for m, w in SHAPES:
        f = dict(dtype=torch.float32, device=dev)
        ld = L.ld(w)
        z, dy = torch.randn((m, ld), **f), torch.randn((m, ld), **f)
        y, dz = torch.zeros((m, ld), **f), torch.zeros((m, ld), **f)
        gamma, beta = torch.rand(ld, **f) + 0.5, torch.rand(ld, **f) - 0.5
        mean, rstd = torch.empty(m, **f), torch.empty(m, **f)
        dg, db = torch.empty(w, **f), torch.empty(w, **f)
        scratch = torch.empty(int(L.lib.pqlk_ln_scratch_floats(w)), **f)
        st = L.stream(dev)
        keep = (z, dy, y, dz, gamma, beta, mean, rstd, dg, db, scratch)
        fa = (L.ptr(z), ld, m, w, L.ptr(gamma), L.ptr(beta), 1e-5)
        fo = (L.ptr(y), L.ptr(mean), L.ptr(rstd), st)
        ba = (L.ptr(dy), L.ptr(y), L.ptr(z), ld, m, w, L.ptr(mean), L.ptr(rstd), L.ptr(gamma))
        bo = {"backward": (L.ptr(dz), L.ptr(dg), L.ptr(db), L.ptr(scratch), st), "backward_frozen": (L.ptr(dz), None, None, None, st)}

        def plain_f(fa=fa, fo=fo, keep=keep):
            L.check(L.lib.pqlk_ln_elu_forward(*fa, *fo))

        def drop_f(fa=fa, fo=fo):
            L.check(L.lib.pqlk_drop_ln_elu_forward(*fa, P, SEED, TAG, *fo))

        out[(m, w, "forward", "plain")], out[(m, w, "forward", "drop")] = plain_f, drop_f
        for what, tail in bo.items():
            def plain_b(ba=ba, tail=tail):
                L.check(L.lib.pqlk_ln_elu_backward(*ba, *tail))

            def drop_b(ba=ba, tail=tail):
                L.check(L.lib.pqlk_drop_ln_elu_backward(*ba, P, SEED, TAG, *tail))

            out[(m, w, what, "plain")], out[(m, w, what, "drop")] = plain_b, drop_b
        plain_f()   # y / mean / rstd of a forward for the backward launches (either forward serves for timing)
    return out


def time_launches(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / n * 1e3   # us per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_droq needs a GPU"
    torch.manual_seed(0)
    dev = torch.device("cuda:0")
    kv = variants(dev)
    times = {k: [] for k in kv}
    for r in range(a.rounds + 1):     # round 0 warms up
        for k, fn in kv.items():
            t = time_launches(fn, a.launches)
            if r:
                times[k].append(t)
    res = dict(device=torch.cuda.get_device_name(0), torch=torch.__version__, rounds=a.rounds, launches=a.launches, p=P, kernels=[])
    for m, w in SHAPES:
        for what in ("forward", "backward", "backward_frozen"):
            tp, td = times[(m, w, what, "plain")], times[(m, w, what, "drop")]
            rec = dict(m=m, cols=w, what=what, launches_per_call=2 if what == "backward" else 1,
                       plain_us_median=round(statistics.median(tp), 2), plain_us_min=round(min(tp), 2),
                       drop_us_median=round(statistics.median(td), 2), drop_us_min=round(min(td), 2),
                       ratio_median=round(statistics.median(td) / statistics.median(tp), 3))
            res["kernels"].append(rec)
            print(json.dumps(rec), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
