#!/usr/bin/env python3
"""Times the two diagnostics entries: `pqlk_critic_stats` at B = 8192 on each head kind (scalar; categorical K = 51 and 256; quantile
N = 32) and `pqlk_unit_stats` on 8192 x {128, 256, 512} post-ELU matrices.  Method of tools/bench_hlgauss.py: each point is one
hipGraph of ITERS back-to-back calls (a call is two launches: the reduction and the one-block fold) timed with HIP events; the points
are replayed in turn, ROUNDS times, in one process, so that they share whatever else the card is doing.  Beside each median the
run-to-run spread (max - min over the rounds) is reported.  Recorded, not gated.  GPU only.
    python tools/bench_diag.py [--out profiles/diag_bench.json] [--rows 8192] [--iters 200] [--rounds 9]"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from pql_amd import _lib as L  # noqa: E402

HEADS = (("scalar", L.HEAD_SCALAR, 1), ("categorical", L.HEAD_CATEGORICAL, 51), ("categorical", L.HEAD_CATEGORICAL, 256),
         ("quantile", L.HEAD_QUANTILE, 32))
WIDTHS = (128, 256, 512)
V_MIN, V_MAX, GAMMA_N, TAU = -10.0, 10.0, 0.99 ** 3, 0.025


def critic_point(head, k, B, dev):
    """-> (launch(), bytes the call must read, the buffers it keeps alive)."""
    g = torch.Generator(device=dev); g.manual_seed(1000 + k)
    f = dict(dtype=torch.float32, device=dev)
    ld = L.ld(k)
    q, qt = torch.zeros((2, B, ld), **f), torch.zeros((2, B, ld), **f)
    q[:, :, :k].normal_(generator=g); qt[:, :, :k].normal_(generator=g)
    rew, done = torch.rand(B, generator=g, **f) * 2 - 1, (torch.rand(B, generator=g, **f) < 0.1).float()
    z = torch.linspace(V_MIN, V_MAX, max(k, 2), device=dev)
    out, scr = torch.empty(L.CRITIC_STATS, **f), torch.empty(int(L.lib.pqlk_critic_stats_scratch_floats(B, k)), **f)
    args = (L.ptr(q), L.ptr(qt), ld, head, k, L.ptr(z), V_MIN, V_MAX, L.ptr(rew), L.ptr(done), GAMMA_N, B, L.ptr(out), L.ptr(scr))
    return (lambda: L.check(L.lib.pqlk_critic_stats(*args, L.stream(dev)))), B * (4 * k * 4 + 8), (q, qt, rew, done, z, out, scr)


def unit_point(cols, rows, dev):
    g = torch.Generator(device=dev); g.manual_seed(2000 + cols)
    h = torch.nn.functional.elu(torch.randn((rows, cols), generator=g, dtype=torch.float32, device=dev)).contiguous()
    out = torch.empty(3, dtype=torch.float32, device=dev)
    scr = torch.empty(int(L.lib.pqlk_unit_stats_scratch_floats(cols)), dtype=torch.float32, device=dev)
    args = (L.ptr(h), cols, rows, cols, TAU, L.ptr(out), L.ptr(scr))
    return (lambda: L.check(L.lib.pqlk_unit_stats(*args, L.stream(dev)))), rows * cols * 4, (h, out, scr)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join("profiles", "diag_bench.json"))
    ap.add_argument("--rows", type=int, default=8192)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=9)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_diag.py needs a GPU: it measures, it does not estimate")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    made = [(dict(kernel="pqlk_critic_stats", head=name, k=k, ld=L.ld(k)), critic_point(head, k, a.rows, dev)) for name, head, k in HEADS]
    made += [(dict(kernel="pqlk_unit_stats", cols=c, ld=c), unit_point(c, a.rows, dev)) for c in WIDTHS]
    points, side = [], torch.cuda.Stream()
    for what, (launch, nbytes, buffers) in made:
        launch()                                       # first launch outside the capture (loads the code object)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.graph(graph, stream=side):
            for _ in range(a.iters):
                launch()
        points.append(dict(what, rows=a.rows, bytes_read=nbytes, graph=graph, keep=buffers, us=[]))
    for p in points:                                   # warm-up replay of every graph
        p["graph"].replay()
    torch.cuda.synchronize()
    for _ in range(a.rounds):
        for p in points:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); p["graph"].replay(); e1.record(); e1.synchronize()
            p["us"].append(e0.elapsed_time(e1) / a.iters * 1e3)
    res = []
    for p in points:
        us = p.pop("us")
        p.pop("graph"); p.pop("keep")
        med = statistics.median(us)
        res.append(dict(p, us_median=round(med, 3), us_min=round(min(us), 3), us_max=round(max(us), 3), us_spread=round(max(us) - min(us), 3),
                        us_rounds=[round(t, 3) for t in us], tb_per_s=round(p["bytes_read"] / med / 1e6, 3)))
        tag = f"{p['head']} k={p['k']}" if "head" in p else f"cols={p['cols']}"
        print(f"{p['kernel']:18s} {tag:20s}: {med:8.2f} us per call (min {min(us):.2f}, max {max(us):.2f}), {p['bytes_read'] / 1e6:.2f} MB read "
              f"-> {p['bytes_read'] / med / 1e6:.3f} TB/s", flush=True)
    doc = dict(tool="tools/bench_diag.py", device=torch.cuda.get_device_name(dev), rows=a.rows, launches_per_graph=a.iters, rounds=a.rounds,
               tau=TAU, method="hipGraph replay of back-to-back calls (each call: the reduction launch and its one-block fold), HIP events, "
               "points alternated; terminal rows 10 %; us_spread = max - min over the rounds", results=res)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")
    print(json.dumps(dict(out=a.out, points=len(res))))


if __name__ == "__main__":
    main()
