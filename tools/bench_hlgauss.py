#!/usr/bin/env python3
"""Times the two HL-Gauss loss entries against the C51 loss they stand beside: `pqlk_hlgauss_ce_loss`, `pqlk_hlgauss_ce_loss_per` and
`pqlk_c51_bce_loss` on the SAME buffers at B = 8192 and K = 51, 101, 256 (NJ = 1, 2, 4 atoms per lane).  Method of tools/bench_c51.py:
each point is one hipGraph of ITERS back-to-back calls (the loss kernel and the one-block fold of its partials) timed with HIP events;
the points are replayed in turn, ROUNDS times, in one process, so that they share whatever else the card is doing.  Inputs as a learner
meets them: logits N(0, 1), rewards over 1.2 x the support, one row in ten terminal.  Beside each median the run-to-run spread
(max - min over the rounds) is reported: it is the only margin a comparison of two points of one call gets.  Recorded, not gated.
GPU only.
    python tools/bench_hlgauss.py [--out profiles/hlgauss_bench.json] [--rows 8192] [--iters 200] [--rounds 9]"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from pql_amd import _lib as L  # noqa: E402

KS = (51, 101, 256)
KERNELS = ("pqlk_hlgauss_ce_loss", "pqlk_hlgauss_ce_loss_per", "pqlk_c51_bce_loss")
V_MIN, V_MAX, GAMMA_N, SIGMA = -10.0, 10.0, 0.99 ** 3, 0.75


def make_points(K, B, dev):
    """-> {kernel: launch()} on one set of buffers, and the bytes each must move."""
    g = torch.Generator(device=dev); g.manual_seed(1000 + K)
    f = dict(dtype=torch.float32, device=dev)
    ld = L.ld(K)
    rew = (torch.rand(B, generator=g, **f) * 2 - 1) * (0.6 * (V_MAX - V_MIN))
    done = (torch.rand(B, generator=g, **f) < 0.1).float()
    z = torch.linspace(V_MIN, V_MAX, K, device=dev)
    lg, lt = torch.zeros((2, B, ld), **f), torch.zeros((2, B, ld), **f)
    lg[:, :, :K].normal_(generator=g); lt[:, :, :K].normal_(generator=g)
    w = torch.rand(B, generator=g, **f) * 0.95 + 0.05
    wmax = w.max().reshape(1)
    dy, scr, lo, td = torch.empty((2, B, ld), **f), torch.empty(1024, **f), torch.empty(1, **f), torch.empty(B, **f)
    head = (L.ptr(lg), L.ptr(lt), ld, K, L.ptr(rew), L.ptr(done), L.ptr(z), GAMMA_N, V_MIN, V_MAX)
    out = (B, L.ptr(dy), L.ptr(lo), None, 0, None, L.ptr(scr))
    st = lambda: L.stream(dev)  # noqa: E731
    launches = {
        "pqlk_hlgauss_ce_loss": lambda: L.check(L.lib.pqlk_hlgauss_ce_loss(*head, SIGMA, *out, st())),
        "pqlk_hlgauss_ce_loss_per": lambda: L.check(L.lib.pqlk_hlgauss_ce_loss_per(*head, SIGMA, *out, L.ptr(w), L.ptr(wmax), L.ptr(td), st())),
        "pqlk_c51_bce_loss": lambda: L.check(L.lib.pqlk_c51_bce_loss(*head, *out, st())),
    }
    nbytes = B * (4 * K * 4 + 8 + 2 * ld * 4)          # four logit rows in, two dy rows (pads included) out
    return launches, {k: nbytes + (8 * B if k.endswith("_per") else 0) for k in launches}, (lg, lt, rew, done, z, w, wmax, dy, scr, lo, td)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join("profiles", "hlgauss_bench.json"))
    ap.add_argument("--rows", type=int, default=8192)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=9)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_hlgauss.py needs a GPU: it measures, it does not estimate")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    points, keep = [], []
    side = torch.cuda.Stream()
    for K in KS:
        launches, nbytes, buffers = make_points(K, a.rows, dev)
        keep.append(buffers)
        for kernel in KERNELS:
            launch = launches[kernel]
            launch()                                       # first launch outside the capture (loads the code object)
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.graph(graph, stream=side):
                for _ in range(a.iters):
                    launch()
            points.append(dict(kernel=kernel, K=K, ld=L.ld(K), bytes=nbytes[kernel], graph=graph, us=[]))
    for p in points:                                       # warm-up replay of every graph
        p["graph"].replay()
    torch.cuda.synchronize()
    for _ in range(a.rounds):
        for p in points:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); p["graph"].replay(); e1.record(); e1.synchronize()
            p["us"].append(e0.elapsed_time(e1) / a.iters * 1e3)
    res = []
    for p in points:
        med, spread = statistics.median(p["us"]), max(p["us"]) - min(p["us"])
        res.append(dict(kernel=p["kernel"], K=p["K"], ld=p["ld"], rows=a.rows, bytes_moved=p["bytes"], us_median=round(med, 3),
                        us_min=round(min(p["us"]), 3), us_max=round(max(p["us"]), 3), us_spread=round(spread, 3),
                        us_rounds=[round(t, 3) for t in p["us"]], tb_per_s=round(p["bytes"] / med / 1e6, 3)))
        print(f"{p['kernel']:26s} K={p['K']:3d}: {med:8.2f} us per call (min {min(p['us']):.2f}, max {max(p['us']):.2f}, spread {spread:.2f}), "
              f"{p['bytes'] / 1e6:.2f} MB -> {p['bytes'] / med / 1e6:.3f} TB/s", flush=True)
    versus = []
    for K in KS:
        at = {r["kernel"]: r for r in res if r["K"] == K}
        hl, per, c51 = (at[k] for k in KERNELS)
        margin = max(hl["us_spread"], c51["us_spread"])
        versus.append(dict(K=K, hlgauss_us=hl["us_median"], hlgauss_per_us=per["us_median"], c51_us=c51["us_median"],
                           hlgauss_over_c51=round(hl["us_median"] / c51["us_median"], 4), margin_us=margin,
                           hlgauss_no_slower=bool(hl["us_median"] <= c51["us_median"] + margin)))
        print(f"K={K:3d}: hl_gauss / c51 = {versus[-1]['hlgauss_over_c51']:.3f} (margin {margin:.2f} us): "
              f"{'no slower' if versus[-1]['hlgauss_no_slower'] else 'SLOWER'}", flush=True)
    doc = dict(tool="tools/bench_hlgauss.py", device=torch.cuda.get_device_name(dev), rows=a.rows, launches_per_graph=a.iters, rounds=a.rounds,
               sigma_ratio=SIGMA, method="hipGraph replay of back-to-back calls, HIP events, points alternated; the three entries of one K share "
               "their buffers; terminal rows 10 %; us_spread = max - min over the rounds", results=res, versus_c51=versus)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")
    print(json.dumps(dict(out=a.out, points=len(res))))


if __name__ == "__main__":
    main()
