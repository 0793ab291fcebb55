#!/usr/bin/env python3
"""Times the C51 loss kernels across the 64-atom seam: `pqlk_c51_bce_loss`, `pqlk_c51_project` and the distributional
`pqlk_dpg_loss` at K = 51 (the NJ = 1 instances: one atom per lane, cross-lane projection), 101 and 256 (several atoms per lane,
projection through the wave's LDS image), B = 8192.  Each point is
one hipGraph of ITERS back-to-back launches timed with HIP events; the points are replayed in turn, ROUNDS times, in one
process, so that they share whatever else the card is doing.  Inputs as a learner meets them: logits N(0, 1), rewards over
1.2 x the support, one row in ten terminal (a terminal row is the projection's longest walk: one bin collects every atom).
Recorded, not gated.  GPU only.
    python tools/bench_c51.py [--out profiles/c51_wide.json] [--rows 8192] [--iters 200] [--rounds 7]"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from pql_amd import _lib as L  # noqa: E402

KS = (51, 101, 256)
ENTRY = dict(bce="pqlk_c51_bce_loss", project="pqlk_c51_project", dpg="pqlk_dpg_loss")
V_MIN, V_MAX, GAMMA_N = -10.0, 10.0, 0.99 ** 3


def make_point(kind, K, B, dev):
    """-> (launch(), bytes the kernel must move)"""
    g = torch.Generator(device=dev); g.manual_seed(1000 + K)
    f = dict(dtype=torch.float32, device=dev)
    ld = L.ld(K)
    rew = (torch.rand(B, generator=g, **f) * 2 - 1) * (0.6 * (V_MAX - V_MIN))
    done = (torch.rand(B, generator=g, **f) < 0.1).float()
    z = torch.linspace(V_MIN, V_MAX, K, device=dev)
    st = lambda: L.stream(dev)  # noqa: E731
    if kind == "bce":
        lg, lt = torch.zeros((2, B, ld), **f), torch.zeros((2, B, ld), **f)
        lg[:, :, :K].normal_(generator=g); lt[:, :, :K].normal_(generator=g)
        dy, scr, lo = torch.empty((2, B, ld), **f), torch.empty(1024, **f), torch.empty(1, **f)

        def launch():
            L.check(L.lib.pqlk_c51_bce_loss(L.ptr(lg), L.ptr(lt), ld, K, L.ptr(rew), L.ptr(done), L.ptr(z), GAMMA_N, V_MIN, V_MAX, B,
                                            L.ptr(dy), L.ptr(lo), None, 0, None, L.ptr(scr), st()))
        nbytes = B * (4 * K * 4 + 8 + 2 * ld * 4)          # four logit rows in, two dy rows (pads included) out
    elif kind == "dpg":
        lg = torch.zeros((2, B, ld), **f)
        lg[:, :, :K].normal_(generator=g)
        dy, scr, lo = torch.empty((2, B, ld), **f), torch.empty(1024, **f), torch.empty(1, **f)

        def launch():
            L.check(L.lib.pqlk_dpg_loss(L.ptr(lg), ld, K, L.ptr(z), B, L.ptr(dy), L.ptr(lo), None, 0, L.ptr(scr), st()))
        nbytes = B * (2 * K * 4 + 2 * ld * 4)              # two logit rows in, two dy rows (pads included) out
    else:
        p = torch.softmax(torch.randn((B, K), generator=g, **f), 1).contiguous()
        out = torch.empty((B, K), **f)

        def launch():
            L.check(L.lib.pqlk_c51_project(L.ptr(p), L.ptr(rew), L.ptr(done), L.ptr(z), GAMMA_N, V_MIN, V_MAX, K, B, L.ptr(out), st()))
        nbytes = B * (2 * K * 4 + 8)
    return launch, nbytes


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join("profiles", "c51_wide.json"))
    ap.add_argument("--rows", type=int, default=8192)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=7)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_c51.py needs a GPU: it measures, it does not estimate")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    points = []
    side = torch.cuda.Stream()
    for kind in ("bce", "project", "dpg"):
        for K in KS:
            launch, nbytes = make_point(kind, K, a.rows, dev)
            launch()                                       # first launch outside the capture (loads the code object)
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.graph(graph, stream=side):
                for _ in range(a.iters):
                    launch()
            # the loss entry points are two launches (the loss kernel and the one-block fold of its partials): both are in the figure
            points.append(dict(kernel=ENTRY[kind], K=K, ld=K if kind == "project" else L.ld(K),
                               bytes=nbytes, graph=graph, launch=launch, us=[]))
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
        med = statistics.median(p["us"])
        res.append(dict(kernel=p["kernel"], K=p["K"], ld=p["ld"], rows=a.rows, bytes_moved=p["bytes"], us_median=round(med, 3),
                        us_min=round(min(p["us"]), 3), us_max=round(max(p["us"]), 3), us_rounds=[round(t, 3) for t in p["us"]],
                        tb_per_s=round(p["bytes"] / med / 1e6, 3)))
        print(f"{p['kernel']:18s} K={p['K']:3d}: {med:8.2f} us per call (min {min(p['us']):.2f}, max {max(p['us']):.2f}), "
              f"{p['bytes'] / 1e6:.2f} MB -> {p['bytes'] / med / 1e6:.3f} TB/s", flush=True)
    doc = dict(tool="tools/bench_c51.py", device=torch.cuda.get_device_name(dev), rows=a.rows, launches_per_graph=a.iters, rounds=a.rounds,
               method="hipGraph replay of back-to-back calls, HIP events, points alternated; terminal rows 10 %", results=res)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")
    print(json.dumps(dict(out=a.out, points=len(res))))


if __name__ == "__main__":
    main()
