#!/usr/bin/env python3
"""SHA-256 of every output buffer of the loss (pql_amd/csrc/loss.hip) and tree-walk (pql_amd/csrc/per.hip) entry points on fixed
inputs, as JSON: the tool for "this refactor moved no bit".  Run it on two builds -- `PQLK_LIB=/path/to/other/libpqlk.so` selects the
library, as everywhere -- each in a fresh process, and compare the two files; the tool itself compares nothing.  GPU only.

    python tools/loss_bits.py [--out profiles/loss_bits.json] [--label parent] [--compact]

--compact (a record to commit): one SHA-256 per group of cases -- entry and first parameter, e.g. "tqc_huber_loss_soft N=33" -- over
the sorted "case/buffer=hash" lines of the group, with its counts; the full output says which case and buffer of a differing group moved.

Inputs: tests/reduction_cases.py, tests/c51_wide_cases.py, tests/detdata.py, tests/quantile_cases.py, tests/tqc_cases.py,
tests/tqc_sac_cases.py.  Every output buffer starts as poison, with SLACK floats
of poison behind it, and is hashed whole: pad columns, untouched slack and all.  Cases: the smallest shapes at which these kernels
can go wrong --
  c51_bce, dpg_dist  every (K, ld) of rc.C51_SHAPES and wc.SHAPES (K = 2, a full wave, one atom past it, ragged groups, pad columns
                     past the last group) at B = 37 and B = 5 (a second block with one row, idle waves), saturated rows, proj_out NULL
  c51_project        K in 2, 51, 64, 65, 101, 256 at B = 263: terminal rows, rewards on an atom, rewards past both ends
  td_mse[_per]       B in 1, 255, 257 at ld 32; with a loss slot and without; unit and non-trivial weights
  dpg_scalar         B in 1, 257
  qr_huber[_per], tqc_huber[_soft][_per], dpg_quantile[_mean]
                     N in 2, 8, 33 (ld 64: pad columns), 64 (no idle lane) x B in 1, 5, 37, 4099 (past the 1024-block cap: a second,
                     ragged trip of the row loop); drop in 0, 2, N - 1; no, unit and mixed weights; logp = 0 and normal (log_alpha
                     -1.6); with a loss slot and without; and the dyadic rows of tqc_cases (exact ties in the pool) at B = 16, N = 8
  per                rings of 65, 4097 and 70 000 rows (two, two and three levels), B = 256, alpha in 1.0, 0.6, beta 0.4:
                     pqlk_per_sample + pqlk_per_weights, and pqlk_per_sample_steps over 3 steps"""
import argparse
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import c51_wide_cases as wc  # noqa: E402
import detdata as dd  # noqa: E402
import quantile_cases as qc  # noqa: E402
import reduction_cases as rc  # noqa: E402
import tqc_cases as tc  # noqa: E402
import tqc_sac_cases as sc  # noqa: E402
from pql_amd import _lib as L  # noqa: E402

POISON, SLACK = rc.POISON, rc.SLACK
V_MIN, V_MAX = -10.0, 10.0
PROJECT_KS = (2, 51, 64, 65, 101, 256)
PER_CAPS, PER_B, PER_STEPS, PER_BETA = (65, 4097, 70_000), 256, 3, 0.4
QR_NS, QR_BS, QR_GAMMA_N, QR_KAPPA, QR_LOG_ALPHA = (2, 8, 33, 64), (1, 5, 37, 4099), float(np.float32(0.99 ** 3)), 0.75, -1.6
# (weights, logp, with a loss slot) of the Huber entries; those with a logp run on the pooled (drop) entries only
QR_VARIANTS = ((None, None, 1), (None, None, 0), ("unit", None, 1), ("mixed", None, 1), (None, "zero", 1), (None, "normal", 1), ("unit", "zero", 1),
               ("mixed", "normal", 1), ("mixed", "normal", 0))


def sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


class Out:
    """A poisoned device buffer of `n` elements with SLACK more behind it; hashed whole."""

    def __init__(self, dev, n, dtype=torch.float32):
        self.full = torch.full((int(n) + SLACK,), POISON, dtype=dtype, device=dev)

    @property
    def ptr(self):
        return L.ptr(self.full)


def dev_in(dev, x):
    x = x if torch.is_tensor(x) else rc.T(np.asarray(x))
    return x.contiguous().to(dev)


def padded(dev, x, ld):
    """(2, B, K) -> (2, B, ld) with IN_BIG in the pad columns."""
    out = torch.full((2, x.shape[1], ld), rc.IN_BIG, dtype=torch.float32, device=dev)
    out[:, :, : x.shape[2]] = dev_in(dev, x)
    return out


def c51_cases(dev, res):
    st = L.stream(dev)
    for K, ld in rc.C51_SHAPES + wc.SHAPES:
        z = torch.linspace(V_MIN, V_MAX, K).to(dev)
        for B, sat, with_proj in ((wc.B_SMALL, False, True), (5, False, True), (wc.B_SMALL, True, True), (wc.B_SMALL, False, False)):
            lg, lt, rew, done, gn = (rc.c51_inputs if K <= 64 else wc.bce_inputs)(B, K, saturated=sat)
            lgd, ltd, rd, dn = padded(dev, lg, ld), padded(dev, lt, ld), dev_in(dev, rew.view(-1)), dev_in(dev, done.view(-1))
            parts = int(L.lib.pqlk_loss_parts(B, K))
            dy, lo, scr, pj = Out(dev, 2 * B * ld), Out(dev, 1), Out(dev, parts), Out(dev, B * K)
            L.check(L.lib.pqlk_c51_bce_loss(L.ptr(lgd), L.ptr(ltd), ld, K, L.ptr(rd), L.ptr(dn), L.ptr(z), gn, V_MIN, V_MAX, B, dy.ptr,
                                            lo.ptr, None, 0, pj.ptr if with_proj else None, scr.ptr, st))
            res[f"c51_bce K={K} ld={ld} B={B} sat={int(sat)} proj={int(with_proj)}"] = dict(
                dy=sha(dy.full), loss=sha(lo.full), partials=sha(scr.full), proj_out=sha(pj.full))
        for B in (wc.B_SMALL, 5):
            qd = padded(dev, rc.dpg_dist_inputs(B, K), ld)
            dy, lo, scr = Out(dev, 2 * B * ld), Out(dev, 1), Out(dev, int(L.lib.pqlk_loss_parts(B, K)))
            L.check(L.lib.pqlk_dpg_loss(L.ptr(qd), ld, K, L.ptr(z), B, dy.ptr, lo.ptr, None, 0, scr.ptr, st))
            res[f"dpg_dist K={K} ld={ld} B={B}"] = dict(dy=sha(dy.full), loss=sha(lo.full), partials=sha(scr.full))
    for K in PROJECT_KS:
        B = wc.PROJECT_B
        p, rew, done, gn, _ = wc.project_inputs(B, K)
        pd, rd, dn, z = dev_in(dev, p), dev_in(dev, rew.view(-1)), dev_in(dev, done.view(-1)), torch.linspace(V_MIN, V_MAX, K).to(dev)
        out = Out(dev, B * K)
        L.check(L.lib.pqlk_c51_project(L.ptr(pd), L.ptr(rd), L.ptr(dn), L.ptr(z), gn, V_MIN, V_MAX, K, B, out.ptr, st))
        res[f"c51_project K={K} B={B}"] = dict(proj_out=sha(out.full))


def scalar_cases(dev, res):
    st, ld = L.stream(dev), 32
    for B in (1, 255, 257):
        q, qt = dd.uniform((2, B, 1), 811, -3, 3), dd.uniform((2, B, 1), 812, -3, 3)
        qd, qtd = padded(dev, q, ld), padded(dev, qt, ld)
        rd, dn = dev_in(dev, dd.uniform((B,), 813, -1, 1)), dev_in(dev, dd.bernoulli((B,), 814, 0.2))
        gn = float(np.float32(0.99 ** 3))
        parts = int(L.lib.pqlk_loss_parts(B, 1))
        weights = dict(unit=np.ones(B, dtype=np.float32), mixed=dd.uniform((B,), 815, 0.05, 1.0))
        for with_loss in (True, False):
            for wname, w in [(None, None)] + list(weights.items()):
                dy, lo, scr, td = Out(dev, 2 * B * ld), Out(dev, 1), Out(dev, parts), Out(dev, B)
                head = (L.ptr(qd), L.ptr(qtd), ld, L.ptr(rd), L.ptr(dn), gn, B, dy.ptr, lo.ptr if with_loss else None, None, 0, scr.ptr)
                if w is None:
                    L.check(L.lib.pqlk_td_mse_loss(*head, st))
                else:
                    wd, wm = dev_in(dev, w), dev_in(dev, np.array([w.max()], dtype=np.float32))
                    L.check(L.lib.pqlk_td_mse_loss_per(*head, L.ptr(wd), L.ptr(wm), td.ptr, st))
                res[f"td_mse{'' if w is None else '_per w=' + wname} B={B} loss={int(with_loss)}"] = dict(
                    dy=sha(dy.full), loss=sha(lo.full), partials=sha(scr.full), abs_td=sha(td.full))
    for B in (1, 257):
        qd = padded(dev, rc.dpg_scalar_inputs(B)[:, :, None], ld)
        dy, lo, scr = Out(dev, 2 * B * ld), Out(dev, 1), Out(dev, int(L.lib.pqlk_loss_parts(B, 1)))
        L.check(L.lib.pqlk_dpg_loss(L.ptr(qd), ld, 1, None, B, dy.ptr, lo.ptr, None, 0, scr.ptr, st))
        res[f"dpg_scalar B={B}"] = dict(dy=sha(dy.full), loss=sha(lo.full), partials=sha(scr.full))


def quantile_shape(dev, res, tag, case, N, logps, gamma_n, kappa, log_alpha):
    """All eight quantile entries on one set of heads `case` (theta, theta_t (2, B, N), rew, done, w)."""
    st, ld, B = L.stream(dev), L.ld(N), case["rew"].shape[0]
    th, tt, rd, dn = padded(dev, case["theta"], ld), padded(dev, case["theta_t"], ld), dev_in(dev, case["rew"]), dev_in(dev, case["done"])
    weights = dict(unit=np.ones(B, dtype=np.float32), mixed=case["w"])
    la, parts = dev_in(dev, np.array([log_alpha], dtype=np.float32)), int(L.lib.pqlk_loss_parts(B, N))
    for drop in [None] + sorted({d for d in (0, 2, N - 1) if d < N}):
        for wname, lname, with_loss in QR_VARIANTS:
            if lname is not None and drop is None:
                continue
            dy, lo, scr, td = Out(dev, 2 * B * ld), Out(dev, 1), Out(dev, parts), Out(dev, B)
            args = [L.ptr(th), L.ptr(tt), ld, N, L.ptr(rd), L.ptr(dn), gamma_n, kappa, B, dy.ptr, lo.ptr if with_loss else None, None, 0, scr.ptr]
            if wname is not None:
                wd, wm = dev_in(dev, weights[wname]), dev_in(dev, np.array([weights[wname].max()], dtype=np.float32))
                args += [L.ptr(wd), L.ptr(wm), td.ptr]
            if lname is not None:
                lp = dev_in(dev, logps[lname])
                args += [L.ptr(lp), L.ptr(la)]
            name = ("qr_huber_loss" if drop is None else "tqc_huber_loss") + ("" if lname is None else "_soft") + ("" if wname is None else "_per")
            L.check(getattr(L.lib, "pqlk_" + name)(*args, *([] if drop is None else [drop]), st))
            res[f"{name} {tag} drop={drop} w={wname} logp={lname} loss={with_loss}"] = dict(
                dy=sha(dy.full), loss=sha(lo.full), partials=sha(scr.full), abs_td=sha(td.full))
    for entry in ("dpg_loss_quantile", "dpg_loss_quantile_mean"):
        for with_loss in (1, 0):
            dy, lo, scr = Out(dev, 2 * B * ld), Out(dev, 1), Out(dev, parts)
            L.check(getattr(L.lib, "pqlk_" + entry)(L.ptr(th), ld, N, B, dy.ptr, lo.ptr if with_loss else None, None, 0, scr.ptr, st))
            res[f"{entry} {tag} loss={with_loss}"] = dict(dy=sha(dy.full), loss=sha(lo.full), partials=sha(scr.full))


def quantile_cases(dev, res):
    for N in QR_NS:
        for B in QR_BS:
            seed = 5000 + 100 * N + B % 97
            logps = dict(zero=np.zeros(B, dtype=np.float32), normal=sc.logp_normal(B, seed + 1))
            quantile_shape(dev, res, f"N={N} B={B}", qc.normal_case(B, N, seed, per=True), N, logps, QR_GAMMA_N, QR_KAPPA, QR_LOG_ALPHA)
    B, N = 16, 8   # exact ties between pooled atoms and between the nets' means; log_alpha 0: the shift is logp itself
    case = dict(tc.dyadic_case(B, N, 77), w=np.linspace(0.25, 1.0, B, dtype=np.float32))
    logps = dict(zero=np.zeros(B, dtype=np.float32), normal=sc.logp_dyadic(B, 78))
    quantile_shape(dev, res, f"dyadic N={N} B={B}", case, N, logps, qc.DYADIC_GAMMA, qc.DYADIC_KAPPA, 0.0)


def per_cases(dev, res):
    st, B = L.stream(dev), PER_B
    u = dev_in(dev, dd.uniform((B,), 911, 0.0, 1.0))
    r = dev_in(dev, dd.integers((PER_STEPS * B,), 912, 1 << 24))
    for cap in PER_CAPS:
        for alpha in (1.0, 0.6):
            tree = torch.zeros(int(L.lib.pqlk_per_tree_floats(cap)), device=dev)
            pmax = torch.ones(1, device=dev)
            rows = torch.arange(cap, dtype=torch.int64, device=dev)
            prio = dev_in(dev, np.random.default_rng(1234 + cap).gamma(0.7, 1.0, cap).astype(np.float32))
            L.check(L.lib.pqlk_per_update(L.ptr(tree), cap, L.ptr(pmax), L.ptr(rows), L.ptr(prio), cap, 1e-6, alpha, st))
            idx, w, wmax = Out(dev, B, torch.int64), Out(dev, B), Out(dev, 1)
            L.check(L.lib.pqlk_per_sample(L.ptr(tree), cap, L.ptr(u), B, idx.ptr, st))
            L.check(L.lib.pqlk_per_weights(L.ptr(tree), cap, idx.ptr, B, cap, PER_BETA, w.ptr, wmax.ptr, st))
            res[f"per_sample+weights cap={cap} alpha={alpha}"] = dict(idx=sha(idx.full), w=sha(w.full), wmax=sha(wmax.full), tree=sha(tree))
            idx, w, wmax = Out(dev, PER_STEPS * B, torch.int64), Out(dev, PER_STEPS * B), Out(dev, PER_STEPS)
            L.check(L.lib.pqlk_per_sample_steps(L.ptr(tree), cap, L.ptr(r), B, PER_STEPS, cap, PER_BETA, idx.ptr, w.ptr, wmax.ptr, st))
            res[f"per_sample_steps cap={cap} alpha={alpha}"] = dict(idx=sha(idx.full), w=sha(w.full), wmax=sha(wmax.full))


def compact(res):
    """{group: {cases, buffers, sha256 over the group's sorted "case/buffer=hash" lines}}, group = the first two words of the case."""
    groups = {}
    for case, bufs in res.items():
        groups.setdefault(" ".join(case.split()[:2]), []).append((case, bufs))
    return {g: dict(cases=len(v), buffers=sum(len(b) for _, b in v),
                    sha256=hashlib.sha256("\n".join(sorted(f"{c}/{k}={h}" for c, b in v for k, h in b.items())).encode()).hexdigest())
            for g, v in groups.items()}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join("profiles", "loss_bits.json"))
    ap.add_argument("--label", default="", help="recorded in the output: which build this run hashed")
    ap.add_argument("--compact", action="store_true", help="one hash per group of cases instead of one per buffer")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("loss_bits.py needs a GPU: it hashes what the kernels write")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    res = {}
    c51_cases(dev, res)
    scalar_cases(dev, res)
    quantile_cases(dev, res)
    per_cases(dev, res)
    torch.cuda.synchronize()
    doc = dict(tool="tools/loss_bits.py", device=torch.cuda.get_device_name(dev), label=a.label, **(dict(groups=compact(res)) if a.compact else dict(hashes=res)))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        if a.compact:   # one group per line
            head = json.dumps({k: v for k, v in doc.items() if k != "groups"})
            fh.write(head[:-1] + ', "groups": {\n' + ",\n".join(f" {json.dumps(g)}: {json.dumps(v)}" for g, v in doc["groups"].items()) + "\n}}")
        else:
            json.dump(doc, fh, indent=1)
        fh.write("\n")
    print(json.dumps(dict(out=a.out, cases=len(res), buffers=sum(len(v) for v in res.values()))))


if __name__ == "__main__":
    main()
