#!/usr/bin/env python3
"""SHA-256 of every output buffer of the whole-stack launches of the LayerNorm critic family (pql_amd/csrc/fwd_ln.hip, fwd_ln_bf16.hip,
fwd_bro.hip, fwd_bro_bf16.hip, bwd_ln.hip, sharing lnstack.h) and of the bf16 MLP forward (fwd_bf16.hip, sharing bf16.h) on fixed
inputs, as JSON: the tool for "this refactor moved no bit", on the pattern of tools/loss_bits.py.  Run it on two builds --
`PQLK_LIB=/path/to/other/libpqlk.so` selects the library, as everywhere -- each in a fresh process, and compare the two files; the tool
itself compares nothing.  GPU only.

    python tools/stack_bits.py [--out profiles/stack_bits.json] [--label parent] [--compact]

--compact (a record to commit): one SHA-256 per group of cases -- entry and first parameter, e.g. "bro_forward W=512" -- over the
sorted "case/buffer=hash" lines of the group, with its counts; the full output says which case and buffer of a differing group moved.

Arenas, inputs and upstream gradients are uniform draws of a seeded numpy generator; every output buffer starts as poison, with SLACK
elements of poison behind it, and is hashed whole: pad columns, rows past m, untouched slack and all.  The cases are the lists the GPU
tests of these entries keep, the smallest shapes at which the kernels can go wrong (widths 32 .. 1024, input widths 3, 10, 40, 104,
m in 1 .. 130, K in 0 .. 16):
  lnmlp_forward            CASES of tests/test_lnmlp_kernels_gpu.py, stash on and off; the first case once more with one net
  lnmlp_drop_forward       CASES of tests/test_droq_fused_kernels_gpu.py (p in 0.01, 0.5), stash on
  lnmlp_forward_bf16       CASES of tests/test_lnmlp_bf16_gpu.py: pqlk_lnmlp_pack_bf16, then the forward on the packed copy
  lnmlp_drop_forward_bf16  CASES of tests/test_droq_fused_kernels_gpu.py, on the packed copy
  bro_forward              CASES of tests/test_bro_fused_kernels_gpu.py, stash on and off
  bro_forward_bf16         CASES of tests/test_bro_bf16_gpu.py: pqlk_bro_pack_bf16, then the forward
  lnmlp_dx                 FORMS of tests/lnmlp_dx_cases.py (plain and through the tanh window) at r = 0, 1, 2; a refused r is recorded
  lnmlp_grad_chain         GRAD_CASES of tests/lnmlp_grad_cases.py at r = 0, 1, 2
  mlp_forward_bf16         the smallest stack of tests/test_bf16_forward_gpu.py, [24, 128, 128, 1] x 2 nets, B in 1, 65:
                           pqlk_mlp_pack_bf16, then pqlk_mlp_forward_bf16"""
import argparse
import ctypes as C
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import lnmlp_dx_cases as dxc  # noqa: E402
import lnmlp_grad_cases as gc  # noqa: E402
import reduction_cases as rc  # noqa: E402
import test_bro_bf16_gpu as t_bro_bf16  # noqa: E402
import test_bro_fused_kernels_gpu as t_bro  # noqa: E402
import test_droq_fused_kernels_gpu as t_droq  # noqa: E402
import test_lnmlp_bf16_gpu as t_ln_bf16  # noqa: E402
import test_lnmlp_kernels_gpu as t_ln  # noqa: E402
from pql_amd import _lib as L  # noqa: E402
from pql_amd.models.layernorm import lnmlp_desc  # noqa: E402

POISON, SLACK = rc.POISON, rc.SLACK
EPS = 1e-5
DROP_SEED, DROP_TAG_BASE = 0x9E3779B97F4A7C15, (0xA5 << 40) | (70001 << 8) | (1 << 5)   # both key words, the tag's high word in play
BF16_MLP_DIMS, BF16_MLP_BS = [24, 128, 128, 1], (1, 65)


def sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


class Out:
    """A poisoned device buffer of `n` elements with SLACK more behind it; hashed whole."""

    def __init__(self, dev, n, dtype=torch.float32):
        self.full = torch.full((int(n) + SLACK,), POISON, dtype=dtype, device=dev)

    @property
    def ptr(self):
        return L.ptr(self.full)


def draw(dev, seed, n, lo=-0.3, hi=0.3):
    return torch.from_numpy(np.random.default_rng(seed).uniform(lo, hi, int(n)).astype(np.float32)).to(dev)


def x_of(dev, seed, m, k):
    """(m, ld(k)) input, a big value in the pad columns: they must not reach any output."""
    x = torch.full((m, L.ld(k)), rc.IN_BIG, dtype=torch.float32, device=dev)
    x[:, :k] = draw(dev, seed, m * k, -1.0, 1.0).view(m, k)
    return x


def ln_stack(dev, hidden, k, n_nets=2):
    d = lnmlp_desc([k, *hidden, 1], n_nets)
    return d, draw(dev, 100 + 7 * k + len(hidden), L.lib.pqlk_lnmlp_param_floats(C.byref(d)))


def ln_packed(dev, d, arena):
    pk = Out(dev, L.lib.pqlk_lnmlp_packed_bf16_elems(C.byref(d)), torch.int16)
    L.check(L.lib.pqlk_lnmlp_pack_bf16(C.byref(d), L.ptr(arena), pk.ptr, L.stream(dev)))
    return pk


def ln_cases(dev, res):
    st = L.stream(dev)
    for (hidden, k, m), n_nets in [(c, 2) for c in t_ln.CASES] + [(t_ln.CASES[0], 1)]:
        d, arena = ln_stack(dev, hidden, k, n_nets)
        x = x_of(dev, 200 + m, m, k)
        for stash in (1, 0):
            q, slab = Out(dev, n_nets * m * 32), Out(dev, L.lib.pqlk_lnmlp_stash_floats(C.byref(d), m))
            L.check(L.lib.pqlk_lnmlp_forward(C.byref(d), L.ptr(arena), L.ptr(x), x.stride(0), m, EPS, slab.ptr if stash else None, q.ptr, st))
            res[f"lnmlp_forward hidden={hidden} k={k} m={m} nets={n_nets} stash={stash}"] = dict(q=sha(q.full), stash=sha(slab.full))
    for hidden, k, m in t_ln_bf16.CASES:
        d, arena = ln_stack(dev, hidden, k)
        x, pk, q = x_of(dev, 200 + m, m, k), ln_packed(dev, d, arena), Out(dev, 2 * m * 32)
        L.check(L.lib.pqlk_lnmlp_forward_bf16(C.byref(d), L.ptr(arena), pk.ptr, L.ptr(x), x.stride(0), m, EPS, q.ptr, st))
        res[f"lnmlp_forward_bf16 hidden={hidden} k={k} m={m}"] = dict(packed=sha(pk.full), q=sha(q.full))
    for hidden, k, m, p in t_droq.CASES:
        d, arena = ln_stack(dev, hidden, k)
        x, pk = x_of(dev, 200 + m, m, k), ln_packed(dev, d, arena)
        q, slab, qb = Out(dev, 2 * m * 32), Out(dev, L.lib.pqlk_lnmlp_stash_floats(C.byref(d), m)), Out(dev, 2 * m * 32)
        L.check(L.lib.pqlk_lnmlp_drop_forward(C.byref(d), L.ptr(arena), L.ptr(x), x.stride(0), m, EPS, p, DROP_SEED, DROP_TAG_BASE, slab.ptr,
                                              q.ptr, st))
        L.check(L.lib.pqlk_lnmlp_drop_forward_bf16(C.byref(d), L.ptr(arena), pk.ptr, L.ptr(x), x.stride(0), m, EPS, p, DROP_SEED,
                                                   DROP_TAG_BASE, qb.ptr, st))
        res[f"lnmlp_drop_forward hidden={hidden} k={k} m={m} p={p}"] = dict(q=sha(q.full), stash=sha(slab.full))
        res[f"lnmlp_drop_forward_bf16 hidden={hidden} k={k} m={m} p={p}"] = dict(q=sha(qb.full))


def bro_cases(dev, res):
    st = L.stream(dev)
    for W, K, k, m in t_bro.CASES:
        arena, x = draw(dev, 300 + W + K, L.lib.pqlk_bro_param_floats(k, W, K, 2)), x_of(dev, 200 + m, m, k)
        for stash in (1, 0):
            q, slab = Out(dev, 2 * m * 32), Out(dev, L.lib.pqlk_bro_stash_floats(W, K, 2, m))
            L.check(L.lib.pqlk_bro_forward(k, W, K, 2, L.ptr(arena), L.ptr(x), x.stride(0), m, EPS, slab.ptr if stash else None, q.ptr, st))
            res[f"bro_forward W={W} K={K} k={k} m={m} stash={stash}"] = dict(q=sha(q.full), stash=sha(slab.full))
    for W, K, k, m in t_bro_bf16.CASES:
        arena, x = draw(dev, 300 + W + K, L.lib.pqlk_bro_param_floats(k, W, K, 2)), x_of(dev, 200 + m, m, k)
        pk, q = Out(dev, L.lib.pqlk_bro_packed_bf16_elems(k, W, K, 2), torch.int16), Out(dev, 2 * m * 32)
        L.check(L.lib.pqlk_bro_pack_bf16(k, W, K, 2, L.ptr(arena), pk.ptr, st))
        L.check(L.lib.pqlk_bro_forward_bf16(k, W, K, 2, L.ptr(arena), pk.ptr, L.ptr(x), x.stride(0), m, EPS, q.ptr, st))
        res[f"bro_forward_bf16 W={W} K={K} k={k} m={m}"] = dict(packed=sha(pk.full), q=sha(q.full))


def stashed(dev, hidden, k, m):
    """-> (desc, arena, the slab of a stash forward on m rows, dq (2, m, 32))."""
    d, arena = ln_stack(dev, hidden, k)
    x = x_of(dev, 200 + m, m, k)
    slab, q = torch.zeros(int(L.lib.pqlk_lnmlp_stash_floats(C.byref(d), m)), device=dev), torch.zeros(2 * m * 32, device=dev)
    L.check(L.lib.pqlk_lnmlp_forward(C.byref(d), L.ptr(arena), L.ptr(x), x.stride(0), m, EPS, L.ptr(slab), L.ptr(q), L.stream(dev)))
    return d, arena, slab, draw(dev, 400 + m, 2 * m * 32, -1.0, 1.0)


def backward_cases(dev, res):
    st = L.stream(dev)
    for hidden, k, m, window in dxc.FORMS:
        d, arena, slab, dq = stashed(dev, hidden, k, m)
        col0, cols = window or (0, 0)
        ld_dx = (cols + 3) // 4 * 4 if window else L.ld(k)
        a = draw(dev, 500 + m, m * max(cols, 1), -1.0, 1.0) if window else None
        for r in (0, 1, 2):
            dx = Out(dev, m * ld_dx)
            code = L.lib.pqlk_lnmlp_dx(C.byref(d), L.ptr(arena), L.ptr(slab), L.ptr(dq), m, dx.ptr, ld_dx, col0, cols, L.ptr(a), cols, r, st)
            if code and r != 2:   # (r = 2 is refused where a 64-row block does not fit: recorded with its untouched output)
                L.check(code)
            res[f"lnmlp_dx hidden={hidden} k={k} m={m} window={window} r={r}"] = dict(rc=str(code), dx=sha(dx.full))
    for hidden, k, m in gc.GRAD_CASES:
        d, arena, slab, dq = stashed(dev, hidden, k, m)
        n_ws = int(L.lib.pqlk_lnmlp_grad_ws_floats(C.byref(d), m))
        for r in (0, 1, 2):
            ws, grads = Out(dev, n_ws), Out(dev, arena.numel())
            code = L.lib.pqlk_lnmlp_grad_chain(C.byref(d), L.ptr(arena), L.ptr(slab), L.ptr(dq), m, ws.ptr, n_ws, grads.ptr, r, st)
            if code and r != 2:
                L.check(code)
            res[f"lnmlp_grad_chain hidden={hidden} k={k} m={m} r={r}"] = dict(rc=str(code), ws=sha(ws.full), grads=sha(grads.full))


def mlp_bf16_cases(dev, res):
    st, dims = L.stream(dev), BF16_MLP_DIMS
    d = L.mlp_desc(dims, 2)
    arena = draw(dev, 600, L.lib.pqlk_mlp_param_floats(C.byref(d)))
    pk = Out(dev, L.lib.pqlk_mlp_packed_bf16_elems(C.byref(d)), torch.int16)
    L.check(L.lib.pqlk_mlp_pack_bf16(C.byref(d), L.ptr(arena), pk.ptr, st))
    for B in BF16_MLP_BS:
        x, out = x_of(dev, 200 + B, B, dims[0]), Out(dev, 2 * B * L.ld(dims[-1]))
        L.check(L.lib.pqlk_mlp_forward_bf16(C.byref(d), L.ptr(arena), pk.ptr, L.ptr(x), x.stride(0), B, L.ACT_NONE, None, 0.0, 0.0, out.ptr,
                                            None, 0, st))
        res[f"mlp_forward_bf16 dims={dims} B={B}"] = dict(packed=sha(pk.full), out=sha(out.full))


def compact(res):
    """{group: {cases, buffers, sha256 over the group's sorted "case/buffer=hash" lines}}, group = the first two words of the case."""
    groups = {}
    for case, bufs in res.items():
        groups.setdefault(" ".join(case.replace(", ", ",").split()[:2]), []).append((case, bufs))
    return {g: dict(cases=len(v), buffers=sum(len(b) for _, b in v),
                    sha256=hashlib.sha256("\n".join(sorted(f"{c}/{k}={h}" for c, b in v for k, h in b.items())).encode()).hexdigest())
            for g, v in groups.items()}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join("profiles", "stack_bits.json"))
    ap.add_argument("--label", default="", help="recorded in the output: which build this run hashed")
    ap.add_argument("--compact", action="store_true", help="one hash per group of cases instead of one per buffer")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("stack_bits.py needs a GPU: it hashes what the kernels write")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    res = {}
    ln_cases(dev, res)
    bro_cases(dev, res)
    backward_cases(dev, res)
    mlp_bf16_cases(dev, res)
    torch.cuda.synchronize()
    doc = dict(tool="tools/stack_bits.py", device=torch.cuda.get_device_name(dev), label=a.label, **(dict(groups=compact(res)) if a.compact else dict(hashes=res)))
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
