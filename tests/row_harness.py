"""Guarded, poisoned buffers and the two launchers of the LayerNorm row entries of pql_amd/csrc/ln.hip, for the kernel tests of every
critic class built on them (tests/test_layernorm_kernels_gpu.py, tests/test_droq_kernels_gpu.py, tests/test_bronet_kernels_gpu.py).
Pad columns of the inputs hold POISON too: an over-read moves a row sum by whole units, an over-write is seen.  `forward` and
`backward` take the entry's name and what it has beyond pqlk_ln_elu_forward / pqlk_ln_elu_backward."""
import torch

import layernorm_cases as lc
from guarded import Guarded, T

POISON = lc.POISON


def _layout(align, cols):
    from pql_amd import _lib as L
    return (cols + 3, 1) if align == "scalar" else (L.ld(cols), 0)


def _mat(dev, a, ld, off):
    """(m, cols) values in a guarded (m, ld) buffer whose pad columns hold POISON."""
    m, cols = a.shape
    g = Guarded(dev, (m, ld), POISON, off=off)
    g.t[:, :cols] = T(a).to(dev)
    return g


def _vec(dev, a, off):
    return Guarded(dev, a.shape, POISON, a, off)


def _pads_intact(g, cols):
    return g.intact() and bool((g.t[:, cols:] == POISON).all())


def _np(g, cols=None):
    a = g.t.cpu().numpy()
    return a if cols is None else a[:, :cols]


def forward(dev, entry, z, gamma, beta, align, eps=lc.EPS, extras=(), res=None, **keep):
    """`entry`(z, ld, m, cols, gamma, beta, eps, *extras, [res,] y, mean, rstd, stream) in guarded buffers.  Returns them by name, with
    ld, off and `keep` (what the backward needs again)."""
    from pql_amd import _lib as L
    m, cols = z.shape
    ld, off = _layout(align, cols)
    b = dict(ld=ld, off=off, **keep, z=_mat(dev, z, ld, off))
    if res is not None:
        b["res"] = _mat(dev, res, ld, off)
    b.update(gamma=_vec(dev, gamma, off), beta=_vec(dev, beta, off),
             y=Guarded(dev, (m, ld), POISON, off=off), mean=Guarded(dev, (m,), POISON, off=off), rstd=Guarded(dev, (m,), POISON, off=off))
    more = list(extras) + ([b["res"].ptr] if res is not None else [])
    L.check(getattr(L.lib, entry)(b["z"].ptr, ld, m, cols, b["gamma"].ptr, b["beta"].ptr, eps, *more, b["y"].ptr, b["mean"].ptr,
                                  b["rstd"].ptr, L.stream(dev)))
    torch.cuda.synchronize()
    return b


def backward(dev, entry, b, dy, extras=(), params=True, alias=False, summed=False, dy2=None, act=True, dsum=False, alias_dsum=False):
    """Backward of `forward`'s buffers through `entry`: (dy, y, z, ld, m, cols, mean, rstd, gamma, *extras, dz, dgamma, dbeta, scratch,
    stream), or for `summed` the form of pqlk_ln_sum_backward, (dy, dy2, y (act) or NULL, z, ..., gamma, dsum, dz, ...).  dz may alias
    dy (`alias`) and dsum dy2 (`alias_dsum`).  Returns the guarded (dy, dy2, dz, dsum, dgamma, dbeta, scratch); what was not asked
    for is None."""
    from pql_amd import _lib as L
    m, cols = dy.shape
    ld, off = b["ld"], b["off"]
    gdy = _mat(dev, dy, ld, off)
    gdy2 = _mat(dev, dy2, ld, off) if dy2 is not None else None
    gdz = gdy if alias else Guarded(dev, (m, ld), POISON, off=off)
    gds = None
    if dsum:
        gds = gdy2 if alias_dsum else Guarded(dev, (m, ld), POISON, off=off)
    dg = db = sc = None
    if params:
        dg, db = Guarded(dev, (cols,), POISON, off=off), Guarded(dev, (cols,), POISON, off=off)
        sc = Guarded(dev, (int(L.lib.pqlk_ln_scratch_floats(cols)),), POISON)
    p = lambda g: g.ptr if g is not None else None  # noqa: E731
    if summed:
        head = (gdy.ptr, p(gdy2), b["y"].ptr if act else None)
        out = (p(gds), gdz.ptr)
    else:
        head = (gdy.ptr, b["y"].ptr)
        out = (*extras, gdz.ptr)
    L.check(getattr(L.lib, entry)(*head, b["z"].ptr, ld, m, cols, b["mean"].ptr, b["rstd"].ptr, b["gamma"].ptr, *out, p(dg), p(db), p(sc),
                                  L.stream(dev)))
    torch.cuda.synchronize()
    return gdy, gdy2, gdz, gds, dg, db, sc


def _forward(dev, z, gamma, beta, align, eps=lc.EPS):
    return forward(dev, "pqlk_ln_elu_forward", z, gamma, beta, align, eps)


def _backward(dev, b, dy, params=True, alias=False):
    """Backward of `_forward`'s buffers.  Returns (dz buffer, dgamma, dbeta, scratch) -- guarded, the last three None without params."""
    _, _, gdz, _, dg, db, sc = backward(dev, "pqlk_ln_elu_backward", b, dy, params=params, alias=alias)
    return gdz, dg, db, sc
