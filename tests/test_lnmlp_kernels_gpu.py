"""`pqlk_lnmlp_forward` (pql_amd/csrc/fwd_ln.hip), the one-launch forward of `DoubleQLayerNorm`, against a float64 torch model built
from the same arena views (`F.linear`, `F.layer_norm`), random normal inputs.  No tolerance is fixed in advance: the per-layer
forward's own error against that model is the bar, e_new <= 4 e_parent -- the two paths differ in the order of fp32 sums only."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

from support import dev  # noqa: F401

pytestmark = pytest.mark.gpu

# hidden layers, obs + act, m: one tile and one row past it; two layers; ragged multiples of 32 on more than one block at R = 2 and
# R = 1 ... ; the R = 2 edge (64-row image of 512 columns); the R = 1 path with VPL = 16
CASES = [([32], 3, 1), ([32], 3, 33), ([64, 32], 40, 31), ([64, 32], 40, 65), ([160, 96], 104, 64), ([160, 96], 104, 129),
         ([512, 512, 256], 104, 65), ([1024], 104, 33)]
TAIL = 64   # sentinel floats behind every output block


def _critics(hidden, k, dev):
    from pql_amd.models.layernorm import DoubleQLayerNorm
    torch.manual_seed(len(hidden) * 1000 + k)
    per, fus = (DoubleQLayerNorm((k - 1,), 1, hidden, fused_forward=f).to(dev) for f in (False, True))
    for n in range(2):
        for l in range(len(hidden)):
            per.norm_param(n, l, "gamma").add_(0.2 * torch.randn(hidden[l], device=dev))
            per.norm_param(n, l, "beta").copy_(0.2 * torch.randn(hidden[l], device=dev))
    fus.arena.data.copy_(per.arena.data)
    return per, fus


def _reference(q, x):
    """{("z" | "y", n, l): (m, w), ("q", n): (m,)} in float64."""
    from pql_amd.models.layernorm import LN_EPS
    out, H = {}, q.n_layers - 1
    for n in range(2):
        a = x.double()
        for l in range(H):
            z = F.linear(a, q.weight(n, l).double(), q.bias(n, l).double())
            a = F.elu(F.layer_norm(z, z.shape[1:], q.norm_param(n, l, "gamma").double(), q.norm_param(n, l, "beta").double(), LN_EPS))
            out["z", n, l], out["y", n, l] = z, a
        out["q", n] = F.linear(a, q.weight(n, H).double(), q.bias(n, H).double())[:, 0]
    return out


def _fused(q, x, stash=True):
    """The library call itself on sentinel-filled blocks -> (Q block (2, m, 32), stash slab or None), tails checked."""
    from pql_amd import _lib as L
    from pql_amd.models.layernorm import LN_EPS
    m = x.shape[0]
    qb = torch.full((2 * m * 32 + TAIL,), 7.0, device=x.device)
    slab = torch.full((int(L.lib.pqlk_lnmlp_stash_floats(C.byref(q.fused), m)) + TAIL,), 7.0, device=x.device) if stash else None
    L.check(L.lib.pqlk_lnmlp_forward(C.byref(q.fused), L.ptr(q.arena.data), L.ptr(x), x.stride(0), m, LN_EPS, L.ptr(slab), L.ptr(qb),
                                     L.stream(x.device)))
    assert bool((qb[-TAIL:] == 7.0).all()) and (slab is None or bool((slab[-TAIL:] == 7.0).all()))   # nothing past row m is touched
    assert not bool((qb[:-TAIL] == 7.0).any())                                                        # and every row of Q is written
    return qb[:-TAIL].view(2, m, 32), slab


def _view(q, slab, m, n, l, which):
    from pql_amd import _lib as L
    off, ld = C.c_int64(), C.c_int64()
    L.check(L.lib.pqlk_lnmlp_stash_offset(C.byref(q.fused), m, n, l, which, C.byref(off), C.byref(ld)))
    assert off.value % 4 == 0
    return slab[off.value: off.value + m * ld.value].view(m, ld.value)


@pytest.mark.parametrize("hidden, k, m", CASES, ids=lambda v: str(v).replace(" ", ""))
def test_fused_forward(hidden, k, m, dev):
    from pql_amd import _lib as L
    from pql_amd.models.layernorm import LN_EPS
    from pql_amd.models.mlp import pad_cols
    per, fus = _critics(hidden, k, dev)
    H = len(hidden)
    big = pad_cols(torch.randn(2 * m + 3, k, device=dev), L.ld(k))
    x = big[m + 3:].contiguous()                       # the m rows, and the same rows at another place of a (2m + 3)-row batch
    ref = _reference(per, x[:, :k])
    q_per = per.forward_raw(x)
    ws = per._workspace(m, dev)
    qf, slab = _fused(fus, x)
    assert bool((qf[:, :, 1:] == 0).all())             # pad columns of Q
    got = {("q", n): qf[n, :, 0] for n in range(2)}
    old = {("q", n): q_per[n, :, 0] for n in range(2)}
    for n in range(2):
        for l in range(H):
            z, y = _view(fus, slab, m, n, l, L.LNMLP_Z), _view(fus, slab, m, n, l, L.LNMLP_Y)
            got["z", n, l], got["y", n, l], old["z", n, l], old["y", n, l] = z, y, ws["z"][(n, l)], ws["y"][(n, l)]
            # the epilogue is ln.hip's law: its row kernel on the stashed z gives the stashed y, mean, rstd bit for bit
            y2, mean, rstd = torch.empty_like(y), torch.empty(m, device=dev), torch.empty(m, device=dev)
            L.check(L.lib.pqlk_ln_elu_forward(L.ptr(z), hidden[l], m, hidden[l], L.ptr(fus.norm_param(n, l, "gamma")),
                                              L.ptr(fus.norm_param(n, l, "beta")), LN_EPS, L.ptr(y2), L.ptr(mean), L.ptr(rstd), L.stream(dev)))
            assert torch.equal(y2, y) and torch.equal(mean, _view(fus, slab, m, n, l, L.LNMLP_MEAN)[:, 0])
            assert torch.equal(rstd, _view(fus, slab, m, n, l, L.LNMLP_RSTD)[:, 0])
    # e_new <= 4 e_parent, per quantity (Q; z and y of each hidden layer), both nets together
    for kind in [("q",), *((t, l) for l in range(H) for t in "zy")]:
        keys = [(kind[0], n, *kind[1:]) for n in range(2)]
        e_new, e_parent = (max(float((d[key].double() - ref[key]).abs().max()) for key in keys) for d in (got, old))
        print(f"{hidden} k={k} m={m} {kind}: e_new {e_new:.3e} e_parent {e_parent:.3e} ratio {e_new / e_parent if e_parent else float('inf'):.2f}")
        assert e_new <= 4.0 * e_parent, (kind, e_new, e_parent)
    # bits: no stash; the same rows in a larger batch
    assert torch.equal(_fused(fus, x, stash=False)[0], qf)
    qb, slab_b = _fused(fus, big)
    assert torch.equal(qb[:, m + 3:], qf)
    for n in range(2):
        for l in range(H):
            for which in (L.LNMLP_Z, L.LNMLP_Y, L.LNMLP_MEAN, L.LNMLP_RSTD):
                assert torch.equal(_view(fus, slab_b, 2 * m + 3, n, l, which)[m + 3:], _view(fus, slab, m, n, l, which))


@pytest.mark.parametrize("dims", [[40, 48, 1], [40, 1056, 1], [40, 1]], ids=["width48", "width1056", "no_hidden"])
def test_ineligible_shapes_are_refused(dims, dev):
    from pql_amd import _lib as L
    from pql_amd.models.layernorm import lnmlp_desc
    d, buf = lnmlp_desc(dims), torch.zeros(4096, device=dev)
    assert L.lib.pqlk_lnmlp_ok(C.byref(d)) == 0 and L.lib.pqlk_lnmlp_stash_floats(C.byref(d), 4) == 0
    assert L.lib.pqlk_lnmlp_forward(C.byref(d), L.ptr(buf), L.ptr(buf), 64, 4, 1e-5, None, L.ptr(buf), L.stream(dev)) == L.E_SHAPE
