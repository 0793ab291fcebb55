"""`pqlk_bro_forward` (pql_amd/csrc/fwd_bro.hip), the one-launch forward of `DoubleQBroNet`, against a float64 torch model built from
the same arena views (`F.linear`, `F.layer_norm`, the skip), random normal inputs.  No tolerance is fixed in advance: the per-layer
forward's own error against that model is the bar, e_new <= 4 e_parent -- the two paths differ in the order of fp32 sums only."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

from support import dev  # noqa: F401

pytestmark = pytest.mark.gpu

# W, K, obs + act, m: one tile, one row / one row past it; two blocks at R = 2; 5 tiles on 8 waves, VPL 4; the R = 2 edge with 64 skip
# registers; R = 1 forced by the width, 3 tiles per wave; R = 1, VPL 16; 10 layers, past PQLK_MAX_LAYERS; no blocks
CASES = [(32, 1, 3, 1), (32, 1, 3, 33), (64, 2, 40, 65), (160, 1, 104, 129), (512, 2, 104, 65), (544, 1, 104, 33), (1024, 1, 104, 33),
         (64, 4, 40, 31), (64, 0, 40, 65)]
TAIL = 64   # sentinel floats behind every output block
WHICH = range(4)   # PQLK_LNMLP_Z, _Y, _MEAN, _RSTD


def _critics(W, K, k, dev):
    from pql_amd.models.bronet import DoubleQBroNet
    torch.manual_seed(W * 100 + K * 10 + k)
    per, fus = (DoubleQBroNet((k - 1,), 1, W, K, fused_forward=f).to(dev) for f in (False, True))
    for n in range(2):
        for l in range(2 * K + 1):
            per.norm_param(n, l, "gamma").add_(0.2 * torch.randn(W, device=dev))
            per.norm_param(n, l, "beta").copy_(0.2 * torch.randn(W, device=dev))
    fus.arena.data.copy_(per.arena.data)
    return per, fus


def _reference(q, x):
    """{("z" | "y", n, l): (m, W), ("q", n): (m,)} in float64."""
    from pql_amd.models.layernorm import LN_EPS
    out, H = {}, q.n_layers - 1
    for n in range(2):
        a = x.double()
        for l in range(H):
            z = F.linear(a, q.weight(n, l).double(), q.bias(n, l).double())
            t = F.layer_norm(z, z.shape[1:], q.norm_param(n, l, "gamma").double(), q.norm_param(n, l, "beta").double(), LN_EPS)
            a = out["y", n, l - 2] + t if q._closes_block(l) else F.elu(t)
            out["z", n, l], out["y", n, l] = z, a
        out["q", n] = F.linear(a, q.weight(n, H).double(), q.bias(n, H).double())[:, 0]
    return out


def _fused(q, x, stash=True):
    """The library call itself on sentinel-filled blocks -> (Q block (2, m, 32), stash slab or None), tails checked."""
    from pql_amd import _lib as L
    from pql_amd.models.layernorm import LN_EPS
    m = x.shape[0]
    qb = torch.full((2 * m * 32 + TAIL,), 7.0, device=x.device)
    slab = torch.full((int(L.lib.pqlk_bro_stash_floats(*q.fused[1:], m)) + TAIL,), 7.0, device=x.device) if stash else None
    L.check(L.lib.pqlk_bro_forward(*q.fused, L.ptr(q.arena.data), L.ptr(x), x.stride(0), m, LN_EPS, L.ptr(slab), L.ptr(qb), L.stream(x.device)))
    assert bool((qb[-TAIL:] == 7.0).all()) and (slab is None or bool((slab[-TAIL:] == 7.0).all()))   # nothing past the end is touched
    assert not bool((qb[:-TAIL] == 7.0).any())                                                        # and every row of Q is written
    return qb[:-TAIL].view(2, m, 32), slab


def _view(q, slab, m, n, l, which):
    from pql_amd import _lib as L
    off, ld = C.c_int64(), C.c_int64()
    L.check(L.lib.pqlk_bro_stash_offset(*q.fused[1:], m, n, l, which, C.byref(off), C.byref(ld)))
    assert off.value % 4 == 0
    return slab[off.value: off.value + m * ld.value].view(m, ld.value)


@pytest.mark.parametrize("W, K, k, m", CASES, ids=lambda v: str(v))
def test_fused_forward(W, K, k, m, dev):
    from pql_amd import _lib as L
    from pql_amd.models.layernorm import LN_EPS, lnmlp_desc
    from pql_amd.models.mlp import pad_cols
    per, fus = _critics(W, K, k, dev)
    H = 2 * K + 1
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
            z, y, mean, rstd = (_view(fus, slab, m, n, l, w) for w in WHICH)
            got["z", n, l], got["y", n, l], old["z", n, l], old["y", n, l] = z, y, ws["z"][(n, l)], ws["y"][(n, l)]
            # the epilogues are ln.hip's laws: its row kernels on the stashed z (and skip) give the stashed y, mean, rstd bit for bit
            y2, mean2, rstd2 = torch.empty_like(y), torch.empty(m, device=dev), torch.empty(m, device=dev)
            head = (L.ptr(z), W, m, W, L.ptr(fus.norm_param(n, l, "gamma")), L.ptr(fus.norm_param(n, l, "beta")), LN_EPS)
            tail = (L.ptr(y2), L.ptr(mean2), L.ptr(rstd2), L.stream(dev))
            if fus._closes_block(l):
                L.check(L.lib.pqlk_ln_res_forward(*head, L.ptr(got["y", n, l - 2]), *tail))
            else:
                L.check(L.lib.pqlk_ln_elu_forward(*head, *tail))
            assert torch.equal(y2, y) and torch.equal(mean2, mean[:, 0]) and torch.equal(rstd2, rstd[:, 0]), (n, l)
    # e_new <= 4 e_parent, per quantity (Q; z and y of each hidden layer), both nets together
    for kind in [("q",), *((t, l) for l in range(H) for t in "zy")]:
        keys = [(kind[0], n, *kind[1:]) for n in range(2)]
        e_new, e_parent = (max(float((d[key].double() - ref[key]).abs().max()) for key in keys) for d in (got, old))
        print(f"W={W} K={K} k={k} m={m} {kind}: e_new {e_new:.3e} e_parent {e_parent:.3e} ratio {e_new / e_parent if e_parent else float('inf'):.2f}")
        assert e_new <= 4.0 * e_parent, (kind, e_new, e_parent)
    if K == 0:   # the bits of pqlk_lnmlp_forward for [in, W, 1]
        d = lnmlp_desc([k, W, 1])
        q0, s0 = torch.zeros_like(qf), torch.full_like(slab[:-TAIL], 7.0)   # (the pad floats behind mean / rstd are written by neither)
        L.check(L.lib.pqlk_lnmlp_forward(C.byref(d), L.ptr(fus.arena.data), L.ptr(x), x.stride(0), m, LN_EPS, L.ptr(s0), L.ptr(q0), L.stream(dev)))
        assert s0.numel() == L.lib.pqlk_lnmlp_stash_floats(C.byref(d), m) and torch.equal(q0, qf) and torch.equal(s0, slab[:-TAIL])
    # bits: no stash; the same rows in a larger batch
    assert torch.equal(_fused(fus, x, stash=False)[0], qf)
    qb, slab_b = _fused(fus, big)
    assert torch.equal(qb[:, m + 3:], qf)
    for n in range(2):
        for l in range(H):
            for which in WHICH:
                assert torch.equal(_view(fus, slab_b, 2 * m + 3, n, l, which)[m + 3:], _view(fus, slab, m, n, l, which))


@pytest.mark.parametrize("W, K", [(48, 1), (1056, 1), (64, 17)], ids=["width48", "width1056", "blocks17"])
def test_ineligible_shapes_are_refused(W, K, dev):
    from pql_amd import _lib as L
    buf = torch.full((4096,), 7.0, device=dev)
    assert L.lib.pqlk_bro_ok(40, W, K, 2) == 0 and L.lib.pqlk_bro_param_floats(40, W, K, 2) == 0 and L.lib.pqlk_bro_stash_floats(W, K, 2, 4) == 0
    assert L.lib.pqlk_bro_forward(40, W, K, 2, L.ptr(buf), L.ptr(buf), 64, 4, 1e-5, None, L.ptr(buf), L.stream(dev)) == L.E_SHAPE
    assert bool((buf == 7.0).all())   # a refused call writes nothing
