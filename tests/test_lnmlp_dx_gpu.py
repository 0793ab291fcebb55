"""`pqlk_lnmlp_dx` (pql_amd/csrc/bwd_ln.hip), the one-launch input gradient of `DoubleQLayerNorm` with frozen parameters, against
float64 autograd (lnmlp_dx_cases.py).  No tolerance is fixed in advance: the per-layer `backward_raw(grads=None, need_dx=True)` on the
same arena and inputs sets the bar, e_new <= 4 e_parent -- the two paths differ in the order of fp32 sums only."""
import ctypes as C

import pytest
import torch

from lnmlp_dx_cases import FORMS, dx64
from support import dev  # noqa: F401

pytestmark = pytest.mark.gpu
TAIL, S = 64, 7.0   # sentinel floats behind the output, and the sentinel


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


def _dx(fus, x, dq, window, a, r):
    """The fused stash forward on x, then the library call itself on a sentinel-filled block -> (return code, (m, ld_dx) output)."""
    from pql_amd import _lib as L
    m, ld = x.shape[0], x.stride(0) if window is None else 32
    fus.forward_raw(x)
    out = torch.full((m * ld + TAIL,), S, device=x.device)
    col0, cols = window or (0, 0)
    rc = L.lib.pqlk_lnmlp_dx(C.byref(fus.fused), L.ptr(fus.arena.data), L.ptr(fus._workspace(m, x.device)["stash"]), L.ptr(dq), m,
                             L.ptr(out), ld, col0, cols, L.ptr(a), 0 if a is None else a.stride(0), r, L.stream(x.device))
    assert bool((out[-TAIL:] == S).all())   # nothing past row m is touched
    return rc, out[:-TAIL].view(m, ld)


@pytest.mark.parametrize("hidden, k, m, window", FORMS, ids=lambda v: str(v).replace(" ", ""))
def test_fused_dx(hidden, k, m, window, dev):
    from pql_amd import _lib as L
    from pql_amd.models.mlp import pad_cols
    per, fus = _critics(hidden, k, dev)
    M = 2 * m + 3
    big = pad_cols(torch.randn(M, k, device=dev), L.ld(k))
    dq_big = torch.zeros(2, M, 32, device=dev)
    dq_big[:, :, 0] = torch.randn(2, M, device=dev)
    a_big = None if window is None else torch.tanh(torch.randn(M, 32, device=dev))
    x, dq = big[m + 3:].contiguous(), dq_big[:, m + 3:].contiguous()   # the m rows, and the same rows inside a (2m + 3)-row batch
    a = None if window is None else a_big[m + 3:].contiguous()
    ref = dx64(per, x, dq)
    per.forward_raw(x)
    old = per.backward_raw(x, dq.clone(), grads=None, need_dx=True)
    rc, got = _dx(fus, x, dq, window, a, 0)
    assert rc == L.OK
    if window is None:
        assert bool((got[:, k:] == 0).all()) and not bool((got == S).any())   # pad columns zero, every row written
        got_v, old_v = got[:, :k], old[:, :k]
    else:
        col0, cols = window
        assert bool((got[:, cols:] == S).all())                                # columns [cols, ld_dx) stay
        ref = ref[:, col0:col0 + cols] * (1.0 - a[:, :cols].double() ** 2)
        got_v, old_v = got[:, :cols], old[:, col0:col0 + cols] * (1.0 - a[:, :cols] * a[:, :cols])
    e_new, e_parent = (float((v.double() - ref).abs().max()) for v in (got_v, old_v))
    print(f"{hidden} k={k} m={m} {window}: e_new {e_new:.3e} e_parent {e_parent:.3e} ratio {e_new / e_parent if e_parent else float('inf'):.2f}")
    assert e_new <= 4.0 * e_parent
    # bits: the same rows in a larger batch, and both block heights (64 rows only where the forward may take them)
    assert torch.equal(_dx(fus, big, dq_big, window, a_big, 0)[1][m + 3:], got)
    assert torch.equal(_dx(fus, x, dq, window, a, 1)[1], got)
    rc2, got2 = _dx(fus, x, dq, window, a, 2)
    assert (rc2 == L.E_SHAPE and bool((got2 == S).all())) if max(hidden) > 512 else (rc2 == L.OK and torch.equal(got2, got))


@pytest.mark.parametrize("dims, window, shift, code", [([40, 48, 1], (24, 16), 0, "E_SHAPE"), ([40, 64, 1], (30, 16), 0, "E_RANGE"),
                                                       ([40, 64, 1], (24, 16), 1, "E_ALIGN")], ids=["ineligible", "window", "misaligned_dx"])
def test_refusals(dims, window, shift, code, dev):
    from pql_amd import _lib as L
    from pql_amd.models.layernorm import lnmlp_desc
    buf = torch.zeros(8192, device=dev)
    rc = L.lib.pqlk_lnmlp_dx(C.byref(lnmlp_desc(dims)), L.ptr(buf), L.ptr(buf), L.ptr(buf), 4, L.ptr(buf[4096 + shift:]), 32, *window,
                             L.ptr(buf), 32, 0, L.stream(dev))
    assert rc == getattr(L, code)
