"""`pqlk_lnmlp_grad_chain` (pql_amd/csrc/bwd_ln.hip) and `DoubleQLayerNorm(fused_backward=True)`, the one-launch gradient chain of the
critic's own update, against float64 autograd over every parameter (lnmlp_grad_cases.py).  No tolerance is fixed in advance: the per-layer
`backward_raw(grads=...)` on the same arena and inputs sets the bar per parameter group, e_new <= 4 e_parent -- the two paths differ in
the order of fp32 sums only."""
import ctypes as C

import pytest
import torch

from lnmlp_grad_cases import GRAD_CASES, GROUPS, grads64, group_errors
from support import dev  # noqa: F401

pytestmark = pytest.mark.gpu
TAIL, S = 64, 7.0   # sentinel floats behind an output, and the sentinel
IDS = dict(ids=lambda v: str(v).replace(" ", ""))


def _critics(hidden, k, dev):
    from pql_amd.models.layernorm import DoubleQLayerNorm
    torch.manual_seed(len(hidden) * 1000 + k)
    per, fus = (DoubleQLayerNorm((k - 1,), 1, hidden, fused_forward=f, fused_backward=f).to(dev) for f in (False, True))
    for n in range(2):
        for l in range(len(hidden)):
            per.norm_param(n, l, "gamma").add_(0.2 * torch.randn(hidden[l], device=dev))
            per.norm_param(n, l, "beta").copy_(0.2 * torch.randn(hidden[l], device=dev))
    fus.arena.data.copy_(per.arena.data)
    return per, fus


def _inputs(k, m, dev):
    """x, dq of M = 2 m + 3 rows, and their last m rows as a batch of its own."""
    from pql_amd import _lib as L
    from pql_amd.models.mlp import pad_cols
    M = 2 * m + 3
    big = pad_cols(torch.randn(M, k, device=dev), L.ld(k))
    dq_big = torch.zeros(2, M, 32, device=dev)
    dq_big[:, :, 0] = torch.randn(2, M, device=dev)
    return big, dq_big, big[m + 3:].contiguous(), dq_big[:, m + 3:].contiguous()


def _chain(fus, x, dq, r):
    """The fused stash forward on x, then the library call itself on sentinel-filled blocks -> (code, dz matrices, grads); the sentinels
    behind both blocks, the Linear slots of grads and the stash must come out as they went in."""
    from pql_amd import _lib as L
    m, d = x.shape[0], C.byref(fus.fused)
    fus.forward_raw(x)
    stash = fus._workspace(m, x.device)["stash"]
    before, need = stash.clone(), int(L.lib.pqlk_lnmlp_grad_ws_floats(d, m))
    ws, grads = torch.full((need + TAIL,), S, device=x.device), torch.full((fus.total + TAIL,), S, device=x.device)
    rc = L.lib.pqlk_lnmlp_grad_chain(d, L.ptr(fus.arena.data), L.ptr(stash), L.ptr(dq), m, L.ptr(ws), need, L.ptr(grads), r, L.stream(x.device))
    norm = torch.zeros(fus.total + TAIL, dtype=torch.bool, device=x.device)
    dz = []
    for n in range(2):
        for l in range(fus.n_layers - 1):
            off, ld = C.c_int64(), C.c_int64()
            assert L.lib.pqlk_lnmlp_grad_offset(d, m, n, l, C.byref(off), C.byref(ld)) == L.OK and off.value % 4 == 0
            dz.append(ws[off.value: off.value + m * ld.value])
            for which in ("gamma", "beta"):
                fus.norm_param(n, l, which, norm).fill_(True)
    assert bool((ws[need:] == S).all()) and bool((grads[~norm] == S).all()) and torch.equal(stash, before)
    return rc, torch.cat(dz), grads[norm]


@pytest.mark.parametrize("hidden, k, m", GRAD_CASES, **IDS)
def test_fused_backward(hidden, k, m, dev):
    per, fus = _critics(hidden, k, dev)
    _, _, x, dq = _inputs(k, m, dev)
    ref = grads64(per, x, dq)
    got = {}
    for name, q in (("parent", per), ("new", fus), ("again", fus)):
        q.forward_raw(x)
        g = torch.full((q.total + TAIL,), S, device=dev)
        assert q.backward_raw(x, dq.clone(), grads=g[:q.total]) is None and bool((g[q.total:] == S).all())
        got[name] = g
    assert torch.equal(got["new"] == S, got["parent"] == S)   # written where the per-layer path writes, pads included
    assert torch.equal(got["new"], got["again"])
    e_new, e_parent = (group_errors(per, got[name][:per.total], ref) for name in ("new", "parent"))
    for grp in GROUPS:
        print(f"{hidden} k={k} m={m} {grp}: e_new {e_new[grp]:.3e} e_parent {e_parent[grp]:.3e} "
              f"ratio {e_new[grp] / e_parent[grp] if e_parent[grp] else float('nan'):.2f}")
    for grp in GROUPS:
        assert e_new[grp] <= 4.0 * e_parent[grp], grp


@pytest.mark.parametrize("hidden, k, m", GRAD_CASES, **IDS)
def test_chain_bits(hidden, k, m, dev):
    from pql_amd import _lib as L
    _, fus = _critics(hidden, k, dev)
    big, dq_big, x, dq = _inputs(k, m, dev)
    rc, dz, gb = _chain(fus, x, dq, 0)
    assert rc == L.OK and not bool((dz == S).any()) and not bool((gb == S).any())
    # both block heights (64 rows only where the image and the table allow them), and the same rows inside a larger batch
    rc1, dz1, gb1 = _chain(fus, x, dq, 1)
    assert rc1 == L.OK and torch.equal(dz1, dz) and torch.equal(gb1, gb)
    rc2, dz2, gb2 = _chain(fus, x, dq, 2)
    if max(hidden) > 512:
        assert rc2 == L.E_SHAPE and bool((dz2 == S).all()) and bool((gb2 == S).all())
    else:
        assert rc2 == L.OK and torch.equal(dz2, dz) and torch.equal(gb2, gb)
    M, rows = big.shape[0], []
    _, dz_big, _ = _chain(fus, big, dq_big, 0)
    for w in hidden * 2:   # (net 0's layers, then net 1's: the order of `_chain`)
        rows.append(dz_big[:M * w].view(M, w)[m + 3:].reshape(-1))
        dz_big = dz_big[M * w:]
    assert torch.equal(torch.cat(rows), dz)


@pytest.mark.parametrize("dims, short, shift, null, code", [([40, 48, 1], 0, 0, False, "E_SHAPE"), ([40, 64, 1], 1, 0, False, "E_SHAPE"),
                                                            ([40, 64, 1], 0, 1, False, "E_ALIGN"), ([40, 64, 1], 0, 0, True, "E_NULL")],
                         ids=["ineligible", "ws_one_short", "misaligned_ws", "null_grads"])
def test_refusals(dims, short, shift, null, code, dev):
    from pql_amd import _lib as L
    from pql_amd.models.layernorm import lnmlp_desc
    d, m = lnmlp_desc(dims), 4
    need = int(L.lib.pqlk_lnmlp_grad_ws_floats(C.byref(lnmlp_desc([40, 64, 1])), m))
    assert need == 2 * (m + 2) * 64 and int(L.lib.pqlk_lnmlp_grad_ws_floats(C.byref(lnmlp_desc([40, 48, 1])), m)) == 0
    buf, ws, grads = torch.zeros(16384, device=dev), torch.full((need + 8,), S, device=dev), torch.full((16384,), S, device=dev)
    rc = L.lib.pqlk_lnmlp_grad_chain(C.byref(d), L.ptr(buf), L.ptr(buf), L.ptr(buf), m, L.ptr(ws[shift:]), need - short,
                                     None if null else L.ptr(grads), 0, L.stream(dev))
    assert rc == getattr(L, code) and bool((ws == S).all()) and bool((grads == S).all())
