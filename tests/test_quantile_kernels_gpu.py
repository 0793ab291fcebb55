"""The quantile loss kernels (pqlk_qr_huber_loss, pqlk_qr_huber_loss_per, pqlk_dpg_loss_quantile) on the GPU against the float64
references of tests/quantile_cases.py: bit-equal on exactly representable data, within bounds computed from the reference
otherwise (derivations: quantile_cases.qr_bounds / dpg_loss_bound), with guarded output buffers."""
import ctypes as C

import numpy as np
import pytest
import torch

import quantile_cases as Q
from guarded import Guarded
from quantile_cases import _check_buffers, _heads
from reduction_cases import T
from support import dev  # noqa: F401

pytestmark = pytest.mark.gpu

E_NULL, E_SHAPE, E_ALIGN, E_UNSUPPORTED = 1, 2, 4, 5
RING = 5
# every B of {1, 3, 4, 5, 257, 4100} (the last: past the 1024-block cap at four rows per block) and every N of {2, 3, 31, 32, 33,
# 64} at least once; ld = pqlk_ld(N), and once a wider one (columns past lane 63 are pad columns too)
SHAPES = [(1, 2, None), (3, 3, None), (4, 31, None), (5, 32, None), (257, 64, None), (4100, 33, None), (5, 33, 96)]
GAMMA_N = 0.99 ** 3


@pytest.fixture(scope="module")
def L():
    from pql_amd import _lib
    return _lib


def _launch(L, dev, case, gamma_n, kappa, per=False, ld=None, ring=False, slot=0, dpg=False):
    """One launch on guarded outputs -> dict of what came back (numpy) and whether the guards are intact."""
    _, B, N = case["theta"].shape
    ld = L.ld(N) if ld is None else ld
    parts = int(L.lib.pqlk_loss_parts(B, N))
    th = _heads(dev, case["theta"], ld)
    dy = Guarded(dev, (2, B, ld), 777.0, init=np.full((2, B, ld), np.nan, np.float32))
    scratch = Guarded(dev, (parts,), 777.0, init=np.full(parts, np.nan, np.float32))
    abs_td = Guarded(dev, (B,), 777.0, init=np.full(B, np.nan, np.float32))
    out = torch.full((RING,), -7.0, dtype=torch.float32, device=dev)
    slot_dev = torch.tensor([slot], dtype=torch.int32, device=dev)
    tail = (L.ptr(out) if ring else None, L.ptr(slot_dev) if ring else None, RING if ring else 0, scratch.ptr)
    with torch.cuda.device(dev):
        if dpg:
            rc = L.lib.pqlk_dpg_loss_quantile(L.ptr(th), ld, N, B, dy.ptr, *tail, L.stream(dev))
        else:
            tt, rew, done = _heads(dev, case["theta_t"], ld), T(case["rew"]).to(dev), T(case["done"]).to(dev)
            head = (L.ptr(th), L.ptr(tt), ld, N, L.ptr(rew), L.ptr(done), gamma_n, kappa, B, dy.ptr, *tail)
            if per:
                w, wmax = T(case["w"]).to(dev), T(case["wmax"]).to(dev)
                rc = L.lib.pqlk_qr_huber_loss_per(*head, L.ptr(w), L.ptr(wmax), abs_td.ptr, L.stream(dev))
            else:
                rc = L.lib.pqlk_qr_huber_loss(*head, L.stream(dev))
        torch.cuda.synchronize(dev)
    assert rc == 0, rc
    full = dy.t.cpu().numpy()
    return dict(dy=full[:, :, :N], pad=full[:, :, N:], parts=scratch.t.cpu().numpy(), n_parts=parts, ring=out.cpu().numpy(),
                abs_td=abs_td.t.cpu().numpy(), intact=dy.intact() and scratch.intact() and abs_td.intact(), B=B, N=N)


# ------------------------------------------------------------------------------------------------ exact data
@pytest.mark.parametrize("B,N", [(16, 2), (64, 8), (16, 64), (2048, 32)])
def test_huber_dy_is_bit_equal_on_dyadic_data(L, dev, B, N):
    case = Q.dyadic_case(B, N, 11 * N + B)
    ref = Q.qr_huber_ref(case["theta"], case["theta_t"], case["rew"], case["done"], Q.DYADIC_GAMMA, Q.DYADIC_KAPPA)
    # the reference itself is exact in fp32: the targets, every k term, every partial sum in increasing k, the result
    assert Q.survives_fp32(ref["T"]) and Q.survives_fp32(ref["p"]) and Q.survives_fp32(np.cumsum(ref["p"], axis=3)) and Q.survives_fp32(ref["dy"])
    assert (ref["S"][0, :4] == ref["S"][1, :4]).all() and (ref["istar"][:4] == 0).all() and (ref["istar"][4:8] == 1).all()
    other = Q.qr_huber_ref(case["theta"], case["theta_t"], case["rew"], case["done"], Q.DYADIC_GAMMA, Q.DYADIC_KAPPA, force_net=1 - ref["istar"])
    assert all((other["dy"][:, row] != ref["dy"][:, row]).any() for row in range(8))   # the other net would show
    got = _launch(L, dev, case, Q.DYADIC_GAMMA, Q.DYADIC_KAPPA)
    _check_buffers(got)
    assert np.array_equal(got["dy"].astype(np.float64), ref["dy"])


@pytest.mark.parametrize("B,N", [(16, 2), (64, 8), (16, 64), (2048, 32)])
def test_dpg_shares_are_exact_on_dyadic_data(L, dev, B, N):
    case = Q.dyadic_case(B, N, 13 * N + B)
    ref = Q.dpg_quantile_ref(case["theta"])
    assert (ref["share"][:, 8:12] == 0.5).all() and (ref["share"][1, 12:16] == 1.0).all() and Q.survives_fp32(ref["dy"]) and Q.survives_fp32(ref["Q"])
    got = _launch(L, dev, case, 0.0, 1.0, dpg=True, ring=True)
    _check_buffers(got)
    assert np.array_equal(got["dy"].astype(np.float64), ref["dy"])
    # the row minima are multiples of 2^-4 / N below 2 and B of them stay below 2^24 units: every sum on the way is exact
    assert float(got["ring"][0]) == ref["loss"]


# ------------------------------------------------------------------------------------------------ general data
@pytest.mark.parametrize("per", [False, True])
@pytest.mark.parametrize("B,N,ld", SHAPES)
def test_huber_on_normal_data_within_the_rounding_bounds(L, dev, B, N, ld, per):
    case = Q.normal_case(B, N, 1000 + 7 * B + N, per=per)
    assert Q.margins_hold(case["theta_t"])   # |S_1 - S_0| >= 1e-3 (|S_0| + |S_1| + 1) on every row: no row is excluded below
    kappa = 1.0 if N != 31 else 0.5
    ref = Q.qr_huber_ref(case["theta"], case["theta_t"], case["rew"], case["done"], GAMMA_N, kappa, case.get("w"), case.get("wmax"))
    got = _launch(L, dev, case, GAMMA_N, kappa, per=per, ld=ld, ring=True, slot=7)
    _check_buffers(got, per)
    dy_b, loss_b, td_b = Q.qr_bounds(ref, got["n_parts"])
    err = np.abs(got["dy"].astype(np.float64) - ref["dy"])
    print(f"B={B} N={N} per={per}: max dy err / bound = {(err / np.maximum(dy_b, 1e-300)).max():.3f}; loss rel err = "
          f"{abs(float(got['ring'][2]) - ref['loss']) / ref['loss']:.3e}, bound {loss_b:.3e}")
    assert (err <= dy_b).all()
    assert abs(float(got["ring"][7 % RING]) - ref["loss"]) <= loss_b * ref["loss"]
    assert (np.delete(got["ring"], 7 % RING) == -7.0).all()   # the slot is slot_dev % ring_len, the others are untouched
    if per:
        assert (np.abs(got["abs_td"].astype(np.float64) - ref["abs_td"]) <= td_b).all()


@pytest.mark.parametrize("B,N,ld", SHAPES)
def test_dpg_on_normal_data(L, dev, B, N, ld):
    case = Q.normal_case(B, N, 2000 + 7 * B + N)
    assert Q.margins_hold(case["theta"])   # |Q_1 - Q_0| >= 1e-3 (|Q_0| + |Q_1| + 1) on every row
    ref = Q.dpg_quantile_ref(case["theta"])
    got = _launch(L, dev, case, 0.0, 1.0, ld=ld, ring=True, slot=3, dpg=True)
    _check_buffers(got)
    g = -(np.float32(1.0) / (np.float32(B) * np.float32(N)))   # the kernel's own constant; a share is 0 or 1 here
    assert np.array_equal(got["dy"], (ref["share"].astype(np.float32) * g)[:, :, None].repeat(N, axis=2))
    np.testing.assert_allclose(got["dy"], ref["dy"], rtol=3 * Q.U, atol=0)
    assert abs(float(got["ring"][3]) - ref["loss"]) <= Q.dpg_loss_bound(ref, got["n_parts"])


# ------------------------------------------------------------------------------------------------ loss outputs, repeatability
@pytest.mark.parametrize("B,N", [(5, 3), (4100, 33)])
def test_partials_fold_to_the_ring_value_and_launches_repeat(L, dev, B, N):
    case = Q.normal_case(B, N, 31, per=True)
    for kw, scale in ((dict(), np.float32(1.0) / (np.float32(B) * np.float32(N))), (dict(per=True), np.float32(1.0) / (np.float32(B) * np.float32(N))),
                      (dict(dpg=True), np.float32(-1.0) / np.float32(B))):
        bare = _launch(L, dev, case, GAMMA_N, 1.0, **kw)                       # loss_out = NULL: the partials stay in scratch
        assert bare["n_parts"] == min((B + 3) // 4, 1024) and (bare["ring"] == -7.0).all()
        ringed = _launch(L, dev, case, GAMMA_N, 1.0, ring=True, slot=RING + 1, **kw)
        assert np.array_equal(bare["parts"], ringed["parts"]) and np.array_equal(bare["dy"], ringed["dy"])   # two launches, the same bits
        assert np.array_equal(bare["abs_td"], ringed["abs_td"], equal_nan=True)
        assert ringed["ring"][1] == Q.fold_ref(bare["parts"], scale) and (np.delete(ringed["ring"], 1) == -7.0).all()


@pytest.mark.parametrize("B,N", [(5, 3), (257, 32), (4100, 64)])
def test_unit_weights_change_no_bit(L, dev, B, N):
    case = Q.normal_case(B, N, 41)
    case["w"], case["wmax"] = np.ones(B, np.float32), np.ones(1, np.float32)
    plain = _launch(L, dev, case, GAMMA_N, 1.0, ring=True)
    weighted = _launch(L, dev, case, GAMMA_N, 1.0, per=True, ring=True)
    assert np.array_equal(plain["dy"], weighted["dy"]) and np.array_equal(plain["parts"], weighted["parts"])
    assert np.array_equal(plain["ring"], weighted["ring"])


# ------------------------------------------------------------------------------------------------ errors
def test_errors_leave_the_outputs_untouched(L, dev):
    B, N, ld = 8, 8, 32
    case = Q.normal_case(B, N, 51, per=True)
    th, tt = _heads(dev, case["theta"], ld), _heads(dev, case["theta_t"], ld)
    rew, done, w, wmax = (T(case[k]).to(dev) for k in ("rew", "done", "w", "wmax"))
    dy, scratch, abs_td = (torch.full(s, 5.0, dtype=torch.float32, device=dev) for s in ((2, B, ld), (1024,), (B,)))
    out, slot = torch.full((RING,), 5.0, dtype=torch.float32, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
    ok = dict(theta=L.ptr(th), theta_t=L.ptr(tt), ld=ld, n=N, rew=L.ptr(rew), done=L.ptr(done), g=GAMMA_N, kappa=1.0, b=B, dy=L.ptr(dy),
              out=L.ptr(out), slot=L.ptr(slot), ring=RING, scratch=L.ptr(scratch), w=L.ptr(w), wmax=L.ptr(wmax), abs_td=L.ptr(abs_td))

    def huber(per, **k):
        a = dict(ok, **k)
        head = (a["theta"], a["theta_t"], a["ld"], a["n"], a["rew"], a["done"], a["g"], a["kappa"], a["b"], a["dy"], a["out"], a["slot"],
                a["ring"], a["scratch"])
        with torch.cuda.device(dev):
            if per:
                return L.lib.pqlk_qr_huber_loss_per(*head, a["w"], a["wmax"], a["abs_td"], L.stream(dev))
            return L.lib.pqlk_qr_huber_loss(*head, L.stream(dev))

    def dpg(**k):
        a = dict(ok, **k)
        with torch.cuda.device(dev):
            return L.lib.pqlk_dpg_loss_quantile(a["theta"], a["ld"], a["n"], a["b"], a["dy"], a["out"], a["slot"], a["ring"], a["scratch"],
                                                L.stream(dev))

    bad = [(dict(theta=None), E_NULL), (dict(dy=None), E_NULL), (dict(scratch=None), E_NULL), (dict(b=0), E_SHAPE), (dict(ring=0), E_SHAPE),
           (dict(ld=48), E_ALIGN), (dict(ld=32, n=33), E_ALIGN), (dict(n=1), E_UNSUPPORTED), (dict(n=65, ld=96), E_UNSUPPORTED)]
    for k, code in bad:
        assert huber(False, **k) == code and huber(True, **k) == code and dpg(**k) == code, k
    for k, code in [(dict(theta_t=None), E_NULL), (dict(rew=None), E_NULL), (dict(done=None), E_NULL), (dict(kappa=0.0), E_SHAPE),
                    (dict(kappa=-1.0), E_SHAPE)]:
        assert huber(False, **k) == code and huber(True, **k) == code, k
    for name in ("w", "wmax", "abs_td"):
        assert huber(True, **{name: None}) == E_NULL
    torch.cuda.synchronize(dev)
    for t in (dy, scratch, abs_td, out):
        assert (t == 5.0).all()
