"""The truncated pooled target kernels (pqlk_tqc_huber_loss, pqlk_tqc_huber_loss_per) on the GPU against the float64 reference of
tests/tqc_cases.py: bit-equal on exactly representable data for every valid d, within bounds computed from the reference otherwise
(derivation: tqc_cases.tqc_bounds), with guarded output buffers.  B of {1, 3, 4, 5, 257, 4100} (the last: past the 1024-block cap at
four rows per block) times N of {2, 3, 31, 32, 33, 64} (partial waves, a full wave: the 128-atom pool), d of {0, 1, N / 2, N - 1}."""
import numpy as np
import pytest
import torch

import quantile_cases as Q
import tqc_cases as TQ
from guarded import Guarded
from quantile_cases import _check_buffers, _heads
from reduction_cases import T
from support import dev  # noqa: F401

pytestmark = pytest.mark.gpu

E_NULL, E_SHAPE, E_ALIGN, E_UNSUPPORTED = 1, 2, 4, 5
RING = 5
BS, NS = (1, 3, 4, 5, 257, 4100), (2, 3, 31, 32, 33, 64)
GAMMA_N = 0.99 ** 3
WORST = dict(dy=0.0, loss=0.0, abs_td=0.0)   # the largest observed fraction of each bound, printed by the last normal-data case


@pytest.fixture(scope="module")
def L():
    from pql_amd import _lib
    return _lib


def _launch(L, dev, case, gamma_n, kappa, drop, per=False, ld=None, ring=False, slot=0):
    """One launch on guarded outputs -> dict of what came back (numpy) and whether the guards are intact."""
    _, B, N = case["theta"].shape
    ld = L.ld(N) if ld is None else ld
    parts = int(L.lib.pqlk_loss_parts(B, N))
    th, tt = _heads(dev, case["theta"], ld), _heads(dev, case["theta_t"], ld)
    rew, done = T(case["rew"]).to(dev), T(case["done"]).to(dev)
    dy = Guarded(dev, (2, B, ld), 777.0, init=np.full((2, B, ld), np.nan, np.float32))
    scratch = Guarded(dev, (parts,), 777.0, init=np.full(parts, np.nan, np.float32))
    abs_td = Guarded(dev, (B,), 777.0, init=np.full(B, np.nan, np.float32))
    out = torch.full((RING,), -7.0, dtype=torch.float32, device=dev)
    slot_dev = torch.tensor([slot], dtype=torch.int32, device=dev)
    head = (L.ptr(th), L.ptr(tt), ld, N, L.ptr(rew), L.ptr(done), gamma_n, kappa, B, dy.ptr, L.ptr(out) if ring else None,
            L.ptr(slot_dev) if ring else None, RING if ring else 0, scratch.ptr)
    with torch.cuda.device(dev):
        if per:
            w, wmax = T(case["w"]).to(dev), T(case["wmax"]).to(dev)
            rc = L.lib.pqlk_tqc_huber_loss_per(*head, L.ptr(w), L.ptr(wmax), abs_td.ptr, drop, L.stream(dev))
        else:
            rc = L.lib.pqlk_tqc_huber_loss(*head, drop, L.stream(dev))
        torch.cuda.synchronize(dev)
    assert rc == 0, rc
    full = dy.t.cpu().numpy()
    return dict(dy=full[:, :, :N], pad=full[:, :, N:], parts=scratch.t.cpu().numpy(), n_parts=parts, ring=out.cpu().numpy(),
                abs_td=abs_td.t.cpu().numpy(), intact=dy.intact() and scratch.intact() and abs_td.intact(), B=B, N=N)


# ------------------------------------------------------------------------------------------------ exact data
@pytest.mark.parametrize("B,N", [(16, 2), (64, 8), (16, 64), (2048, 32)])
def test_dy_is_bit_equal_on_dyadic_data_for_every_d(L, dev, B, N):
    """Every term and chain is exact, so dy is the reference's chain sums with the tail (/ kappa, * 1 / (B M), negation) in fp32.
    Rows 0 ... 3: equal atoms straddle the cut; 4 ... 7: done = 1; 8 ... 11: identical target nets.  A wrong kept set shows: two
    kept sets of one row that differ in an atom's value give another chain sum."""
    case = TQ.dyadic_case(B, N, 17 * N + B)
    base = TQ.tqc_base(case["theta"], case["theta_t"], case["rew"], case["done"], Q.DYADIC_GAMMA, Q.DYADIC_KAPPA, TQ.drops_for(N), terms=True)
    assert Q.survives_fp32(base["T"]) and Q.survives_fp32(base["p"])
    assert (case["done"][4:8] == 1).all() and np.array_equal(case["theta_t"][0, 8:12], case["theta_t"][1, 8:12])
    zs = np.sort(base["z"], axis=1)
    refs = {}
    for d in TQ.drops_for(N):
        ref = refs[d] = TQ.tqc_ref(base, d)
        M = ref["M"]
        assert Q.survives_fp32(np.cumsum(base["p"] * ref["keep"][None, :, None, :], axis=3))   # the chain in increasing p, dropped skipped
        if d > 0:
            assert (zs[:4, M - 1] == zs[:4, M]).any()   # equal atoms on both sides of the cut
        got = _launch(L, dev, case, Q.DYADIC_GAMMA, Q.DYADIC_KAPPA, d)
        _check_buffers(got)
        assert np.array_equal(got["dy"], TQ.dy_tail_fp32(ref["G"], Q.DYADIC_KAPPA, B, M)), d
        w = _launch(L, dev, dict(case, w=np.full(B, 0.5, np.float32), wmax=np.full(1, 2.0, np.float32)), Q.DYADIC_GAMMA, Q.DYADIC_KAPPA, d,
                    per=True)
        _check_buffers(w, per=True)
        assert np.array_equal(w["dy"], TQ.dy_tail_fp32(ref["G"], Q.DYADIC_KAPPA, B, M, np.full(B, 0.25, np.float32))), d
    live = case["done"] == 0
    for a in refs:   # the chain sums tell the kept sets apart (per kept atom: G / M), on rows whose targets differ
        for b in refs:
            if a < b:
                ga, gb = refs[a]["G"] / refs[a]["M"], refs[b]["G"] / refs[b]["M"]
                assert (ga != gb).any(axis=(0, 2))[live].mean() > 0.5


# ------------------------------------------------------------------------------------------------ general data
@pytest.mark.parametrize("B", BS)
@pytest.mark.parametrize("N", NS)
def test_normal_data_within_the_rounding_bounds(L, dev, B, N):
    """dy, the loss and |TD| of both instances at every d against the float64 law, inside tqc_cases.tqc_bounds."""
    case = Q.normal_case(B, N, 3000 + 7 * B + N, per=True)
    kappa = 1.0 if N != 31 else 0.5
    base = TQ.tqc_base(case["theta"], case["theta_t"], case["rew"], case["done"], GAMMA_N, kappa, TQ.drops_for(N))
    for d in TQ.drops_for(N):
        for per in (False, True):
            ref = TQ.tqc_ref(base, d, case["w"] if per else None, case["wmax"] if per else None)
            got = _launch(L, dev, case, GAMMA_N, kappa, d, per=per, ring=True, slot=7)
            _check_buffers(got, per)
            dy_b, loss_b, td_b = TQ.tqc_bounds(ref, got["n_parts"])
            err = np.abs(got["dy"].astype(np.float64) - ref["dy"])
            loss_err = abs(float(got["ring"][7 % RING]) - ref["loss"]) / ref["loss"]
            WORST["dy"] = max(WORST["dy"], float((err / np.maximum(dy_b, 1e-300)).max()))
            WORST["loss"] = max(WORST["loss"], loss_err / loss_b)
            assert (err <= dy_b).all(), (d, per)
            assert loss_err <= loss_b, (d, per)
            assert (np.delete(got["ring"], 7 % RING) == -7.0).all()   # the slot is slot_dev % ring_len, the others are untouched
            if per:
                td_err = np.abs(got["abs_td"].astype(np.float64) - ref["abs_td"])
                WORST["abs_td"] = max(WORST["abs_td"], float((td_err / td_b).max()))
                assert (td_err <= td_b).all(), d
    print(f"B={B} N={N}: largest fraction of the bound so far: dy {WORST['dy']:.3f}, loss {WORST['loss']:.3f}, |TD| {WORST['abs_td']:.3f}")


def test_a_wider_ld_and_the_fold(L, dev):
    """ld = 96 at N = 33 (columns past lane 63 are pad columns too); loss_out = NULL leaves the partials, the ring value is their fold
    with scale 1 / (B M), and the partial count is pqlk_loss_parts(b, N) whatever d; two launches give the same bits."""
    for B, N, ld in [(5, 33, 96), (4100, 33, None)]:
        case = Q.normal_case(B, N, 31, per=True)
        for d in (0, 5):
            scale = np.float32(1.0) / (np.float32(B) * np.float32(2 * (N - d)))
            for per in (False, True):
                bare = _launch(L, dev, case, GAMMA_N, 1.0, d, per=per, ld=ld)
                assert bare["n_parts"] == min((B + 3) // 4, 1024) and (bare["ring"] == -7.0).all()
                ringed = _launch(L, dev, case, GAMMA_N, 1.0, d, per=per, ld=ld, ring=True, slot=RING + 1)
                _check_buffers(ringed, per)
                assert np.array_equal(bare["parts"], ringed["parts"]) and np.array_equal(bare["dy"], ringed["dy"])
                assert np.array_equal(bare["abs_td"], ringed["abs_td"], equal_nan=True)
                assert ringed["ring"][1] == Q.fold_ref(bare["parts"], scale) and (np.delete(ringed["ring"], 1) == -7.0).all()


@pytest.mark.parametrize("B,N,d", [(5, 3, 1), (257, 32, 2), (4100, 64, 32)])
def test_unit_weights_change_no_bit(L, dev, B, N, d):
    case = Q.normal_case(B, N, 41)
    case["w"], case["wmax"] = np.ones(B, np.float32), np.ones(1, np.float32)
    plain = _launch(L, dev, case, GAMMA_N, 1.0, d, ring=True)
    weighted = _launch(L, dev, case, GAMMA_N, 1.0, d, per=True, ring=True)
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
              out=L.ptr(out), slot=L.ptr(slot), ring=RING, scratch=L.ptr(scratch), w=L.ptr(w), wmax=L.ptr(wmax), abs_td=L.ptr(abs_td), drop=2)

    def huber(per, **k):
        a = dict(ok, **k)
        head = (a["theta"], a["theta_t"], a["ld"], a["n"], a["rew"], a["done"], a["g"], a["kappa"], a["b"], a["dy"], a["out"], a["slot"],
                a["ring"], a["scratch"])
        with torch.cuda.device(dev):
            if per:
                return L.lib.pqlk_tqc_huber_loss_per(*head, a["w"], a["wmax"], a["abs_td"], a["drop"], L.stream(dev))
            return L.lib.pqlk_tqc_huber_loss(*head, a["drop"], L.stream(dev))

    bad = [(dict(theta=None), E_NULL), (dict(theta_t=None), E_NULL), (dict(rew=None), E_NULL), (dict(done=None), E_NULL), (dict(dy=None), E_NULL),
           (dict(scratch=None), E_NULL), (dict(b=0), E_SHAPE), (dict(ring=0), E_SHAPE), (dict(kappa=0.0), E_SHAPE), (dict(kappa=-1.0), E_SHAPE),
           (dict(ld=48), E_ALIGN), (dict(ld=32, n=33), E_ALIGN), (dict(n=1, drop=0), E_UNSUPPORTED), (dict(n=65, ld=96), E_UNSUPPORTED),
           (dict(drop=-1), E_SHAPE), (dict(drop=N), E_SHAPE), (dict(drop=N + 1), E_SHAPE)]
    for k, code in bad:
        assert huber(False, **k) == code and huber(True, **k) == code, k
    for name in ("w", "wmax", "abs_td"):
        assert huber(True, **{name: None}) == E_NULL
    torch.cuda.synchronize(dev)
    for t in (dy, scratch, abs_td, out):
        assert (t == 5.0).all()
