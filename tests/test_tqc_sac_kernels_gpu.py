"""The TQC agent's loss kernels on the GPU (pqlk_tqc_huber_loss_soft, pqlk_tqc_huber_loss_soft_per, pqlk_dpg_loss_quantile_mean)
against the float64 references of tests/tqc_sac_cases.py: bit-equal on exactly representable data for every valid d, bit-equal to the
entries without the shift when every log-probability is zero, within bounds computed from the reference otherwise (derivation:
tqc_sac_cases.soft_bounds over tqc_cases.tqc_bounds), with guarded output buffers.  Shapes are those of tests/test_tqc_kernels_gpu.py:
B of {1, 3, 4, 5, 257, 4100} (the last: past the 1024-block cap at four rows per block) times N of {2, 3, 31, 32, 33, 64}, d of
{0, 1, N / 2, N - 1}."""
import numpy as np
import pytest
import torch

import quantile_cases as Q
import tqc_cases as TQ
import tqc_sac_cases as TS
from guarded import Guarded
from quantile_cases import _check_buffers, _heads
from reduction_cases import T
from support import dev  # noqa: F401

pytestmark = pytest.mark.gpu

E_NULL, E_SHAPE, E_ALIGN, E_UNSUPPORTED = 1, 2, 4, 5
RING = 5
BS, NS = (1, 3, 4, 5, 257, 4100), (2, 3, 31, 32, 33, 64)
GAMMA_N = 0.99 ** 3
LOG_ALPHA = float(np.log(0.2))
WORST = dict(dy=0.0, loss=0.0, abs_td=0.0)   # the largest observed fraction of each bound, printed by every normal-data case


@pytest.fixture(scope="module")
def L():
    from pql_amd import _lib
    return _lib


def _launch(L, dev, case, gamma_n, kappa, drop, per=False, ld=None, ring=False, slot=0, entry="soft"):
    """One launch on guarded outputs -> dict of what came back (numpy) and whether the guards are intact.  entry: "soft" (the entries
    under test; case["logp"], case["log_alpha"]), "hard" (pqlk_tqc_huber_loss{,_per} on the same inputs) or "mean" (the actor loss)."""
    _, B, N = case["theta"].shape
    ld = L.ld(N) if ld is None else ld
    parts = int(L.lib.pqlk_loss_parts(B, N))
    th = _heads(dev, case["theta"], ld)
    dy = Guarded(dev, (2, B, ld), 777.0, init=np.full((2, B, ld), np.nan, np.float32))
    scratch = Guarded(dev, (parts,), 777.0, init=np.full(parts, np.nan, np.float32))
    abs_td = Guarded(dev, (B,), 777.0, init=np.full(B, np.nan, np.float32))
    out = torch.full((RING,), -7.0, dtype=torch.float32, device=dev)
    slot_dev = torch.tensor([slot], dtype=torch.int32, device=dev)
    tail = (dy.ptr, L.ptr(out) if ring else None, L.ptr(slot_dev) if ring else None, RING if ring else 0, scratch.ptr)
    with torch.cuda.device(dev):
        if entry == "mean":
            rc = L.lib.pqlk_dpg_loss_quantile_mean(L.ptr(th), ld, N, B, *tail, L.stream(dev))
        else:
            tt = _heads(dev, case["theta_t"], ld)
            rew, done = T(case["rew"]).to(dev), T(case["done"]).to(dev)
            head = (L.ptr(th), L.ptr(tt), ld, N, L.ptr(rew), L.ptr(done), gamma_n, kappa, B, *tail)
            w, wmax = (T(case["w"]).to(dev), T(case["wmax"]).to(dev)) if per else (None, None)
            pw = (L.ptr(w), L.ptr(wmax), abs_td.ptr) if per else ()
            if entry == "soft":
                logp = T(np.asarray(case["logp"], np.float32)).to(dev)
                la = torch.tensor([case["log_alpha"]], dtype=torch.float32, device=dev)
                fn = L.lib.pqlk_tqc_huber_loss_soft_per if per else L.lib.pqlk_tqc_huber_loss_soft
                rc = fn(*head, *pw, L.ptr(logp), L.ptr(la), drop, L.stream(dev))
            else:
                fn = L.lib.pqlk_tqc_huber_loss_per if per else L.lib.pqlk_tqc_huber_loss
                rc = fn(*head, *pw, drop, L.stream(dev))
        torch.cuda.synchronize(dev)
    assert rc == 0, rc
    full = dy.t.cpu().numpy()
    return dict(dy=full[:, :, :N], pad=full[:, :, N:], parts=scratch.t.cpu().numpy(), n_parts=parts, ring=out.cpu().numpy(),
                abs_td=abs_td.t.cpu().numpy(), intact=dy.intact() and scratch.intact() and abs_td.intact(), B=B, N=N)


# ------------------------------------------------------------------------------------------------ exact data
@pytest.mark.parametrize("B,N", [(16, 2), (64, 8), (16, 64), (2048, 32)])
def test_soft_dy_is_bit_equal_on_dyadic_data_for_every_d(L, dev, B, N):
    """tqc_cases.dyadic_case (ties straddling every cut, done = 1 rows, identical target nets) with log_alpha = 0 -- expf is exactly 1
    on host and device -- and log-probabilities that are multiples of 2^-4 of both signs: every term and chain is exact, so dy is
    the reference's chain sums with the tail in fp32.  A shift that was left out, applied twice or given the wrong sign shows: it
    moves every target of a live row by a multiple of 2^-5."""
    case = dict(TQ.dyadic_case(B, N, 17 * N + B), logp=TS.logp_dyadic(B, N + B), log_alpha=0.0)
    drops = TQ.drops_for(N)
    base = TS.soft_base(case["theta"], case["theta_t"], case["rew"], case["done"], case["logp"], 0.0, Q.DYADIC_GAMMA, Q.DYADIC_KAPPA, drops, terms=True)
    hard = TQ.tqc_base(case["theta"], case["theta_t"], case["rew"], case["done"], Q.DYADIC_GAMMA, Q.DYADIC_KAPPA, drops)
    assert Q.survives_fp32(base["s"]) and Q.survives_fp32(base["T"]) and Q.survives_fp32(base["p"])
    assert (case["logp"] > 0).any() and (case["logp"] < 0).any()
    assert (case["done"][4:8] == 1).all() and np.array_equal(case["theta_t"][0, 8:12], case["theta_t"][1, 8:12])
    zs = np.sort(base["z"], axis=1)
    live = (case["done"] == 0) & (case["logp"] != 0)
    for d in drops:
        ref = TS.soft_ref(base, d)
        M = ref["M"]
        assert Q.survives_fp32(np.cumsum(base["p"] * ref["keep"][None, :, None, :], axis=3))   # the chain in increasing p, dropped skipped
        if d > 0:
            assert (zs[:4, M - 1] == zs[:4, M]).any()   # equal atoms on both sides of the cut
        assert (ref["G"] != TQ.tqc_ref(hard, d)["G"]).any(axis=(0, 2))[live].mean() > 0.5   # the shift shows in the chain sums
        got = _launch(L, dev, case, Q.DYADIC_GAMMA, Q.DYADIC_KAPPA, d)
        _check_buffers(got)
        assert np.array_equal(got["dy"], TQ.dy_tail_fp32(ref["G"], Q.DYADIC_KAPPA, B, M)), d
        w = _launch(L, dev, dict(case, w=np.full(B, 0.5, np.float32), wmax=np.full(1, 2.0, np.float32)), Q.DYADIC_GAMMA, Q.DYADIC_KAPPA, d,
                    per=True)
        _check_buffers(w, per=True)
        assert np.array_equal(w["dy"], TQ.dy_tail_fp32(ref["G"], Q.DYADIC_KAPPA, B, M, np.full(B, 0.25, np.float32))), d


@pytest.mark.parametrize("B", BS)
@pytest.mark.parametrize("N", NS)
def test_mean_actor_dy_is_bit_equal_for_every_shape(L, dev, B, N):
    """dy does not depend on the values: -(1.0f / ((float)B * (float)(2 N))) in every column below N, zero pad columns, intact guards;
    the loss inside the bound of the reference (tqc_sac_cases.dpg_mean_loss_bound)."""
    case = Q.normal_case(B, N, 2000 + 7 * B + N)
    ref = TS.dpg_mean_ref(case["theta"])
    got = _launch(L, dev, case, 0.0, 1.0, 0, ring=True, slot=3, entry="mean")
    _check_buffers(got)
    assert np.array_equal(got["dy"], np.full((2, B, N), TS.dpg_mean_dy_fp32(B, N), np.float32))
    np.testing.assert_allclose(got["dy"], ref["dy"], rtol=3 * Q.U, atol=0)
    assert abs(float(got["ring"][3]) - ref["loss"]) <= TS.dpg_mean_loss_bound(ref, got["n_parts"])
    assert (np.delete(got["ring"], 3) == -7.0).all()


@pytest.mark.parametrize("B,N", [(16, 2), (64, 8), (16, 64), (2048, 32)])
def test_mean_actor_loss_is_bit_equal_on_dyadic_data(L, dev, B, N):
    """theta multiples of 2^-4 below 2, N and B powers of two: 2 N B of them stay below 2^24 units, every sum on the way is exact and
    both scales are powers of two."""
    case = Q.dyadic_case(B, N, 13 * N + B)
    ref = TS.dpg_mean_ref(case["theta"])
    assert Q.survives_fp32(ref["Qbar"]) and Q.survives_fp32(ref["loss"]) and Q.survives_fp32(ref["dy"])
    assert not np.isclose(ref["loss"], Q.dpg_quantile_ref(case["theta"])["loss"])   # the min-of-means law would show
    got = _launch(L, dev, case, 0.0, 1.0, 0, ring=True, entry="mean")
    _check_buffers(got)
    assert float(got["ring"][0]) == ref["loss"]
    assert np.array_equal(got["dy"].astype(np.float64), ref["dy"])
    bare = _launch(L, dev, case, 0.0, 1.0, 0, entry="mean")   # loss_out = NULL: the partials stay, their fold (-1 / B) is the ring value
    assert (bare["ring"] == -7.0).all() and np.array_equal(bare["parts"], got["parts"])
    assert got["ring"][0] == Q.fold_ref(bare["parts"], np.float32(-1.0) / np.float32(B))


# ------------------------------------------------------------------------------------------------ ties to the tested instances
@pytest.mark.parametrize("B,N,d", [(5, 3, 1), (257, 32, 2), (257, 33, 16), (4100, 64, 32), (4100, 31, 0)])
def test_zero_log_probabilities_change_no_bit(L, dev, B, N, d):
    """logp = 0 everywhere, any log_alpha: z - 0 is z, so dy, the partials, the loss and |TD| are the bits of the entries without the
    shift on the same inputs -- which tests/test_tqc_kernels_gpu.py holds to the reference."""
    case = dict(Q.normal_case(B, N, 61, per=True), logp=np.zeros(B, np.float32))
    for per in (False, True):
        hard = _launch(L, dev, case, GAMMA_N, 1.0, d, per=per, ring=True, entry="hard")
        for la in (0.0, LOG_ALPHA, 3.0):
            soft = _launch(L, dev, dict(case, log_alpha=la), GAMMA_N, 1.0, d, per=per, ring=True)
            _check_buffers(soft, per)
            assert np.array_equal(soft["dy"], hard["dy"]) and np.array_equal(soft["parts"], hard["parts"]), (per, la)
            assert np.array_equal(soft["ring"], hard["ring"]) and np.array_equal(soft["abs_td"], hard["abs_td"], equal_nan=True), (per, la)


@pytest.mark.parametrize("B,N,d", [(5, 3, 1), (257, 32, 2), (4100, 64, 32)])
def test_unit_weights_change_no_bit(L, dev, B, N, d):
    case = dict(Q.normal_case(B, N, 41), logp=TS.logp_normal(B, 43), log_alpha=LOG_ALPHA)
    case["w"], case["wmax"] = np.ones(B, np.float32), np.ones(1, np.float32)
    plain = _launch(L, dev, case, GAMMA_N, 1.0, d, ring=True)
    weighted = _launch(L, dev, case, GAMMA_N, 1.0, d, per=True, ring=True)
    assert np.array_equal(plain["dy"], weighted["dy"]) and np.array_equal(plain["parts"], weighted["parts"])
    assert np.array_equal(plain["ring"], weighted["ring"])
    hard = _launch(L, dev, case, GAMMA_N, 1.0, d, ring=True, entry="hard")
    assert not np.array_equal(plain["dy"], hard["dy"])   # (and the shift is there)


# ------------------------------------------------------------------------------------------------ general data
@pytest.mark.parametrize("B", BS)
@pytest.mark.parametrize("N", NS)
def test_normal_data_within_the_rounding_bounds(L, dev, B, N):
    """dy, the loss and |TD| of both instances at every d against the float64 law with log_alpha = log 0.2, inside
    tqc_sac_cases.soft_bounds: f18's bounds with the target's error enlarged by one rounding for alpha * logp, one for the subtraction
    and a 1-ulp expf."""
    case = dict(Q.normal_case(B, N, 3000 + 7 * B + N, per=True), logp=TS.logp_normal(B, 4000 + 7 * B + N), log_alpha=LOG_ALPHA)
    kappa = 1.0 if N != 31 else 0.5
    base = TS.soft_base(case["theta"], case["theta_t"], case["rew"], case["done"], case["logp"], LOG_ALPHA, GAMMA_N, kappa, TQ.drops_for(N))
    for d in TQ.drops_for(N):
        for per in (False, True):
            ref = TS.soft_ref(base, d, case["w"] if per else None, case["wmax"] if per else None)
            got = _launch(L, dev, case, GAMMA_N, kappa, d, per=per, ring=True, slot=7)
            _check_buffers(got, per)
            dy_b, loss_b, td_b = TS.soft_bounds(ref, got["n_parts"])
            err = np.abs(got["dy"].astype(np.float64) - ref["dy"])
            loss_err = abs(float(got["ring"][7 % RING]) - ref["loss"]) / ref["loss"]
            WORST["dy"] = max(WORST["dy"], float((err / np.maximum(dy_b, 1e-300)).max()))
            WORST["loss"] = max(WORST["loss"], loss_err / loss_b)
            td_err = np.abs(got["abs_td"].astype(np.float64) - ref["abs_td"]) if per else None
            if per:
                WORST["abs_td"] = max(WORST["abs_td"], float((td_err / td_b).max()))
            print(f"B={B} N={N} d={d} per={per}: dy {float((err / np.maximum(dy_b, 1e-300)).max()):.3f} of its bound, loss {loss_err / loss_b:.3f}"
                  + (f", |TD| {float((td_err / td_b).max()):.3f}" if per else ""))
            assert (err <= dy_b).all(), (d, per)
            assert loss_err <= loss_b, (d, per)
            assert (np.delete(got["ring"], 7 % RING) == -7.0).all()   # the slot is slot_dev % ring_len, the others are untouched
            if per:
                assert (td_err <= td_b).all(), d
    print(f"B={B} N={N}: largest fraction of the bound so far: dy {WORST['dy']:.3f}, loss {WORST['loss']:.3f}, |TD| {WORST['abs_td']:.3f}")


def test_a_wider_ld_and_the_fold(L, dev):
    """ld = 96 at N = 33; loss_out = NULL leaves the partials, the ring value is their fold with scale 1 / (B M); two launches give the
    same bits."""
    for B, N, ld in [(5, 33, 96), (4100, 33, None)]:
        case = dict(Q.normal_case(B, N, 31, per=True), logp=TS.logp_normal(B, 33), log_alpha=LOG_ALPHA)
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
        mean = _launch(L, dev, case, 0.0, 1.0, 0, ld=ld, ring=True, entry="mean")
        _check_buffers(mean)


# ------------------------------------------------------------------------------------------------ errors
def test_errors_leave_the_outputs_untouched(L, dev):
    B, N, ld = 8, 8, 32
    case = Q.normal_case(B, N, 51, per=True)
    th, tt = _heads(dev, case["theta"], ld), _heads(dev, case["theta_t"], ld)
    rew, done, w, wmax = (T(case[k]).to(dev) for k in ("rew", "done", "w", "wmax"))
    logp, la = T(TS.logp_normal(B, 53)).to(dev), torch.tensor([LOG_ALPHA], dtype=torch.float32, device=dev)
    dy, scratch, abs_td = (torch.full(s, 5.0, dtype=torch.float32, device=dev) for s in ((2, B, ld), (1024,), (B,)))
    out, slot = torch.full((RING,), 5.0, dtype=torch.float32, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
    ok = dict(theta=L.ptr(th), theta_t=L.ptr(tt), ld=ld, n=N, rew=L.ptr(rew), done=L.ptr(done), g=GAMMA_N, kappa=1.0, b=B, dy=L.ptr(dy),
              out=L.ptr(out), slot=L.ptr(slot), ring=RING, scratch=L.ptr(scratch), w=L.ptr(w), wmax=L.ptr(wmax), abs_td=L.ptr(abs_td),
              logp=L.ptr(logp), log_alpha=L.ptr(la), drop=2)

    def huber(per, **k):
        a = dict(ok, **k)
        head = (a["theta"], a["theta_t"], a["ld"], a["n"], a["rew"], a["done"], a["g"], a["kappa"], a["b"], a["dy"], a["out"], a["slot"],
                a["ring"], a["scratch"])
        with torch.cuda.device(dev):
            if per:
                return L.lib.pqlk_tqc_huber_loss_soft_per(*head, a["w"], a["wmax"], a["abs_td"], a["logp"], a["log_alpha"], a["drop"], L.stream(dev))
            return L.lib.pqlk_tqc_huber_loss_soft(*head, a["logp"], a["log_alpha"], a["drop"], L.stream(dev))

    def mean(**k):
        a = dict(ok, **k)
        with torch.cuda.device(dev):
            return L.lib.pqlk_dpg_loss_quantile_mean(a["theta"], a["ld"], a["n"], a["b"], a["dy"], a["out"], a["slot"], a["ring"], a["scratch"],
                                                     L.stream(dev))

    bad = [(dict(theta=None), E_NULL), (dict(theta_t=None), E_NULL), (dict(rew=None), E_NULL), (dict(done=None), E_NULL), (dict(dy=None), E_NULL),
           (dict(scratch=None), E_NULL), (dict(logp=None), E_NULL), (dict(log_alpha=None), E_NULL), (dict(b=0), E_SHAPE), (dict(ring=0), E_SHAPE),
           (dict(kappa=0.0), E_SHAPE), (dict(kappa=-1.0), E_SHAPE), (dict(ld=48), E_ALIGN), (dict(ld=32, n=33), E_ALIGN),
           (dict(n=1, drop=0), E_UNSUPPORTED), (dict(n=65, ld=96), E_UNSUPPORTED), (dict(drop=-1), E_SHAPE), (dict(drop=N), E_SHAPE),
           (dict(drop=N + 1), E_SHAPE)]
    for k, code in bad:
        assert huber(False, **k) == code and huber(True, **k) == code, k
    for name in ("w", "wmax", "abs_td"):
        assert huber(True, **{name: None}) == E_NULL
    for k, code in [(dict(theta=None), E_NULL), (dict(dy=None), E_NULL), (dict(scratch=None), E_NULL), (dict(b=0), E_SHAPE), (dict(ring=0), E_SHAPE),
                    (dict(ld=48), E_ALIGN), (dict(ld=32, n=33), E_ALIGN), (dict(n=1), E_UNSUPPORTED), (dict(n=65, ld=96), E_UNSUPPORTED)]:
        assert mean(**k) == code, k
    torch.cuda.synchronize(dev)
    for t in (dy, scratch, abs_td, out):
        assert (t == 5.0).all()
