"""pqlk_critic_stats and pqlk_unit_stats on the GPU against tests/diag_cases.py: the exact-data designs bit for bit at one row, at a
ragged block, at several blocks and one row past the grid cap; the categorical head within the derived bound of float64; the bit
ties with the |TD| of the weighted loss entries; non-finite rows; the unit statistics at their column and chunk edges with poisoned
pad columns; reproducibility; refused calls that write nothing.

Every buffer a kernel writes has SLACK floats of poison behind it, which must come back intact; every input has IN_BIG in its
slack and its pad columns, which would move the result."""
import numpy as np
import pytest
import torch

import diag_cases as dc
import reduction_cases as rc
from guarded import Guarded
from support import T, bits, dev  # noqa: F401

pytestmark = pytest.mark.gpu

POISON = rc.POISON
F32 = np.float32


def _same(a, b):
    return np.array_equal(bits(np.asarray(a, F32)), bits(np.asarray(b, F32)))


def _ld(k):
    from pql_amd import _lib as L
    return int(L.lib.pqlk_ld(k))


def _critic(dev, case, ld=None, keep=None):
    """One call on guarded buffers -> out (10,) on the host.  keep: a dict that receives the device tensors (for the bit ties)."""
    from pql_amd import _lib as L
    b, k, head = case["b"], case["k"], case["head"]
    ld = ld or _ld(k)

    def padded(x):
        g = Guarded(dev, (2, b, ld), rc.IN_BIG)
        g.t[:, :, :k] = T(x).to(dev)
        return g

    def vec(x):
        return Guarded(dev, x.shape, rc.IN_BIG, x)

    q, qt, rew, done = padded(case["q"]), padded(case["qt"]), vec(case["rew"]), vec(case["done"])
    z = vec(case["z"]) if head == dc.CATEGORICAL else None
    n = int(L.lib.pqlk_critic_stats_scratch_floats(b, k))
    assert n == dc.N_STATS * dc.blocks_of(b, k)
    out, scr = Guarded(dev, (dc.N_STATS,), POISON), Guarded(dev, (n,), POISON)
    L.check(L.lib.pqlk_critic_stats(q.ptr, qt.ptr, ld, head, k, z.ptr if z else None, float(case.get("v_min", 0.0)), float(case.get("v_max", 0.0)),
                                    rew.ptr, done.ptr, float(case["gamma_n"]), b, out.ptr, scr.ptr, L.stream(dev)))
    torch.cuda.synchronize()
    assert out.intact() and scr.intact(), "a guard word behind out / scratch was overwritten"
    if keep is not None:
        keep.update(q=q, qt=qt, rew=rew, done=done, z=z, ld=ld)
    return out.host().copy()


# =========================================================================== the exact designs: bits
@pytest.mark.parametrize("b", dc.SCALAR_B)
def test_scalar_head_exact_design_bitwise(dev, b):
    case = dc.exact_scalar_case(b)
    want, _ = dc.critic_stats_model(case, F32)
    for ld in (32, 96) if b < 1000 else (32,):          # (a wider row stride changes nothing)
        got = _critic(dev, case, ld)
        assert _same(got, want), (b, ld, dict(zip(dc.NAMES, zip(got, want))))
    assert want[9] == 0 and want[2] <= want[0] <= want[3]


@pytest.mark.parametrize("k", dc.QUANTILE_K)
@pytest.mark.parametrize("b", dc.QUANTILE_B)
def test_quantile_head_exact_design_bitwise(dev, b, k):
    case = dc.exact_quantile_case(b, k)
    want, _ = dc.critic_stats_model(case, F32)
    for ld in (_ld(k), _ld(k) + 32):
        got = _critic(dev, case, ld)
        assert _same(got, want), (b, k, ld, dict(zip(dc.NAMES, zip(got, want))))


# =========================================================================== the categorical head: the derived bound
@pytest.mark.parametrize("k", dc.CATEGORICAL_K)
def test_categorical_head_within_the_bound(dev, k):
    """Every output within diag_cases.categorical_bounds of the float64 reference; the observed error is printed beside the bound."""
    case = dc.categorical_case(dc.CATEGORICAL_B, k)
    ref, bound = dc.categorical_bounds(case)
    got = _critic(dev, case).astype(np.float64)
    err = np.abs(got - ref)
    print(f"critic_stats categorical K={k}: " + "  ".join(f"{n} {e:.2e}/{bd:.2e}" for n, e, bd in zip(dc.NAMES, err, bound)))
    assert np.isfinite(got).all() and got[9] == 0
    assert (err <= bound).all(), dict(zip(dc.NAMES, zip(err, bound)))
    assert dc.V_MIN <= got[4] <= dc.V_MAX and got[2] <= min(got[0], got[1]) and max(got[0], got[1]) <= got[3]


# =========================================================================== bit ties with the loss entries' |TD|
def test_scalar_td_max_is_the_weighted_mse_entrys(dev):
    from pql_amd import _lib as L
    b = 1000
    rng = np.random.default_rng(77)
    case = dict(head=dc.SCALAR, k=1, b=b, q=rng.standard_normal((2, b, 1)).astype(F32), qt=rng.standard_normal((2, b, 1)).astype(F32),
                rew=rng.uniform(-1, 1, b).astype(F32), done=(rng.random(b) < 0.2).astype(F32), gamma_n=0.99 ** 3)
    keep = {}
    got = _critic(dev, case, 32, keep)
    f = lambda *s, v=0.0: torch.full(s, v, device=dev)   # noqa: E731
    dy, td, scr, w, wmax = f(2, b, 32), f(b), f(2048), f(b, v=1.0), f(1, v=1.0)
    L.check(L.lib.pqlk_td_mse_loss_per(keep["q"].ptr, keep["qt"].ptr, 32, keep["rew"].ptr, keep["done"].ptr, float(case["gamma_n"]), b, L.ptr(dy),
                                       None, None, 0, L.ptr(scr), L.ptr(w), L.ptr(wmax), L.ptr(td), L.stream(dev)))
    torch.cuda.synchronize()
    assert _same(got[7], td.max().cpu().numpy())
    # (the mean of the same |TD|: at most 1 + 8 + 1 + 8 adds and two roundings of the scale on the longest path of 1000 positive terms)
    assert abs(float(got[6]) - float(td.double().mean())) <= 20 * dc.U * float(td.double().mean())


@pytest.mark.parametrize("k", [51, 256])
def test_categorical_td_max_is_the_weighted_hlgauss_entrys(dev, k):
    from pql_amd import _lib as L
    case = dc.categorical_case(dc.CATEGORICAL_B, k)
    b, keep = case["b"], {}
    got = _critic(dev, case, None, keep)
    ld = keep["ld"]
    f = lambda *s, v=0.0: torch.full(s, v, device=dev)   # noqa: E731
    dy, td, scr, w, wmax = f(2, b, ld), f(b), f(2048), f(b, v=1.0), f(1, v=1.0)
    L.check(L.lib.pqlk_hlgauss_ce_loss_per(keep["q"].ptr, keep["qt"].ptr, ld, k, keep["rew"].ptr, keep["done"].ptr, keep["z"].ptr,
                                           float(case["gamma_n"]), float(case["v_min"]), float(case["v_max"]), 0.75, b, L.ptr(dy), None, None, 0,
                                           None, L.ptr(scr), L.ptr(w), L.ptr(wmax), L.ptr(td), L.stream(dev)))
    torch.cuda.synchronize()
    assert _same(got[7], td.max().cpu().numpy())


# =========================================================================== non-finite rows
def test_non_finite_rows_are_counted_and_propagate(dev):
    case = dc.exact_scalar_case(300)
    case = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in case.items()}
    case["q"][0, 3, 0], case["qt"][:, 7, 0], case["rew"][270] = np.nan, np.inf, np.nan
    case["done"][7] = 0.0
    want, _ = dc.critic_stats_model(case, F32)
    got = _critic(dev, case, 32)
    assert got[9] == 3 == want[9]
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.isnan(got[[0, 4, 5, 6, 8]]).all()
    assert np.isfinite(got[1]) and got[7] == np.inf
    ok = ~np.isnan(want)
    assert _same(got[ok], want[ok])


def test_repeat_calls_give_identical_bits(dev):
    for case in (dc.exact_scalar_case(70000), dc.categorical_case(5000, 101, seed=1), dc.exact_quantile_case(4097, 32)):
        assert _same(_critic(dev, case), _critic(dev, case))


# =========================================================================== unit statistics
def _unit(dev, case):
    from pql_amd import _lib as L
    rows, cols, ld = case["rows"], case["cols"], case["ld"]
    h = Guarded(dev, (rows, ld), dc.PAD_POISON, case["h"])
    n = int(L.lib.pqlk_unit_stats_scratch_floats(cols))
    out, scr = Guarded(dev, (3,), POISON), Guarded(dev, (n,), POISON)
    L.check(L.lib.pqlk_unit_stats(h.ptr, ld, rows, cols, float(case["tau"]), out.ptr, scr.ptr, L.stream(dev)))
    torch.cuda.synchronize()
    assert out.intact() and scr.intact()
    assert np.array_equal(h.host(), case["h"])          # read-only
    return out.host().copy()


@pytest.mark.parametrize("rows,cols,ld", dc.UNIT_SHAPES)
def test_unit_stats_exact_design_bitwise(dev, rows, cols, ld):
    """The dormant fraction (so the count), A and the mean slope are the model's bits; at tau = 0 exactly the all-zero columns count."""
    for tau in (0.25, 0.0, 0.9):
        case = dict(dc.unit_case(rows, cols, ld), tau=tau)
        want, a, dormant = dc.unit_stats_model(case["h"], cols, tau)
        got = _unit(dev, case)
        assert _same(got, want), (rows, cols, ld, tau, got, want)
        assert round(float(got[0]) * cols) == int(dormant.sum())
    assert _same(_unit(dev, case), got)                 # a second call: the same bits


def test_unit_on_the_threshold_is_dormant(dev):
    case = dc.threshold_case()
    got = _unit(dev, case)
    assert got.tolist() == [0.25, 1.0, 0.75]
    assert _unit(dev, dict(case, tau=0.49))[0] == 0.0


# =========================================================================== refused calls write nothing
def test_refused_calls_write_nothing(dev):
    from pql_amd import _lib as L
    f = lambda n: torch.full((n,), POISON, device=dev)   # noqa: E731
    q, qt, rew, done, z, out, scr, h = f(2 * 4 * 64), f(2 * 4 * 64), f(4), f(4), f(8), f(10), f(4096), f(4 * 64)
    st = L.stream(dev)

    def critic(head=0, k=1, ld=32, b=4, v_min=-1.0, v_max=1.0, q_=q, out_=out):
        return L.lib.pqlk_critic_stats(L.ptr(q_), L.ptr(qt), ld, head, k, L.ptr(z), v_min, v_max, L.ptr(rew), L.ptr(done), 0.5, b, L.ptr(out_),
                                       L.ptr(scr), st)

    def unit(ld=64, rows=4, cols=8, tau=0.1, h_=h):
        return L.lib.pqlk_unit_stats(L.ptr(h_), ld, rows, cols, tau, L.ptr(out), L.ptr(scr), st)

    assert critic(q_=None) == L.E_NULL and critic(out_=None) == L.E_NULL and critic(head=5) == L.E_UNSUPPORTED
    assert critic(b=0) == L.E_SHAPE and critic(head=1, k=1) == L.E_SHAPE and critic(head=1, k=8, v_min=1.0, v_max=1.0) == L.E_SHAPE
    assert critic(head=2, k=65, ld=96) == L.E_UNSUPPORTED and critic(head=1, k=51, ld=32) == L.E_ALIGN and critic(ld=40) == L.E_ALIGN
    assert unit(h_=None) == L.E_NULL and unit(rows=0) == L.E_SHAPE and unit(cols=0) == L.E_SHAPE and unit(ld=7) == L.E_SHAPE
    assert unit(tau=1.0) == L.E_SHAPE and unit(tau=-0.1) == L.E_SHAPE and unit(tau=float("nan")) == L.E_SHAPE
    torch.cuda.synchronize()
    assert bool((out == POISON).all()) and bool((scr == POISON).all())
    assert critic() == L.OK and unit() == L.OK          # the same buffers, accepted: now they are written
    torch.cuda.synchronize()
    assert not bool((out[:3] == POISON).all())
