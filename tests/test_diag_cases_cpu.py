"""tests/diag_cases.py proved on the CPU: the NumPy models of pqlk_critic_stats and pqlk_unit_stats against float64 on random data,
and on the exact-data designs the GPU kernel tests run on (where they must be exact, not close)."""
import numpy as np
import pytest

import diag_cases as dc

F32 = np.float32


def _random_case(head, k, b, seed):
    rng = np.random.default_rng(seed)
    case = dict(head=head, k=k, b=b, q=rng.standard_normal((2, b, k)).astype(F32), qt=rng.standard_normal((2, b, k)).astype(F32),
                rew=rng.uniform(-1, 1, b).astype(F32), done=(rng.random(b) < 0.3).astype(F32), gamma_n=0.97)
    if head == dc.CATEGORICAL:
        case.update(z=np.linspace(-3.0, 3.0, k).astype(F32), v_min=-3.0, v_max=3.0)
    return case


@pytest.mark.parametrize("head,k", [(dc.SCALAR, 1), (dc.QUANTILE, 32), (dc.QUANTILE, 7), (dc.CATEGORICAL, 51)])
def test_critic_model_fp32_agrees_with_float64_on_random_data(head, k):
    case = _random_case(head, k, 300, 11 + k)
    got, _ = dc.critic_stats_model(case, F32)
    ref, rows = dc.critic_stats_model(case, np.float64)
    assert got.dtype == F32 and ref.dtype == np.float64
    # a loose sanity band (the fp32 model's own rounding: a few ulp of values of order 1 to 10), not the kernels' bound
    np.testing.assert_allclose(got, ref, rtol=0, atol=2e-5)
    assert ref[9] == 0 and ref[2] <= min(ref[0], ref[1]) and max(ref[0], ref[1]) <= ref[3]
    assert ref[7] >= ref[6] >= abs(ref[5]) - 1e-12 and ref[8] >= 0
    if head == dc.CATEGORICAL:
        assert (rows["y"] >= -3.0).all() and (rows["y"] <= 3.0).all()


def test_critic_model_against_a_hand_computed_batch():
    """Two rows, scalar head, gamma_n = 1/2.  Row 0: V = (1, 3), V' = (2, 4), r = 1, d = 0 -> y = 2; row 1: V = (-1, -2), V' = (8, 6),
    r = -1, d = 1 -> y = -1."""
    case = dict(head=dc.SCALAR, k=1, b=2, q=np.array([[[1.0], [-1.0]], [[3.0], [-2.0]]], F32), qt=np.array([[[2.0], [8.0]], [[4.0], [6.0]]], F32),
                rew=np.array([1.0, -1.0], F32), done=np.array([0.0, 1.0], F32), gamma_n=0.5)
    for dt in (F32, np.float64):
        out, rows = dc.critic_stats_model(case, dt)
        assert rows["y"].tolist() == [2.0, -1.0]
        #                      q1   q2   min   max  y    bias                 td             tdmax gap  bad
        assert out.tolist() == [0.0, 0.5, -2.0, 3.0, 0.5, ((2 - 2) + (-1.5 + 1)) / 2, (1 + 1) / 2, 1.0, (2 + 1) / 2, 0.0]


def test_critic_model_non_finite_rows():
    """A NaN in q, +inf in qt and a NaN reward: three rows are counted; the sums carry the NaN (or the infinity), the min and the max
    drop a NaN and keep an infinity."""
    case = dc.exact_scalar_case(40)
    case = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in case.items()}
    case["q"][0, 3, 0], case["qt"][:, 7, 0], case["rew"][11] = np.nan, np.inf, np.nan
    case["done"][7] = 0.0
    out, _ = dc.critic_stats_model(case, F32)
    assert out[9] == 3
    assert np.isnan(out[0]) and np.isfinite(out[1])             # V_1 carries the NaN, V_2 does not
    assert np.isnan(out[4]) and np.isnan(out[5]) and np.isnan(out[6])
    assert np.isfinite(out[2]) and np.isfinite(out[3]) and out[7] == np.inf      # |V - inf| = inf is kept by the max
    assert np.isnan(out[8])


@pytest.mark.parametrize("b", dc.SCALAR_B)
def test_exact_scalar_design(b):
    case = dc.exact_scalar_case(b)            # (asserts that every partial sum is exact)
    got, ref = dc.critic_stats_model(case, F32)[0], dc.critic_stats_model(case, np.float64)[0]
    # the sums are exact: the fp32 model differs from float64 by the one rounded product sum * fl(1 / b) alone
    for j in (0, 1, 4, 5, 6, 8):
        assert got[j] == F32(F32(ref[j] * b) * (F32(1.0) / F32(b)))
    for j in (2, 3, 7, 9):
        assert got[j] == ref[j]
    assert dc.blocks_of(b, 1) == min(-(-b // 256), 1024)


@pytest.mark.parametrize("k", dc.QUANTILE_K)
@pytest.mark.parametrize("b", dc.QUANTILE_B)
def test_exact_quantile_design(b, k):
    case = dc.exact_quantile_case(b, k)
    got, ref = dc.critic_stats_model(case, F32)[0], dc.critic_stats_model(case, np.float64)[0]
    for j in (0, 1, 4, 5, 6, 8):
        assert got[j] == F32(F32(ref[j] * b) * (F32(1.0) / F32(b)))
    for j in (2, 3, 7, 9):
        assert got[j] == ref[j]


@pytest.mark.parametrize("k", dc.CATEGORICAL_K)
def test_categorical_bound_is_small_and_covers_the_fp32_model(k):
    """The a-priori bound is of the order of fp32 rounding on values of order 10 -- far below anything a wrong law would produce --
    and the op-by-op fp32 NumPy model lies inside it (NumPy's expf is within the E_EXP ulp the bound allows the device's)."""
    case = dc.categorical_case(dc.CATEGORICAL_B, k)
    ref, bound = dc.categorical_bounds(case)
    got, rows = dc.critic_stats_model(case, F32)
    assert bound[9] == 0 and (bound[:9] > 0).all() and bound.max() < 1e-4
    assert (np.abs(got.astype(np.float64) - ref) <= bound).all(), (got - ref, bound)
    y = rows["y"]
    assert (y == F32(dc.V_MIN)).any() and (y == F32(dc.V_MAX)).any()          # the clamp is exercised at both ends


# ------------------------------------------------------------------------------------------------ unit statistics
def test_block_sum_model_is_a_sum():
    rng = np.random.default_rng(5)
    v = rng.integers(-8, 9, 256).astype(F32)
    assert dc.block_sum_256(v) == v.sum()
    cols = rng.integers(-8, 9, 700).astype(F32)
    assert dc.block_sum_256(dc.thread_chains(cols)) == cols.sum()


@pytest.mark.parametrize("rows,cols,ld", dc.UNIT_SHAPES)
def test_unit_model_on_the_exact_design(rows, cols, ld):
    case = dc.unit_case(rows, cols, ld)
    out, a, dormant = dc.unit_stats_model(case["h"], cols, case["tau"])
    ref = dc.unit_stats_ref64(case["h"], cols, case["tau"])
    assert out.dtype == F32
    np.testing.assert_allclose(out[1:], ref[1:], rtol=1e-5)       # a_c and A round (division by rows, cols); the slope sum is exact
    assert a[0] == 0 and dormant[0]                                # the column of zeros is dormant at any tau
    if cols > 1:
        assert a[cols - 1] == 1 and not dormant[cols - 1]          # the column at -1: |h| = 1, slope 0
    assert out[0] == F32(F32(dormant.sum()) / F32(cols))
    # tau = 0: exactly the all-zero columns
    out0, a0, dormant0 = dc.unit_stats_model(case["h"], cols, 0.0)
    assert (dormant0 == (a0 == 0)).all() and dormant0[0]


def test_unit_model_random_data_against_float64():
    rng = np.random.default_rng(6)
    h = (0.25 * rng.integers(-3, 9, (33, 96))).astype(F32)
    out, _, _ = dc.unit_stats_model(h, 70, 0.1)
    np.testing.assert_allclose(out, dc.unit_stats_ref64(h, 70, 0.1), rtol=1e-5)


def test_unit_on_the_threshold_is_dormant():
    case = dc.threshold_case()
    out, a, dormant = dc.unit_stats_model(case["h"], case["cols"], case["tau"])
    assert a.tolist() == [1.0, 1.0, 1.5, 0.5] and out[1] == 1.0
    assert dormant.tolist() == [False, False, False, True] and out[0] == 0.25
    assert out[2] == F32((4 * 1 + 4 * 0 + 4 * 1 + 4 * 1) / 16.0)
