"""The laws of the critic diagnostics (include/pqlk.h, "Critic diagnostics") as NumPy models written from the prose, the exact-data
designs the kernel tests run on, a generic categorical design, and the error bound that one is held to.  Nothing here runs on a GPU;
tests/test_diag_cases_cpu.py proves the models and the designs.

`critic_stats_model(case, F32)` follows the law op by op in fp32 wherever an op rounds; its sums over the rows are taken in float64
and rounded once, which is what ANY fp32 summation order gives on the exact designs (every partial sum is representable there:
`exact_*_case` asserts it) and nothing else is claimed for it.  `critic_stats_model(case, np.float64)` is the float64 reference.
`unit_stats_model` follows pqlk_unit_stats' documented order where it can matter (the sum over the columns), so its outputs, the
dormant decision included, are the kernel's bits on any matrix whose column sums are exact.

U = 2^-24 is the unit roundoff of fp32 round-to-nearest.
"""
import numpy as np

from hlgauss_cases import E_EXP
from quantile_cases import SLOP, U, f32, survives_fp32  # noqa: F401  (re-exported)

F32 = np.float32
N_STATS = 10
SCALAR, CATEGORICAL, QUANTILE = 0, 1, 2
LOSS_MAX_BLOCKS = 1024
UNIT_CHUNKS = 64
NAMES = ("q1_mean", "q2_mean", "q_min", "q_max", "target_mean", "td_bias", "td_abs_mean", "td_abs_max", "twin_gap", "nonfinite")
GAMMA = 0.5


def blocks_of(b, k):
    return min(-(-b // (256 if k <= 1 else 4)), LOSS_MAX_BLOCKS)


# ------------------------------------------------------------------------------------------------ pqlk_critic_stats
def row_values(x, head, z, dt):
    """x (2, B, k) -> V (2, B) in dtype dt."""
    x = np.asarray(x, dt)
    if head == SCALAR:
        return x[:, :, 0]
    if head == QUANTILE:
        k = x.shape[-1]
        s = x.astype(np.float64).sum(axis=-1).astype(dt)      # (exact on the designs)
        return s * (dt(1.0) / dt(k)) if dt is F32 else s / k
    m = x.max(axis=-1, keepdims=True)
    e = np.exp(x - m)
    p = e / e.sum(axis=-1, keepdims=True)
    return (p * np.asarray(z, dt)).sum(axis=-1)


def critic_stats_model(case, dt=F32):
    """-> (out (10,) in dtype dt, rows: dict of the per-row quantities)."""
    head, b = case["head"], case["b"]
    with np.errstate(all="ignore"):
        v = row_values(case["q"], head, case.get("z"), dt)
        vt = row_values(case["qt"], head, case.get("z"), dt)
        r, d, g = np.asarray(case["rew"], dt), np.asarray(case["done"], dt), dt(F32(case["gamma_n"]))
        y_raw = r + ((dt(1.0) - d) * g) * np.fmin(vt[0], vt[1])
        y = y_raw
        if head == CATEGORICAL:
            y = np.where(np.isnan(y_raw), y_raw, np.fmin(np.fmax(y_raw, dt(F32(case["v_min"]))), dt(F32(case["v_max"]))))
        td = np.fmax(np.abs(v[0] - y), np.abs(v[1] - y))
        bias = (v[0] + v[1]) * dt(0.5) - y
        gap = np.abs(v[0] - v[1])
        bad = ~(np.isfinite(v[0]) & np.isfinite(v[1]) & np.isfinite(y_raw))
        rows = dict(v=v, vt=vt, y=y, td=td, bias=bias, gap=gap, bad=bad)

        def mean(t):
            s = t.astype(np.float64).sum()
            return F32(s) * (F32(1.0) / F32(b)) if dt is F32 else s / b

        def fold(fn, t, start):
            return dt(fn.reduce(np.concatenate(([dt(start)], t.reshape(-1)))))

        out = np.array([mean(v[0]), mean(v[1]), fold(np.fmin, np.fmin(v[0], v[1]), np.inf), fold(np.fmax, np.fmax(v[0], v[1]), -np.inf),
                        mean(y), mean(bias), mean(td), fold(np.fmax, td, -np.inf), mean(gap), dt(bad.sum())], dt)
    return out, rows


def _dyadic(rng, shape, lo=-2.0, hi=2.0, step=0.25):
    n = int(round((hi - lo) / step))
    return (lo + step * rng.integers(0, n + 1, shape)).astype(F32)


def _assert_exact_sums(rows, b, resolution):
    """Every partial sum of the summed statistics, in any order, is a multiple of `resolution` below 2^24 of them: exact in fp32."""
    for name in ("y", "td", "bias", "gap"):
        t = rows[name].astype(np.float64)
        assert ((t / resolution) == np.round(t / resolution)).all(), name
        assert np.abs(t).sum() / resolution < 2.0 ** 24, name
    for t in rows["v"].astype(np.float64):
        assert ((t / resolution) == np.round(t / resolution)).all() and np.abs(t).sum() / resolution < 2.0 ** 24


SCALAR_B = [1, 255, 256, 257, LOSS_MAX_BLOCKS * 256 + 1]
QUANTILE_K, QUANTILE_B = [2, 32, 64], [1, 3, 4, 5, LOSS_MAX_BLOCKS * 4 + 1]


def exact_scalar_case(b, seed=0):
    """Dyadic zero-centred values, |v| <= 2, step 1/4; gamma_n = 1/2; done in {0, 1}: y and every statistic's terms are multiples
    of 1/8."""
    rng = np.random.default_rng(1000 + seed + b)
    case = dict(head=SCALAR, k=1, b=b, q=_dyadic(rng, (2, b, 1)), qt=_dyadic(rng, (2, b, 1)), rew=_dyadic(rng, (b,)),
                done=rng.integers(0, 2, b).astype(F32), gamma_n=GAMMA)
    _assert_exact_sums(critic_stats_model(case, np.float64)[1], b, 1.0 / 8)
    return case


def exact_quantile_case(b, k, seed=0):
    """The same with k quantile locations per row: k is a power of two, so the row mean (sum * fl(1 / k)) is exact, a multiple of
    1 / (4 k); y a multiple of 1 / (8 k)."""
    assert k & (k - 1) == 0
    rng = np.random.default_rng(2000 + seed + 7 * b + k)
    case = dict(head=QUANTILE, k=k, b=b, q=_dyadic(rng, (2, b, k)), qt=_dyadic(rng, (2, b, k)), rew=_dyadic(rng, (b,)),
                done=rng.integers(0, 2, b).astype(F32), gamma_n=GAMMA)
    _assert_exact_sums(critic_stats_model(case, np.float64)[1], b, 1.0 / (8 * k))
    return case


CATEGORICAL_K, CATEGORICAL_B, V_MIN, V_MAX, GAMMA_N = [2, 51, 64, 65, 256], 263, -10.0, 10.0, 0.99 ** 3


def categorical_case(b, k, seed=0):
    """Gaussian logits (standard deviation 2) on the support linspace(-10, 10, k); rewards that send every fifth row's y past v_min
    and every fifth past v_max (the clamp); a quarter of the rows terminal."""
    rng = np.random.default_rng(3000 + seed + k)
    z = np.linspace(V_MIN, V_MAX, k).astype(F32)
    rew = rng.uniform(-1.0, 1.0, b)
    rew[np.arange(b) % 5 == 3] -= 14.0
    rew[np.arange(b) % 5 == 4] += 14.0
    return dict(head=CATEGORICAL, k=k, b=b, q=(2.0 * rng.standard_normal((2, b, k))).astype(F32),
                qt=(2.0 * rng.standard_normal((2, b, k))).astype(F32), z=z, v_min=V_MIN, v_max=V_MAX, rew=rew.astype(F32),
                done=(rng.random(b) < 0.25).astype(F32), gamma_n=GAMMA_N)


def categorical_bounds(case):
    """-> (float64 reference out (10,), absolute bound (10,)) for a categorical case, a first-order forward bound in the manner of
    hlgauss_cases.hl_bounds; chain = ceil(k / 64) + 5 adds in a row reduction.

    dV.  expf(x_k - m): rho_e = U max_k |x_k - m| + 2 E_EXP U; s, a positive sum chain deep: rho_s = rho_e + chain U; p_k = e_k / s:
      rho_p = rho_e + rho_s + U; V = sum_k fl(p_k z_k) along the chain: |dV| <= (rho_p + (chain + 1) U) sum_k p_k |z_k|.
    dy.  y = fl(r + fl(fl((1 - d) gamma_n) fmin(V'))): mult max_i dV'_i + U (3 |mult min V'| + |r|); the clamp is 1-Lipschitz, exact.
    rows.  td = max_i |fl(V_i - y)|: max_i (dV_i + dy + U |V_i - y|); bias = fl(fl(fl(V_0 + V_1) 0.5) - y): (dV_0 + dV_1) / 2 + dy +
      U (|V_0 + V_1| / 2 + |bias|); gap: dV_0 + dV_1 + U gap.
    means.  The mean of the rows' bounds, plus the summation: on the longest path ceil(b / (4 blocks)) adds in the wave's row loop, 2
      across the block's waves, ceil(blocks / 256) + 6 + 2 in the fold, then the rounding of 1 / B and the product: (adds + 2) U times
      the mean of the terms' magnitudes.  min / max: fmin and fmax are 1-Lipschitz and exact: the largest row bound.  The count is exact."""
    out, rows = critic_stats_model(case, np.float64)
    b, k = case["b"], case["k"]
    chain = -(-k // 64) + 5
    absz = np.abs(case["z"].astype(np.float64))

    def d_value(x):
        x = x.astype(np.float64)
        m = x.max(axis=-1, keepdims=True)
        e = np.exp(x - m)
        p = e / e.sum(axis=-1, keepdims=True)
        rho_e = U * np.abs(x - m).max(axis=-1) + 2.0 * E_EXP * U
        rho_p = rho_e + (rho_e + chain * U) + U
        return (rho_p + (chain + 1) * U) * (p * absz).sum(axis=-1)          # (2, B)

    dv, dvt = d_value(case["q"]), d_value(case["qt"])
    v, y = rows["v"], rows["y"]
    mult = (1.0 - case["done"].astype(np.float64)) * f32(case["gamma_n"])
    dy = mult * dvt.max(axis=0) + U * (3.0 * np.abs(mult * np.minimum(rows["vt"][0], rows["vt"][1])) + np.abs(case["rew"].astype(np.float64)))
    d_td = (dv + dy[None] + U * np.abs(v - y[None])).max(axis=0)
    d_bias = 0.5 * (dv[0] + dv[1]) + dy + U * (0.5 * np.abs(v[0] + v[1]) + np.abs(rows["bias"]))
    d_gap = dv[0] + dv[1] + U * rows["gap"]
    blocks = blocks_of(b, k)
    adds = -(-b // (4 * blocks)) + 2 + -(-blocks // 256) + 8

    def mean(d_rows, t):
        return d_rows.mean() + (adds + 2) * U * np.abs(t).mean()

    bound = np.array([mean(dv[0], v[0]), mean(dv[1], v[1]), dv.max(), dv.max(), mean(dy, y), mean(d_bias, rows["bias"]),
                      mean(d_td, rows["td"]), d_td.max(), mean(d_gap, rows["gap"]), 0.0])
    return out, SLOP * bound


# ------------------------------------------------------------------------------------------------ pqlk_unit_stats
def block_sum_256(per_thread):
    """per_thread (256,) fp32 -> the kernels' block sum: per wave the xor butterfly (offsets 32 ... 1), then (w0 + w1) + (w2 + w3)."""
    v = np.asarray(per_thread, F32).reshape(4, 64).copy()
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = (v + v[:, lane ^ o]).astype(F32)
    w = v[:, 0]
    return F32(F32(w[0] + w[1]) + F32(w[2] + w[3]))


def thread_chains(per_col):
    """per_col (cols,) fp32 -> (256,): thread t adds columns t, t + 256, ... in increasing order, from 0.f."""
    acc = np.zeros(256, F32)
    cols = len(per_col)
    for c0 in range(0, cols, 256):
        part = np.zeros(256, F32)
        part[: min(256, cols - c0)] = per_col[c0: c0 + 256]
        acc = (acc + part).astype(F32)
    return acc


def unit_stats_model(h, cols, tau):
    """h (rows, >= cols) fp32 -> (out (3,) fp32, a (cols,) fp32, dormant (cols,) bool).  The column sums over the rows are taken in
    float64 and rounded once (exact on the designs, whatever the order)."""
    x = np.asarray(h, F32)[:, :cols]
    rows = x.shape[0]
    s_abs = np.abs(x).astype(np.float64).sum(axis=0)
    slope = np.where(x > 0, F32(1.0), x + F32(1.0)).astype(F32)
    s_slope = slope.astype(np.float64).sum(axis=0)
    assert survives_fp32(s_abs) and survives_fp32(s_slope), "the design's column sums must be exact in fp32"
    a = (s_abs.astype(F32) / F32(rows)).astype(F32)
    A = F32(block_sum_256(thread_chains(a)) / F32(cols))
    S = block_sum_256(thread_chains(s_slope.astype(F32)))
    thr = F32(F32(tau) * A)
    dormant = a <= thr
    out = np.array([F32(F32(dormant.sum()) / F32(cols)), A, F32(S / F32(F32(rows) * F32(cols)))], F32)
    return out, a, dormant


def unit_stats_ref64(h, cols, tau):
    x = np.asarray(h, np.float64)[:, :cols]
    a = np.abs(x).mean(axis=0)
    A = a.mean()
    return np.array([(a <= f32(tau) * A).mean(), A, np.where(x > 0, 1.0, x + 1.0).mean()])


# (rows, cols, ld): one row; cols 1, 63, 64, 65, 512, 513, 1025; ld > cols; rows one past the chunk cap (and well past it)
UNIT_SHAPES = [(1, 1, 32), (1, 65, 96), (7, 63, 64), (64, 64, 64), (UNIT_CHUNKS + 1, 65, 128), (5, 512, 512), (9, 513, 544),
               (3, 1025, 1056), (4 * UNIT_CHUNKS + 3, 130, 160)]
PAD_POISON = 1.0e6


def unit_case(rows, cols, ld, seed=0, tau=0.25):
    """Post-ELU-like dyadic values in (-1, 2], step 1/4 (negative ones -3/4 ... -1/4, as an ELU's output lies above -1), poisoned pad
    columns; column 0 all zeros (always dormant) and the last column all -1 exactly (slope 0; |h| = 1).  A unit exactly on the threshold
    is `threshold_case`'s."""
    rng = np.random.default_rng(4000 + seed + rows + 3 * cols)
    h = np.full((rows, ld), PAD_POISON, F32)
    h[:, :cols] = (-0.75 + 0.25 * rng.integers(0, 12, (rows, cols))).astype(F32)
    h[:, 0] = 0.0
    if cols > 1:
        h[:, cols - 1] = -1.0
    return dict(h=h, rows=rows, cols=cols, ld=ld, tau=tau)


def threshold_case():
    """4 rows x 4 columns with a = (1, 1, 1.5, 0.5): A = 1, tau = 0.5 -> tau * A = 0.5 = a_3 exactly: unit 3 is dormant by `<=`,
    the others are not."""
    h = np.full((4, 32), PAD_POISON, F32)
    h[:, 0], h[:, 1], h[:, 2], h[:, 3] = 1.0, -1.0, 1.5, 0.5
    return dict(h=h, rows=4, cols=4, ld=32, tau=0.5)
