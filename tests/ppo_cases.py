"""Inputs, references and shapes for tests/test_ppo_kernels_gpu.py (plain numpy / torch, no GPU).

The shapes come from the constants of pql_amd/csrc/ppo.hip and rollout.hip, mirrored below next to the shapes that cross
them (tests/test_ppo_cases_cpu.py fails and names the shape when one moves).  The exact designs use +-1 / 0 advantages,
logstd = 0 and quarter-integers: every cross-row sum is exact in fp32 in ANY order, every per-row quantity is restated op by
op in fp32 numpy (the library is built with -ffp-contract=off), and a dropped or doubled row fails an equality assert."""
import functools

import numpy as np
import torch

import detdata as dd
from reduction_cases import F32, IN_BIG, IN_ONE, POISON, SLACK, T, ints, sums_three_orders  # noqa: F401  (re-exported)

F64 = np.float64

# ---------------------------------------------------------------- kernel constants (ppo.hip, rollout.hip)
PPO_HEAD_BLOCKS = 256                                     # fixed grid cap of k_ppo_policy_head / k_ppo_value_head
PPO_GATHER_ROWS = 64                                      # minibatch rows (= one advantage partial) per k_ppo_gather block
GAE_UNROLL = (8, 16, 32)                                  # k_ppo_gae<TM>: T <= TM takes the unrolled kernel, T > 32 the loop
ELEMENTWISE_MAX_BLOCKS, ELEMENTWISE_THREADS = 4096, 256   # k_rms_normalize, k_action_noise
LOG_SQRT_2PI = F32(0.91893853320467274)                   # PPO_LOG_SQRT_2PI
ENT_CONST = F32(1.4189385332046727)                       # PPO_ENT_CONST


def group_of(A):
    """Lanes per row of the Gaussian / policy heads: the power of two >= A."""
    G = 1
    while G < A:
        G <<= 1
    return G


def groups_per_block(A):
    return 256 // group_of(A)


def rows_per_grid(A):
    """Rows one trip of the capped policy-head grid covers."""
    return PPO_HEAD_BLOCKS * groups_per_block(A)


# ---------------------------------------------------------------- shapes
HEAD_A = [1, 3, 21, 33, 64]                               # G = 1, 4, 32, 64 (partly filled) and 64 (full)
HEAD_B = [1, 5, 257]
POLICY_SMALL_B = {1: 37, 3: 37, 21: 5, 33: 3, 64: 3}      # fewer rows than one block has groups
POLICY_CROSS_B = {1: 65793, 3: 16449, 21: 4109, 33: 2055, 64: 2055, 16: 8229}   # odd, past the cap, ragged (CPU test)
POLICY_CROSS = [(A, POLICY_CROSS_B[A]) for A in HEAD_A + [16]]                   # A = 16: the workload's own
POLICY_CASES = sorted([(A, b) for A in HEAD_A for b in (1, POLICY_SMALL_B[A])] + POLICY_CROSS)
VALUE_B = [1, 255, 257, PPO_HEAD_BLOCKS * 256 + 257]      # second trip of 257 rows: one full block + 1 row
GATHER_MB = [1, 63, 64, 65, 64 * PPO_GATHER_ROWS + 37]    # 65 partials: a second trip of ppo_adv_stats, a ragged tail
GATHER_OA = [(1, 1), (13, 3), (88, 21), (8, 64)]
GAE_T = [1, 8, 9, 16, 17, 32, 33]
GAE_N = [1, 255, 257]
ELEMENTWISE_COLS = 13
ELEMENTWISE_ROWS = -(-(ELEMENTWISE_MAX_BLOCKS * ELEMENTWISE_THREADS + 257) // ELEMENTWISE_COLS)   # first row count past cap + 257
ELEMENTWISE_LD_OUT = 16


def seq_sum(x):
    """fp32 sum over the last axis in index order, starting from 0.f."""
    x = np.asarray(x, dtype=F32)
    s = np.zeros(x.shape[:-1], dtype=F32)
    for k in range(x.shape[-1]):
        s = (s + x[..., k]).astype(F32)
    return s


# ---------------------------------------------------------------- advantages: +-1 and one 0
def adv_design(n, fixed=None):
    """n advantages in {+1, -1, 0}.  Rows [0, r0), r0 = the start of the ragged last PPO_GATHER_ROWS-block, hold as many +1
    as -1; so does the ragged block, whose odd row (when it has one: the LAST row) is 0.  Every block sum is an integer, every
    full block's mean a multiple of 1/64, the ragged block's mean 0: all of the gather's partials and the minibatch statistics
    are exact in any order.  For odd n: mean 0, sum of squared deviations n - 1, unbiased std 1 and std + 1e-8f == 1.
    fixed = {row: +-1} prescribes rows (not the last row of an odd n); the others are dealt by a hash."""
    fixed = dict(fixed or {})
    a = np.zeros(n, dtype=F32)
    r0 = ((n - 1) // PPO_GATHER_ROWS) * PPO_GATHER_ROWS if n % PPO_GATHER_ROWS else n
    hi_ragged = n - 1 if (n - r0) % 2 else n
    assert all(0 <= r < n and s in (1, -1) and (r < hi_ragged or r < r0) for r, s in fixed.items()), fixed
    for lo, hi, seed in ((0, r0, 7001), (r0, hi_ragged, 7002)):
        free = np.array([r for r in range(lo, hi) if r not in fixed], dtype=np.int64)
        npos = (hi - lo) // 2 - sum(1 for r, s in fixed.items() if lo <= r < hi and s > 0)
        nneg = (hi - lo) // 2 - sum(1 for r, s in fixed.items() if lo <= r < hi and s < 0)
        assert npos >= 0 and nneg >= 0 and npos + nneg == len(free), (n, lo, hi, npos, nneg)
        if len(free):
            order = np.argsort(dd.uniform((len(free),), seed + n), kind="stable")
            a[free[order]] = np.r_[np.ones(npos, dtype=F32), -np.ones(nneg, dtype=F32)]
    for r, s in fixed.items():
        a[r] = s
    return a


def adv_partials(a):
    """k_ppo_gather's partials { rows, sum, sum((x - block mean)^2) } per PPO_GATHER_ROWS rows, op by op in fp32; the two sums
    through float64 (exact on adv_design's data, which the CPU test proves in three fp32 orders)."""
    a = np.asarray(a, dtype=F32)
    n = a.size
    out = np.zeros((-(-n // PPO_GATHER_ROWS), 3), dtype=F32)
    for i in range(out.shape[0]):
        blk = a[i * PPO_GATHER_ROWS:(i + 1) * PPO_GATHER_ROWS]
        s = F32(blk.astype(F64).sum())
        m = s / F32(blk.size)
        dv = (blk - m).astype(F32)
        out[i] = (F32(blk.size), s, F32((dv * dv).astype(F32).astype(F64).sum()))
    return out


def adv_stats_model(part, n, order=None):
    """ppo_adv_stats op by op in fp32, the partials taken in `order`: (mean, std, std + 1e-8f)."""
    part = np.asarray(part, dtype=F32)
    order = np.arange(part.shape[0]) if order is None else order
    s = F32(0)
    for i in order:
        s = F32(s + part[i, 1])
    m = s / F32(n)
    q = F32(0)
    with np.errstate(invalid="ignore", divide="ignore"):
        for i in order:
            c = part[i, 0]
            d = F32(part[i, 1] / c) - m
            q = F32(q + F32(part[i, 2] + F32(c * F32(d * d))))
        std = np.sqrt(F32(q / F32(n - 1)))
    return m, std, F32(std + F32(1e-8))


# ---------------------------------------------------------------- policy head, exact
def policy_markers(A, b):
    """Rows whose d = act - mean is 0 in one column (everywhere else it is +-1): the first and the last row, both sides of every
    trip boundary of the capped grid, and in the last trip the last row of the last full block and the first row of the partial
    block behind it.  Marker i sits in column i % A and, unless it is the last row (adv 0), carries adv +1 / -1 in turn: at most
    two markers of each sign per column (CPU test), so the dlogstd partial sums stay in {0, +-g, +-2g}, exact in any order."""
    g, rpg = groups_per_block(A), rows_per_grid(A)
    rows = {0, b - 1}
    k = rpg
    while k < b:
        rows |= {k - 1, k}
        k += rpg
    start = ((b - 1) // rpg) * rpg
    full = (b - start) // g
    if full and start + full * g < b:
        rows |= {start + full * g - 1, start + full * g}
    rows = sorted(rows)
    cols = [i % A for i in range(len(rows))]
    signs = [0 if r == b - 1 else (1 if i % 2 == 0 else -1) for i, r in enumerate(rows)]
    return rows, cols, signs


@functools.lru_cache(maxsize=None)
def policy_exact_inputs(A, b):
    """mean = quarter-integers, act = mean + d with d = +-1 (0 on the markers), logstd = 0, adv_design advantages and their
    partials.  Nobody writes to what this returns."""
    rows, cols, signs = policy_markers(A, b)
    adv = adv_design(b, {r: s for r, s in zip(rows, signs) if s})
    mu = (ints((b, A), 7100 + A, -4, 4) * F32(0.25)).astype(F32)
    d = np.where(dd.bernoulli((b, A), 7101 + A, 0.5) > 0, F32(1), F32(-1)).astype(F32)
    d[rows, cols] = 0.0
    act = (mu + d).astype(F32)
    assert np.array_equal((act - mu).astype(F32), d)
    return dict(mu=mu, act=act, d=d, adv=adv, part=adv_partials(adv), logstd=np.zeros(A, dtype=F32), markers=(rows, cols, signs))


def row_logp(d, var=F32(1), ls=F32(0)):
    """Normal.log_prob per element as the kernels write it, summed over the action axis in index order."""
    d = np.asarray(d, dtype=F32)
    lp = ((-(d * d) / (F32(2) * var)) - ls) - LOG_SQRT_2PI
    return seq_sum(lp.astype(F32))


def entropy_sum(A, ls=F32(0)):
    h = F32(0)
    for _ in range(A):
        h = F32(h + F32(ENT_CONST + ls))
    return h


def policy_exact_reference(A, b, lam):
    """k_ppo_policy_head / k_ppo_policy_fold op by op in fp32 on policy_exact_inputs: ratio = expf(0) = 1 (old_logp = the
    kernel's own logp), na = (adv - 0) / 1 = adv, every row on the max tie and inside the closed clamp interval."""
    c = policy_exact_inputs(A, b)
    d, adv = c["d"], c["adv"]
    one, g = F32(1), F32(1) / F32(b)
    na = ((adv - F32(0)) / one).astype(F32)
    l1 = (-na * one).astype(F32)
    w = F32(g * F32(0.5))
    dratio = (w * -na + w * -na).astype(F32)
    dlp = (dratio * one).astype(F32)
    dy = (dlp[:, None] * (d / one)).astype(F32)
    ls_terms = (dlp[:, None] * ((d * d) / one - one)).astype(F32)
    loss_terms = np.maximum(l1, l1)
    loss = F32(F32(loss_terms.astype(F64).sum()) / F32(b)) - F32(F32(lam) * entropy_sum(A))
    dlogstd = (ls_terms.astype(F64).sum(0).astype(F32) - F32(lam)).astype(F32)
    return dict(logp=row_logp(d), dy=dy, ls_terms=ls_terms, loss_terms=loss_terms, loss=F32(loss), dlogstd=dlogstd, g=g)


# ---------------------------------------------------------------- policy head, dense
@functools.lru_cache(maxsize=None)
def policy_dense_inputs(A, b):
    """test_policy_head_matches_autograd's data at (A, b): trajectory U-ranges, logstd U(-1, 0.3), and the shifts that put the
    ratio inside the clip (+-0.05), on both clipped sides (+-0.5, +-1) and exactly at 1 (0: also both bounds of clip = 0)."""
    shift = np.array([0.0, 0.05, -0.05, 0.5, -0.5, 0.0, 1.0, -1.0], dtype=F32)[np.arange(b) % 8]
    return dict(y=dd.uniform((b, A), 320, -1, 1), act=dd.uniform((b, A), 301 + A, -2, 2), adv=dd.uniform((b,), 303 + A, -2, 3),
                logstd=dd.uniform((A,), 321, -1.0, 0.3), shift=shift)


def policy_dense_reference(y, logstd, act, old_logp, adv, clip, lam, logp_kernel):
    """test_ppo_gpu._policy_ref in float64 on the CPU: ppo.py:156-175 with autograd, the kernel's log-probs taken into the graph
    (lp and logp_kernel differ by ~1e-6, so lp + (logp_kernel - lp) is logp_kernel to the bit and ratio = 1 where old == logp)."""
    from torch.distributions import Independent, Normal
    t64 = lambda a: T(np.asarray(a, dtype=F64))  # noqa: E731
    mean, ls = t64(y).requires_grad_(True), t64(logstd).requires_grad_(True)
    old, a = t64(old_logp), t64(adv)
    dist = Independent(Normal(loc=mean, scale=torch.exp(ls.expand_as(mean))), 1)
    lp = dist.log_prob(t64(act))
    lp = lp + (t64(logp_kernel) - lp).detach()
    ratio = (lp - old).exp()
    na = (a - a.mean()) / (a.std() + 1e-8)
    loss = torch.max(-na * ratio, -na * torch.clamp(ratio, 1 - clip, 1 + clip)).mean() - lam * dist.entropy().mean()
    loss.backward()
    return loss.item(), mean.grad.numpy(), ls.grad.numpy(), ratio.detach().numpy()


# ---------------------------------------------------------------- value head
VALUE_CLIP = 0.25


@functools.lru_cache(maxsize=None)
def value_exact_inputs(b):
    """Quarter-integers: R in [-2, 2], v - R in [-2, 2], v - V in {0, +-0.25, +-0.5}: against clip = 0.25 inside, ON both clamp
    bounds and outside.  Inside and on the bounds V + clamp(v - V) == v, so lu == lc (the max tie)."""
    R = (ints((b,), 7201, -8, 8) * F32(0.25)).astype(F32)
    v = (R + ints((b,), 7202, -8, 8) * F32(0.25)).astype(F32)
    V = (v - (ints((b,), 7203, -2, 2) * F32(0.25))).astype(F32)
    return v, R, V


def value_reference(v, R, V, b, clip_on, clip=VALUE_CLIP):
    """k_ppo_value_head / k_ppo_value_fold op by op in fp32: (loss terms, their float64 sum, loss, dy column 0)."""
    g = F32(F32(0.5) * (F32(1) / F32(b)))
    du = (v - R).astype(F32)
    lu = (du * du).astype(F32)
    if clip_on:
        c = F32(clip)
        ddv = (v - V).astype(F32)
        cd = np.minimum(np.maximum(ddv, -c), c).astype(F32)
        dc = ((V + cd).astype(F32) - R).astype(F32)
        lc = (dc * dc).astype(F32)
        h = F32(g * F32(0.5))
        w1 = np.where(lu > lc, g, np.where(lu == lc, h, F32(0))).astype(F32)
        w2 = np.where(lc > lu, g, np.where(lu == lc, h, F32(0))).astype(F32)
        inside = (ddv >= -c) & (ddv <= c)
        dv = ((w1 * (F32(2) * du)).astype(F32) + np.where(inside, (w2 * (F32(2) * dc)).astype(F32), F32(0))).astype(F32)
        terms = np.maximum(lu, lc)
    else:
        dv = (g * (F32(2) * du)).astype(F32)
        terms = lu
    S = float(terms.astype(F64).sum())
    return terms, S, F32(F32(0.5) * (F32(S) / F32(b))), dv


def value_autograd(v, R, V, clip_on, clip):
    """The value loss of ppo.py:161-172 in float64 torch with autograd: (loss, d loss / d v)."""
    vv = T(np.asarray(v, dtype=F64)).requires_grad_(True)
    R, V = T(np.asarray(R, dtype=F64)), T(np.asarray(V, dtype=F64))
    if clip_on:
        loss = 0.5 * torch.max((vv - R) ** 2, (V + torch.clamp(vv - V, -clip, clip) - R) ** 2).mean()
    else:
        loss = 0.5 * ((vv - R) ** 2).mean()
    loss.backward()
    return loss.item(), vv.grad.numpy()


VALUE_DENSE_CLIP = 0.2
VALUE_DENSE_SHIFTS = [0.0, 0.1, -0.1, 0.5, -0.5, 0.15, -0.15, 1.0]
VALUE_DENSE_MIN_GAP = 0.05


@functools.lru_cache(maxsize=None)
def value_dense_inputs(b):
    """test_value_head_matches_autograd's data with two changes that make FLOAT64 a valid reference for an fp32 kernel:
    * |v - R| >= 0.05 (or exactly 0 on the R = V = v rows).  Where v - V is inside the clip, float64 sees V + (v - V) == v and
      the max tie; fp32 may round V + fl(v - V) one ulp off v and pick a side.  Either way the gradient is 2 g du or 2 g dc with
      |dc - du| <= 2.4e-7, which is inside rtol 2e-5 only while |du| is not tiny.
    * the shifts +-0.2 == clip became +-0.15: fl(v - fl(v - 0.2f)) lands on either side of 0.2f by rounding alone, and the
      closed-interval rule then differs between the two precisions.  The bounds themselves are tested on exact data."""
    v = dd.uniform((b,), 400, -2, 2)
    gap = dd.uniform((b,), 401, VALUE_DENSE_MIN_GAP + 0.01, 2.0) * np.where(dd.bernoulli((b,), 402, 0.5) > 0, F32(1), F32(-1))
    R = (v - gap).astype(F32)
    V = (v - np.array(VALUE_DENSE_SHIFTS, dtype=F32)[np.arange(b) % 8]).astype(F32)
    R[::16] = V[::16]                                     # rows with shift 0: v == V == R
    return v, R, V


# ---------------------------------------------------------------- gather
@functools.lru_cache(maxsize=None)
def gather_inputs(mb, O, A):
    """A trajectory of rows = mb + 9 and mb indices whose gathered advantages are adv_design(mb): distinct rows of [1, rows - 2],
    then idx[0] = -5 (must read row 0), idx[mb - 1] = rows + 3 (must read row rows - 1) and one duplicate.  Trajectory rows
    that no index names hold advantage 3.0: a wrong row moves a partial.  A ragged block of ONE row gets -1 instead of the
    design's 0: its mean is the row itself and its squared deviation 0, exactly, but only when divided by its own row count."""
    rows = mb + 9
    want = adv_design(mb)
    if mb % PPO_GATHER_ROWS == 1:
        want[-1] = -1.0
    base = 1 + np.argsort(dd.uniform((rows - 2,), 7300 + mb), kind="stable")[:mb].astype(np.int64)
    idx = base.copy()
    adv = np.full(rows, 3.0, dtype=F32)
    adv[base] = want
    if mb >= 4:
        twin = next(r for r in range(2, mb - 1) if want[r] == want[1])
        idx[twin] = idx[1]
    idx[0] = -5
    adv[0] = want[0]
    if mb >= 2:
        idx[mb - 1] = rows + 3
        adv[rows - 1] = want[mb - 1]
    traj = dict(obs=dd.uniform((rows, O), 7310 + mb, -3, 3), act=dd.uniform((rows, A), 7311 + mb, -2, 2),
                logp=dd.uniform((rows,), 7312 + mb, -5, -1), adv=adv, ret=dd.uniform((rows,), 7314 + mb, -2, 2),
                val=dd.uniform((rows,), 7315 + mb, -2, 2))
    return dict(rows=rows, idx=idx, k=np.clip(idx, 0, rows - 1), want_adv=want, traj=traj,
                mean=dd.uniform((O,), 7320 + O, -0.5, 0.5), var=dd.uniform((O,), 7321 + O, 0.5, 2.0), eps=F32(1e-4))


def normalize_reference(x, mean, var, eps):
    """(x - mean) / sqrt(var + eps) in fp32, the sqrt through numpy (correctly rounded, as the device's)."""
    return ((x - mean).astype(F32) / np.sqrt((var + F32(eps)).astype(F32))).astype(F32)


# ---------------------------------------------------------------- Gaussian head
@functools.lru_cache(maxsize=None)
def head_inputs(A, B):
    return dict(mu=dd.uniform((B, A), 7400 + A + B, -2, 2), eps=dd.uniform((B, A), 7401 + A + B, -2, 2),
                logstd=dd.uniform((A,), 7402 + A, -1.0, 0.3))


def head_exact_reference(mu, eps):
    """k_ppo_gauss_head at logstd = 0 op by op: act = mu + eps * 1, d = act - mu (NOT eps: one rounding), logp, ent."""
    act = (mu + (eps * F32(1)).astype(F32)).astype(F32)
    return act, row_logp((act - mu).astype(F32)), entropy_sum(mu.shape[1])


def head_dense_reference(mu, logstd, act):
    """float64 of the formula in include/pqlk.h at the actions the kernel returned."""
    mu, ls, a = (np.asarray(x, dtype=F64) for x in (mu, logstd, act))
    lp = -((a - mu) ** 2) / (2 * np.exp(ls) ** 2) - ls - np.log(np.sqrt(2 * np.pi))
    return lp.sum(1), float((0.5 + 0.5 * np.log(2 * np.pi) + ls).sum())


# ---------------------------------------------------------------- GAE
@functools.lru_cache(maxsize=None)
def gae_inputs(Tn, n):
    """test_gae_bit_exact_against_the_reference_loop's data; with n > 1 column 0 is done at every step (and after the last),
    column 1 never."""
    c = dict(rew=dd.uniform((Tn, n), 11, -2, 2), done=dd.bernoulli((Tn, n), 12, 0.15), val=dd.uniform((Tn, n), 13, -3, 3),
             nv=dd.uniform((n,), 14, -3, 3), nd=dd.bernoulli((n,), 15, 0.2), tmo=dd.bernoulli((Tn, n), 16, 0.1))
    if n > 1:
        c["done"][:, 0], c["nd"][0] = 1.0, 1.0
        c["done"][:, 1], c["nd"][1] = 0.0, 0.0
    return c


def gae_reference(rew, done, val, nv, nd, gamma, lam, gae, tmo):
    """`_gae_torch` below (ppo.py:88-124) restated in fp32 numpy, op for op; tmo = None: no time-outs."""
    Tn = rew.shape[0]
    g, gl, one = F32(gamma), F32(gamma * lam), F32(1)     # gamma * lambda in double, then one fp32 rounding, as torch's scalar
    adv, ret = np.zeros_like(rew), np.zeros_like(rew)
    last = np.zeros(rew.shape[1], dtype=F32)
    for t in reversed(range(Tn)):
        tail = t == Tn - 1
        nnt = (one - (nd if tail else done[t + 1])).astype(F32)
        if gae:
            nxv = nv if tail else val[t + 1]
            nnt2 = ((nnt != 0) != (tmo[t] != 0)).astype(F32) if tmo is not None else nnt
            delta = ((rew[t] + ((g * nxv).astype(F32) * nnt2).astype(F32)).astype(F32) - val[t]).astype(F32)
            last = (delta + ((gl * nnt).astype(F32) * last).astype(F32)).astype(F32)
            adv[t] = last
        else:
            nr = nv if tail else ret[t + 1]
            ret[t] = (rew[t] + ((g * nnt).astype(F32) * nr).astype(F32)).astype(F32)
    if gae:
        return adv, (adv + val).astype(F32)
    return (ret - val).astype(F32), ret


# ---------------------------------------------------------------- rollout elementwise kernels
@functools.lru_cache(maxsize=None)
def elementwise_inputs():
    rows, cols = ELEMENTWISE_ROWS, ELEMENTWISE_COLS
    return dict(x=dd.uniform((rows, cols), 7500, -4, 4), mean=dd.uniform((cols,), 7501, -1, 1), var=dd.uniform((cols,), 7502, 0.1, 3.0),
                act=dd.uniform((rows, cols), 7503, -1, 1), draw=dd.uniform((rows, cols), 7504, -3, 3),
                std_rows=np.linspace(0.05, 0.8, rows).astype(F32))


def noise_reference(act, draw, sigma, lo, hi):
    return np.minimum(np.maximum((act + (draw * sigma).astype(F32)).astype(F32), F32(lo)), F32(hi)).astype(F32)


def _gae_torch(rew, dones, values, next_value, next_done, gamma, lam, gae, timeout):
    """ppo.py:88-124, op for op (one torch launch per op: no contraction)."""
    Tn = rew.shape[0]
    next_value = next_value.reshape(1, -1)
    if gae:
        adv = torch.zeros_like(rew)
        last = 0
        for t in reversed(range(Tn)):
            if t == Tn - 1:
                nnt, nv = 1.0 - next_done, next_value
            else:
                nnt, nv = 1.0 - dones[t + 1], values[t + 1]
            nnt2 = torch.logical_xor(nnt, timeout[t]) if timeout is not None else nnt
            delta = rew[t] + gamma * nv * nnt2 - values[t]
            last = delta + gamma * lam * nnt * last
            adv[t] = last
        return adv, adv + values
    ret = torch.zeros_like(rew)
    for t in reversed(range(Tn)):
        if t == Tn - 1:
            nnt, nr = 1.0 - next_done, next_value
        else:
            nnt, nr = 1.0 - dones[t + 1], ret[t + 1]
        ret[t] = rew[t] + gamma * nnt * nr
    return ret - values, ret
