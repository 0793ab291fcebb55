"""Inputs, references and shapes for tests/test_reductions_gpu.py (plain numpy / torch, no GPU).

The shapes come from the kernels' own grid caps and tile sizes (constants below, next to the shapes that
cross them; tests/test_reduction_cases_cpu.py fails and names the shape when a cap moves).  Wherever it
can be done the inputs are small integers or quarter-integers, so an fp32 sum is exact in ANY order and a
dropped or double-counted row fails an equality assert instead of being argued against a tolerance."""
import numpy as np
import torch

import detdata as dd
from support import T  # noqa: F401  (re-exported)

F32 = np.float32

POISON = 5.0          # output slack / pad columns: must come back bit-identical ("untouched") or 0 ("written as zero")
IN_ONE = 1.0          # input slack of the exact-integer designs: an over-read moves the sum by a whole unit
IN_BIG = 1.0e6        # input slack of the others
SLACK = 64            # floats behind every buffer

# ---------------------------------------------------------------- caps (loss.hip, optim.hip) and the shapes that cross them
LOSS_MAX_BLOCKS = 1024
TD_ROWS_PER_BLOCK = 256                                   # k_td_mse<PER>, k_dpg_scalar: one row per thread
C51_ROWS_PER_BLOCK = 4                                    # k_c51_bce<NJ>, k_dpg_dist<NJ>: one row per wave
PROJECT_MAX_BLOCKS, PROJECT_ROWS_PER_BLOCK = 4096, 4      # k_c51_project<NJ>
SUMSQ_TRIP = 1024 * 256 * 4                               # k_sumsq: floats covered by one trip
ADAMW_VEC_TRIP = 2048 * 256 * 4                           # k_adamw, 16-byte path
ADAMW_SCALAR_TRIP = 2048 * 256                            # k_adamw, scalar path
POLYAK_TRIP = 2048 * 256                                  # k_polyak

TD_B = [1, 255, 257, LOSS_MAX_BLOCKS * TD_ROWS_PER_BLOCK + 257]           # second trip of 257 rows: one full block + 1 row
C51_B_BIG = 2 * LOSS_MAX_BLOCKS * C51_ROWS_PER_BLOCK + 5                  # third, ragged trip
PROJECT_B = PROJECT_MAX_BLOCKS * PROJECT_ROWS_PER_BLOCK + 7
ADAM_N_EXACT = 2 * SUMSQ_TRIP + 4 * 300 + 3               # third ragged trip of k_sumsq, second of k_adamw, 3-element tail
ADAM_N_DENSE = 70016 + 3
ADAM_N_MISALIGNED = ADAMW_SCALAR_TRIP + 515
POLYAK_N = [1, 255, POLYAK_TRIP + 257]
PACK_DIMS, PACK_NETS = [40, 64, 32, 1], 2

C51_SHAPES = [(2, 32), (32, 32), (33, 64), (51, 64), (51, 128), (64, 64)]   # (K, ld): K=2; every lane of ld=32; pad-zeroing loop (128)
C51_B = [1, 3, 5, C51_B_BIG]
SAT_GAPS = [8, 60, 120, 60, 120, 8, 120, 60]              # never between 10 and 40: there log(1 - p) hangs on the last bit of p
MOMENTS_N = [2, 3, 63, 64, 65, 129, 4033, 4097]           # 1, 2, 3, 64 chunks; a last chunk of 1 row (4033) and of 2 rows (4097)
MOMENTS_COLS = [1, 31, 33, 88]
BN_M = [2, 5, 63, 64, 65, 257]
BN_COLS = [1, 63, 64, 65, 130]
SG_A = [1, 3, 21, 64]
SG_B = [1, 5, 257]
ALPHA_B = [1, 63, 1023, 1025, 3000]
SHIFT_B = [1, 257, 1000]


def ints(shape, seed, lo, hi):
    """float32 integers in [lo, hi]."""
    return (dd.integers(shape, seed, hi - lo + 1) + lo).astype(F32)


def sums_three_orders(x):
    """fp32 running sums of x taken forward, reversed and in a fixed permutation, and the float64 sum."""
    x = np.asarray(x, dtype=F32).reshape(-1)
    perm = np.random.RandomState(12345).permutation(x.size)
    seq = lambda a: float(np.cumsum(a, dtype=F32)[-1])  # noqa: E731  (cumsum accumulates strictly in order)
    return [seq(x), seq(x[::-1]), seq(x[perm])], float(x.astype(np.float64).sum())


# ---------------------------------------------------------------- A1: TD + twin MSE
def td_inputs(B):
    q, qt = ints((2, B), 811, -1, 1), ints((2, B), 812, -1, 1)
    rew, done = ints((B,), 813, -1, 1), dd.bernoulli((B,), 814, 0.5)
    return q, qt, rew, done, 0.5


def td_reference(q, qt, rew, done, gamma_n, B):
    """The kernel's fp32 expression op by op.  Every intermediate is a multiple of 0.25 of magnitude <= 6.25: exact."""
    y = rew + ((F32(1) - done) * F32(gamma_n)) * np.minimum(qt[0], qt[1])
    d = q - y[None, :]
    terms = (d * d).astype(F32)                       # (2, B), multiples of 0.25
    S = terms.astype(np.float64).sum()
    loss = F32(S) * (F32(1) / F32(B))
    dy = (F32(2) / F32(B)) * d
    return terms, S, loss, dy.astype(F32)


# ---------------------------------------------------------------- A2: DPG, scalar heads
def dpg_scalar_inputs(B):
    q = ints((2, B), 821, -8, 8)
    q[1, ::8] = q[0, ::8]                             # exact ties (hash collisions add a few more)
    return q


def dpg_scalar_reference(q, B):
    a, c = q[0], q[1]
    mins = np.minimum(a, c)
    S = mins.astype(np.float64).sum()
    g = F32(-1) / F32(B)
    loss = F32(S) * g
    h = F32(0.5) * g
    dy = np.stack([np.where(a < c, g, np.where(a == c, h, F32(0))), np.where(c < a, g, np.where(a == c, h, F32(0)))]).astype(F32)
    owner = ((a <= c).astype(np.uint8) | (2 * (c <= a)).astype(np.uint8)).astype(np.uint8)
    return mins, S, loss, dy, owner


# ---------------------------------------------------------------- A3: sixteen ones -> ||g|| = 4 exactly
def adam_exact_positions(n=ADAM_N_EXACT):
    last_quad_end = (n // 4) * 4 - 1
    pos = [0, 3, 4, SUMSQ_TRIP - 1, SUMSQ_TRIP, SUMSQ_TRIP + 3, 2 * SUMSQ_TRIP - 1, 2 * SUMSQ_TRIP, last_quad_end,
           n - 3, n - 2, n - 1,
           300001, 700003, SUMSQ_TRIP + 451426, 2 * SUMSQ_TRIP + 648]
    assert len(set(pos)) == 16 and max(pos) == n - 1 and n % 4 == 3
    return pos


def adam_exact_grad(n=ADAM_N_EXACT):
    g = np.zeros(n, dtype=F32)
    g[adam_exact_positions(n)] = 1.0
    return g


# ---------------------------------------------------------------- A4: Polyak
def polyak_reference(cur, target, tau):
    return (cur * F32(tau) + target * F32(1.0 - float(tau))).astype(F32)   # 1 - tau formed in double, rounded once


# ---------------------------------------------------------------- A5: SAC temperature terms, entropy shift
def alpha_reference(logp, b, target_entropy, prev):
    S = logp.astype(np.float64).sum()
    m = F32(S) / F32(b)
    g = F32(1) * (-m - F32(target_entropy))
    return S, g, F32(prev) + F32(1) * m


# ---------------------------------------------------------------- B1-B3: C51
def c51_inputs(B, K, v_min=-10.0, v_max=10.0, saturated=False):
    """Logits U(-3, 3); rewards spread over 1.4 x the support's half-width around its middle, so that rows clamp at each end;
    one row in five terminal.  saturated=True: the first eight rows of the current logits get one atom above the rest."""
    lg = T(dd.uniform((2, B, K), 91 + K, -3, 3)); lt = T(dd.uniform((2, B, K), 92 + K, -3, 3))
    if B >= C51_B_BIG:
        # Past the grid cap the target logits are 0 on a random half of the atoms and -200 elsewhere: exp(-200) is 0 in fp32, so
        # the pmf is 1 / count on its support in ANY softmax, and kernel and oracle project the same numbers.  With U(-3, 3) logits
        # two fp32 softmaxes (torch's, and a sequential sum) already put 3.6e-7 between two runs of the ORACLE on a bin that
        # collects 0.7 of a row's mass (terminal and clamped rows do), above the 2e-7 bar; over 400,000 bins that tail is met.
        keep = dd.bernoulli((2, B, K), 97 + K, 0.5)
        keep[:, np.arange(B), np.arange(B) % K] = 1.0
        lt = T(np.where(keep > 0, 0.0, -200.0).astype(F32))
    mid, half = 0.5 * (v_max + v_min), 0.5 * (v_max - v_min)
    done = T(dd.bernoulli((B, 1), 94, 0.2))
    # (a terminal row keeps its reward inside the support: clamped, its whole pmf lands in one bin, the sum can round to
    #  1 + 1 ulp, and F.binary_cross_entropy -- the reference -- refuses a target above 1)
    spread = np.where(done.numpy() > 0, 0.9, 1.4) * dd.uniform((B, 1), 93, -1, 1)
    rew = T((mid + half * spread).astype(F32))
    if saturated:
        assert B >= len(SAT_GAPS)
        for i, gap in enumerate(SAT_GAPS):
            for net in range(2):
                lg[net, i] = 0.0
                lg[net, i, (7 * i + 3 * net) % K] = float(gap)
    return lg, lt, rew, done, float(F32(0.99 ** 3))


def c51_reference(ref, lg, lt, rew, done, gn, K, v_min=-10.0, v_max=10.0):
    """torch autograd on the CPU over the oracle's projection, as test_c51_bce_loss does."""
    Fn = torch.nn.functional
    lr = lg.clone().requires_grad_(True)
    with torch.no_grad():
        tgt = torch.min(ref.c51_project_ref(torch.softmax(lt[0], 1), rew, done, gn, v_min, v_max, K),
                        ref.c51_project_ref(torch.softmax(lt[1], 1), rew, done, gn, v_min, v_max, K))
    loss = Fn.binary_cross_entropy(torch.softmax(lr[0], 1), tgt) + Fn.binary_cross_entropy(torch.softmax(lr[1], 1), tgt)
    loss.backward()
    return tgt, loss.detach(), lr.grad


def dpg_dist_inputs(B, K):
    q = T(dd.uniform((2, B, K), 95 + K, -3, 3))
    q[1, ::7] = q[0, ::7]                             # ties -> gradient split evenly (torch.min backward)
    return q


def dpg_dist_reference(q, K):
    z = torch.linspace(-10, 10, K)
    qr = q.clone().requires_grad_(True)
    e = [(torch.softmax(qr[i], 1) * z).sum(1) for i in range(2)]
    loss = -torch.min(e[0], e[1]).mean()
    loss.backward()
    return z, loss.detach(), qr.grad


# ---------------------------------------------------------------- B4: projection
def project_inputs(B=PROJECT_B, K=51, v_min=-10.0, v_max=10.0):
    """Rows i % 4 == 0: terminal, random reward.  Rows i % 4 == 1: terminal with a reward ON an atom, among those for which the kernel's
    own fp32 position (r - v_min) / dz is an integer: lo == up before the fix-up (only a terminal row has that on every lane).
    Others: non-terminal, rewards reaching past both ends of the support."""
    p = torch.softmax(T(dd.uniform((B, K), 71, -3, 3)), 1)
    rew = (0.7 * (v_max - v_min) * dd.uniform((B,), 72, -1, 1)).astype(F32)
    done = np.zeros(B, dtype=F32)
    dz = F32((float(v_max) - float(v_min)) / (K - 1))
    on_atom = []
    for j in range(K):
        r = F32(v_min) + F32(j) * dz
        for _ in range(8):                            # walk to a neighbour whose fp32 position is exactly j
            b = (r - F32(v_min)) / dz
            if b == F32(j):
                break
            r = np.nextafter(r, F32(np.inf) if b < j else F32(-np.inf), dtype=F32)
        if (r - F32(v_min)) / dz == F32(j):           # (near v_min the fp32 grid of r is too coarse for some atoms)
            on_atom.append(r)
    on_atom = np.array(on_atom, dtype=F32)
    assert len(on_atom) >= K // 4 and on_atom[0] == F32(v_min) and on_atom[-1] == F32(v_max)
    i = np.arange(B)
    done[i % 4 == 0] = 1.0
    grid = i % 4 == 1
    done[grid] = 1.0
    rew[grid] = on_atom[(i[grid] // 4) % len(on_atom)]
    return p, T(rew).view(-1, 1), T(done).view(-1, 1), float(F32(0.99 ** 3)), grid


# ---------------------------------------------------------------- B5: batch moments
def moments_inputs(n, cols, ldx):
    x = np.full((n, ldx), IN_BIG, dtype=F32)
    x[:, :cols] = dd.uniform((n, cols), 55 + n + cols, -3, 5)
    return x


def moments_reference(x, cols):
    x64 = x[:, :cols].astype(np.float64)
    return x64.mean(0), x64.var(0, ddof=1)


def moments_extra_inputs(n=4097, rand_cols=33):
    """rand_cols columns U(-3, 5), then a constant column 3.0 (every chunk sum exact), then 1000 + 0.01 U(-1, 1)."""
    cols = rand_cols + 2
    x = moments_inputs(n, cols, cols + 5)
    x[:, rand_cols] = 3.0
    x[:, rand_cols + 1] = (1000.0 + 0.01 * dd.uniform((n,), 57, -1, 1).astype(np.float64)).astype(F32)
    return x, cols


# ---------------------------------------------------------------- B6: BatchNorm + ELU
def bn_inputs(m, cols, ld, beta_shift=0.0):
    """z U(-2, 2) plus a column offset; rows 0 and 1 are pushed to -(1 + |u|) and +(1 + |u|) so that no column of a 2- or 5-row
    batch has a tiny variance: there w = gamma / sqrt(var + eps) reaches the hundreds, z * w and b cancel, and no fp32
    evaluation -- torch's own included -- meets the 5e-6 bar.  A 2-row batch is scaled by 0.003 as a whole: its xhat is +-x0 with
    1 - x0^2 = eps / (var + eps), and dz = (g0 - g1) / 2 * (1 - x0^2) * w is what is left of a cancellation down to 1e-5 unless the
    variance is of eps's order (torch's fp32 autograd misses the gradient bar 500-fold on O(1) rows).  mean / var are float64
    statistics of z rounded once to fp32."""
    z = np.full((m, ld), IN_BIG, dtype=F32)
    zz = dd.uniform((m, cols), 31 + m + cols, -2, 2)
    zz[0] = -(1 + np.abs(zz[0])); zz[1] = 1 + np.abs(zz[1])
    zz = ((zz + 0.5 * dd.uniform((1, cols), 32 + cols, -1, 1)) * (0.003 if m == 2 else 1.0)).astype(F32)
    z[:, :cols] = zz
    gamma = dd.uniform((cols,), 33 + cols, 0.5, 1.5); beta = (dd.uniform((cols,), 34 + cols, -0.5, 0.5) + F32(beta_shift)).astype(F32)
    z64 = zz.astype(np.float64)
    mean, var = z64.mean(0).astype(F32), z64.var(0, ddof=1).astype(F32)
    rm0, rv0 = dd.uniform((cols,), 35 + cols, -1, 1), dd.uniform((cols,), 36 + cols, 0.5, 2.0)
    return z, zz, gamma, beta, mean, var, rm0, rv0


def bn_reference(zz, gamma, beta, dy=None, running=None, eps=1e-5, momentum=0.1):
    """float64 F.elu(F.batch_norm(...)) and, with dy, its autograd.  running=(rm, rv): eval mode on those statistics."""
    Fn = torch.nn.functional
    z = T(zz.astype(np.float64)).requires_grad_(dy is not None)
    g = T(gamma.astype(np.float64)).requires_grad_(dy is not None); b = T(beta.astype(np.float64)).requires_grad_(dy is not None)
    if running is not None:
        rm, rv = (T(a.astype(np.float64)) for a in running)
        return Fn.elu(Fn.batch_norm(z, rm, rv, g, b, training=False, eps=eps)).numpy()
    y = Fn.elu(Fn.batch_norm(z, None, None, g, b, training=True, eps=eps))
    if dy is None:
        return y.numpy()
    (y * T(dy.astype(np.float64))).sum().backward()
    return y.detach().numpy(), z.grad.numpy(), g.grad.numpy(), b.grad.numpy()


# ---------------------------------------------------------------- B7: squashed-Gaussian head
def sg_inputs(B, A, ld_y):
    """Raw log_std U(-6.5, 6.5) (outside the +-5 clamp on about a quarter of the entries); mu = std * U(-3, 3) and eps with mu's
    sign, so that u = mu + eps * std neither cancels (act is asked to rtol 1e-6 with no atol) nor dwarfs std (then the fp32
    u - mu of the header's formula loses eps).  With std up to e^5 that puts |u| in the hundreds: tanh saturates."""
    ls = dd.uniform((B, A), 41 + A + B, -6.5, 6.5)
    sd = np.exp(np.clip(ls.astype(np.float64), -5, 5))
    mp = dd.uniform((B, A), 42 + A + B, -3, 3)
    mu = (sd * mp).astype(F32)
    eps = (np.sign(mp) * dd.uniform((B, A), 43 + A + B, 0.05, 2.0)).astype(F32)
    y = np.full((B, ld_y), IN_BIG, dtype=F32)
    y[:, :A] = mu; y[:, A:2 * A] = ls
    return y, mu, ls, eps


def sg_reference(mu, ls, eps, da=None, glp=0.0):
    """float64 of the formula in include/pqlk.h; with da also autograd of sum(da * a) + glp * sum(logp)."""
    m = T(mu.astype(np.float64)).requires_grad_(da is not None); l = T(ls.astype(np.float64)).requires_grad_(da is not None)
    e = T(eps.astype(np.float64))
    sd = torch.exp(torch.clamp(l, -5, 5))
    u = m + e * sd
    a = torch.tanh(u)
    logp = (-((u - m) ** 2) / (2 * sd ** 2) - torch.log(sd) - 0.5 * np.log(2 * np.pi)
            - 2 * (np.log(2.0) - u - torch.nn.functional.softplus(-2 * u))).sum(1)
    if da is None:
        return a.numpy(), logp.numpy(), u.numpy()
    ((a * T(da.astype(np.float64))).sum() + glp * logp.sum()).backward()
    return a.detach().numpy(), m.grad.numpy(), l.grad.numpy()
