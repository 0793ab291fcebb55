"""A NumPy model of the coloured exploration noise (include/pqlk.h, pqlk_action_noise_colored; pql_amd/utils/noise.py): the table
builders and one step of the law with every rounding applied explicitly -- each operation is one np.float32 operation on np.float32
operands, in the order the header writes them.  Plus the cases and input builders the CPU and GPU tests share.  Not collected as
tests."""
import numpy as np

import detdata as dd

F = np.float32
THREADS, MAX_BLOCKS = 256, 4096   # the launch's block size and grid cap (pql_amd/csrc/noise.hip)
PAST_CAP = THREADS * MAX_BLOCKS + 1
# (rows, cols, R, G, env_offset): one element; odd sizes with two groups; all eight groups from a shifted global index; pink with six
# and with the most octaves over more than one block; one column past the grid cap, where a thread takes a second element
SHAPES = [(1, 1, 1, 1, 0), (5, 3, 1, 2, 0), (37, 16, 1, 8, 3), (64, 21, 6, 1, 0), (300, 16, 8, 1, 0), (PAST_CAP, 1, 1, 3, 5)]
STEPS = 5
LO, HI = F(-1.0), F(1.0)


def linspace32(start, end, steps):
    """torch.linspace's fp32 values: step = (end - start) / (steps - 1); the lower half counts up from start, the upper half down
    from end, every operation in fp32."""
    start, end = F(start), F(end)
    if steps == 1:
        return np.array([start], dtype=F)
    step = F(F(end - start) / F(steps - 1))
    out = np.empty(steps, dtype=F)
    for i in range(steps):
        out[i] = F(start + F(step * F(i))) if i < steps // 2 else F(end - F(step * F(steps - i - 1)))
    return out


def tables(color, *, groups=8, octaves=6, corr_min=0.0, corr_max=0.95):
    """-> rho (G, R) fp32, coef (G, R) fp32, w fp32.  ar1: R = 1, G = groups; pink: R = octaves, G = 1."""
    if color == "ar1":
        rho = linspace32(corr_min, corr_max, groups).reshape(groups, 1)
    else:
        rho = np.array([0.0] + [1.0 - 2.0 ** -k for k in range(1, octaves)], dtype=np.float64)
        assert np.array_equal(rho.astype(F).astype(np.float64), rho)   # dyadic: exact in fp32
        rho = rho.astype(F).reshape(1, octaves)
    r64 = rho.astype(np.float64)
    coef = np.sqrt(1.0 - r64 * r64).astype(F)      # evaluated in float64, rounded once
    w = F(1.0 / np.sqrt(np.float64(rho.shape[1])))
    return rho, coef, w


def step(act, draw, sigma, rho, coef, w, env_offset, fresh, state, lo=LO, hi=HI):
    """One step.  act (N, A), draw (N, R * A), sigma (N,) or a scalar, rho / coef (G, R), fresh (N,) 0 / 1, state (N, R, A), all
    fp32 but fresh.  -> (out (N, A), the new state); nothing is changed in place."""
    N, A = act.shape
    G, R = rho.shape
    assert draw.shape == (N, R * A) and state.shape == (N, R, A) and all(x.dtype == F for x in (act, draw, rho, coef, state))
    g = (np.int64(env_offset) + np.arange(N, dtype=np.int64)) % G
    first = (np.asarray(fresh) != 0)[:, None]
    new = np.empty_like(state)
    n = None
    for k in range(R):
        eps = draw[:, k * A: (k + 1) * A]
        r, c = rho[g, k][:, None], coef[g, k][:, None]
        carried = (r * state[:, k]).astype(F) + (c * eps).astype(F)
        s = np.where(first, eps, carried.astype(F)).astype(F)
        new[:, k] = s
        n = s if k == 0 else (n + s).astype(F)
    n = (n * F(w)).astype(F)
    sig = np.broadcast_to(np.asarray(sigma, dtype=F).reshape(-1, 1), (N, 1))
    noise = (n * sig).astype(F)
    out = np.minimum(np.maximum((act + noise).astype(F), F(lo)), F(hi)).astype(F)
    return out, new


def inputs(rows, cols, R, seed):
    """The sequence of one case: per step act in (-1, 1), a standard-normal draw (rows, R * cols) and the fresh flags -- all ones at
    step 0, then a seeded ~30 % of the rows; and the per-row sigma in [0.05, 0.8]."""
    rng = np.random.default_rng(seed)
    acts = [dd.uniform((rows, cols), seed + 10 + t, -1, 1).astype(F) for t in range(STEPS)]
    draws = [rng.standard_normal((rows, R * cols)).astype(F) for _ in range(STEPS)]
    fresh = [np.ones(rows, dtype=np.uint8)] + [(rng.random(rows) < 0.3).astype(np.uint8) for _ in range(STEPS - 1)]
    sigma = np.linspace(0.05, 0.8, rows).astype(F)
    return acts, draws, fresh, sigma


def run(acts, draws, fresh, sigma, rho, coef, w, env_offset):
    """The model over a sequence, from a zero state -> [(out, state) per step]."""
    N, A = acts[0].shape
    state = np.zeros((N, rho.shape[1], A), dtype=F)
    seq = []
    for a, d, f in zip(acts, draws, fresh):
        out, state = step(a, d, sigma, rho, coef, w, env_offset, f, state)
        seq.append((out, state))
    return seq


def case_tables(R, G):
    """The tables of a kernel case: R = 1 is ar1 with G groups over the default range, R > 1 is pink (G = 1)."""
    return tables("ar1", groups=G) if R == 1 else tables("pink", octaves=R)
