"""The laws of the TQC agent (include/pqlk.h, "TQC as the paper defines it") as float64 references written from the prose: the soft
truncated target's loss, gradient and |TD|, the mean-of-critics actor objective, literal torch formulations for autograd, the inputs
and error bounds the kernel tests use, and a CPU autograd agent for the agent tests.  Nothing here runs on a GPU;
tests/test_tqc_sac_cpu.py checks the references against torch.autograd.  Conventions (U, SLOP, f32, taus, the fold) are those of
tests/quantile_cases.py; the ranks, the kept sets, the dictionary a law is returned in and the shape of the bounds are those of
tests/tqc_cases.py, so `tqc_cases.tqc_ref` and `tqc_cases.tqc_bounds` read a `soft_base` as they read a `tqc_base`.
"""
import numpy as np
import torch

import quantile_cases as Q
import tqc_cases as TQ

U, SLOP = Q.U, Q.SLOP
EXPF_ULPS = 1.0   # the allowance tests/test_reductions_gpu.py documents for k_sac_alpha_terms: "a 1-ulp expf"; one ulp is at most 2 u relative


def alpha_of(log_alpha):
    """alpha = exp(log_alpha) of the fp32 value the device holds, in float64."""
    return float(np.exp(np.float64(np.float32(log_alpha))))


def pool_ranks(theta_t):
    """rank(p) = #{q : z_q < z_p} + #{q < p : z_q = z_p} on the raw pooled target atoms z_p, p = i N + k.  theta_t (2, B, N) ->
    (z (B, 2 N), rank (B, 2 N)).  The same counting as tqc_cases.tqc_base (tests/test_tqc_sac_cpu.py holds the two together)."""
    tt = np.asarray(theta_t, np.float64)
    z = np.concatenate([tt[0], tt[1]], axis=1)
    idx = np.arange(z.shape[1])
    rank = np.zeros(z.shape, np.int64)
    for q in range(z.shape[1]):
        zq = z[:, q: q + 1]
        rank += (zq < z) | ((zq == z) & (q < idx)[None, :])
    return z, rank


# ------------------------------------------------------------------------------------------------ the soft law, float64
def soft_base(theta, theta_t, rew, done, logp, log_alpha, gamma_n, kappa, drops, terms=False, chunk=256):
    """tqc_cases.tqc_base for the soft target: s_b = alpha logp_b, ranks and kept sets on the RAW z_p, T_p = r + c (z_p - s_b).
    Returns tqc_base's dictionary (so tqc_cases.tqc_ref makes the loss, dy and |TD| of it) with `dT` enlarged by what the shift adds
    (see soft_bounds) and the shift `s` itself."""
    th, tt = np.asarray(theta, np.float64), np.asarray(theta_t, np.float64)
    r, d, lp = np.asarray(rew, np.float64), np.asarray(done, np.float64), np.asarray(logp, np.float64)
    g, kap = Q.f32(gamma_n), Q.f32(kappa)
    _, B, N = th.shape
    drops = [int(x) for x in drops]
    assert all(0 <= x <= N - 1 for x in drops) and lp.shape == (B,)
    z, rank = pool_ranks(tt)
    keep = np.stack([rank < 2 * (N - x) for x in drops], axis=2)                 # the kept sets: (B, 2 N, d)
    s = alpha_of(log_alpha) * lp                                                  # s_b
    m = (1.0 - d) * g                                                            # c of the prose
    zs = z - s[:, None]
    T = r[:, None] + m[:, None] * zs                                             # T_p
    # |dT_p|: tqc_bounds' three roundings of r + fl(fl((1 - d) gamma_n) x) with x = z_p - s_b, plus c times the error of x itself:
    # fl(alpha_dev logp) with alpha_dev = alpha (1 + e), |e| <= 2 u EXPF_ULPS, errs by (2 EXPF_ULPS + 1) u |s_b|; the subtraction
    # adds one rounding of its result
    dx = (2.0 * EXPF_ULPS + 1.0) * U * np.abs(s)[:, None] + U * np.abs(zs)
    dT = U * (3.0 * np.abs(m[:, None] * zs) + np.abs(r)[:, None]) + np.abs(m)[:, None] * dx
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x))  # noqa: E731
    th_t, T_t, dT_t, keep_t, tau = t(th), t(T), t(dT), t(keep.astype(np.float64)), t(Q.taus(N))[None, None, :, None]
    out = {k: torch.zeros((2, B, N, len(drops)), dtype=torch.float64) for k in ("G", "absG", "E", "RHO", "AMP")}
    full = dict(u=[], p=[])
    for s0 in range(0, B, chunk):
        sl = slice(s0, s0 + chunk)
        u = T_t[None, sl, None, :] - th_t[:, sl, :, None]                        # u_ijp: (2, b, j, p)
        wgt = (tau - (u < 0).to(torch.float64)).abs()
        a = u.abs()
        H = torch.where(a <= kap, 0.5 * u * u, kap * (a - 0.5 * kap))
        c = u.clamp(-kap, kap)
        p = wgt * c
        du = dT_t[None, sl, None, :] + U * a
        K = keep_t[None, sl]
        out["G"][:, sl] = torch.matmul(p, K)
        out["RHO"][:, sl] = torch.matmul(wgt * H, K)
        out["absG"][:, sl] = torch.matmul(p.abs(), K)
        out["E"][:, sl] = torch.matmul(du + 3.0 * U * c.abs(), K)
        out["AMP"][:, sl] = torch.matmul(wgt * c.abs() * du, K)
        if terms:
            full["u"].append(u.numpy()); full["p"].append(p.numpy())
    res = dict(th=th, z=z, rank=rank, keep=keep, m=m, r=r, T=T, dT=dT, s=s, B=B, N=N, kappa=kap, drops=drops,
               **{k: v.numpy() for k, v in out.items()})
    if terms:
        res.update(u=np.concatenate(full["u"], axis=1), p=np.concatenate(full["p"], axis=1))
    return res


def soft_ref(base, drop, w=None, wmax=None):
    """-> tqc_cases.tqc_ref's dictionary (loss, dy, keep, abs_td, G, ...) for the soft law held in `base`: given T_p and the kept set,
    u, rho, L, dy, the scale and the weighting are f18's, and so is that function."""
    return TQ.tqc_ref(base, drop, w, wmax)


def soft_ref_of(theta, theta_t, rew, done, logp, log_alpha, gamma_n, kappa, drop, w=None, wmax=None):
    return soft_ref(soft_base(theta, theta_t, rew, done, logp, log_alpha, gamma_n, kappa, [drop], terms=True), drop, w, wmax)


def soft_bounds(ref, blocks):
    """tqc_cases.tqc_bounds on a soft_base: the derivation is f18's, term by term, with the error of a target atom enlarged by what
    the shift adds -- one rounding for alpha * logp, one for the subtraction, and the expf error (EXPF_ULPS ulp = 2 EXPF_ULPS u
    relative on alpha), all scaled by c.  That enlargement is soft_base's `dT`; it reaches dy through E, the loss through AMP and
    |TD| through the mean of the kept dT_p, exactly as f18's dT does.  Nothing here is taken from a kernel's output."""
    return TQ.tqc_bounds(ref, blocks)


# ------------------------------------------------------------------------------------------------ the mean-of-critics actor law, float64
def dpg_mean_ref(theta):
    """theta (2, B, N) -> dict: loss = -(1 / B) sum_b Qbar_b, Qbar (B,) = (1 / (2 N)) sum_i sum_j theta, dy (2, B, N) = -1 / (B 2 N)."""
    th = np.asarray(theta, np.float64)
    _, B, N = th.shape
    qbar = th.sum(axis=(0, 2)) / (2 * N)
    return dict(loss=float(-qbar.sum() / B), Qbar=qbar, dy=np.full(th.shape, -1.0 / (B * 2 * N)), th=th, B=B, N=N)


def dpg_mean_dy_fp32(B, N):
    """The gradient element as the kernel forms it: -(1.0f / ((float)B * (float)(2 * N)))."""
    return -(np.float32(1.0) / (np.float32(B) * np.float32(2 * N)))


def dpg_mean_loss_bound(ref, blocks):
    """Absolute bound on the mean-actor loss, after quantile_cases.dpg_loss_bound.  Qbar_b: one add per lane (the two nets), the
    butterfly (6 adds deep), times fl(1 / (2 N)) (two roundings): |dQbar| <= 7 u sum_ij |theta| / (2 N) + 2 u |Qbar|.  The rows are
    added along ceil(B / (4 blocks)) + 8 + ceil(blocks / 256) + 8 adds and scaled by fl(-1 / B) (two roundings)."""
    B, N = ref["B"], ref["N"]
    dq = 7.0 * U * np.abs(ref["th"]).sum(axis=(0, 2)) / (2 * N) + 2.0 * U * np.abs(ref["Qbar"])
    chain = -(-B // (4 * blocks)) + 8 + -(-blocks // 256) + 8 + 2
    return SLOP * float(dq.sum() / B + chain * U * np.abs(ref["Qbar"]).sum() / B)


# ------------------------------------------------------------------------------------------------ the laws, torch (autograd), literal
def soft_torch(theta, theta_t, rew, done, logp, alpha, gamma_n, kappa, drop, wh=None):
    """Shift ALL pooled atoms by alpha logp', sort them with a stable sort, take the first M, apply the quantile Huber loss: the
    literal formulation (tqc_cases.tqc_torch on the shifted heads).  -> (loss, the kept pool indices (B, M), T of the kept (B, M))."""
    return TQ.tqc_torch(theta, theta_t - (alpha * logp)[None, :, None], rew, done, gamma_n, kappa, drop, wh)


def dpg_mean_torch(theta):
    """-mean_b of the mean over both heads of the heads' means."""
    return -theta.mean(dim=2).mean(dim=0).mean()


# ------------------------------------------------------------------------------------------------ inputs
def logp_normal(B, seed):
    """Log-probabilities of the size a squashed Gaussian of a few dimensions gives: normal around -1, of both signs."""
    return (np.random.default_rng(seed).standard_normal(B) * 1.5 - 1.0).astype(np.float32)


def logp_dyadic(B, seed):
    """Multiples of 2^-4 in [-1.5, 1.5], of both signs: with log_alpha = 0 (expf gives exactly 1) z_p - s_b is a multiple of 2^-4
    below 4, and every later quantity of tqc_cases.dyadic_case stays exact (the tests assert it on the reference)."""
    lp = (np.random.default_rng(seed).integers(-24, 25, B) / 16.0).astype(np.float32)
    lp[0], lp[1] = np.float32(0.75), np.float32(-0.75)
    return lp


# ------------------------------------------------------------------------------------------------ the CPU autograd agent
def make_tqc_sac_ref(O, A, hp, cap, actor, q1, q2, drop, kappa=1.0, alpha_lr=5e-3, alpha=None):
    from oracle import pql_ref_cpu as ref

    class TqcSACRef(ref.SACRef):
        """SACRef with the soft truncated target and its quantile Huber loss in place of the entropy-regularised twin MSE, and the mean
        over all atoms of both nets in place of min Q in the actor loss; everything else (draws, optimisers, temperature step,
        Polyak) is SACRef's.  wh (B,): the step's importance weights w / wmax (None: uniform)."""

        def update_once(self, idx, eps_next, eps_cur, wh=None):
            hp = self.hp
            obs, act, rew, nobs, done = self.ring.gather(idx)
            if hp.obs_norm:
                obs = ref.normalize_ref(obs, self.norm, clamp=False); nobs = ref.normalize_ref(nobs, self.norm, clamp=False)
            with torch.no_grad():
                na, nlogp = ref.squashed_gaussian_ref(self.actor, nobs, eps_next)
                theta_t = torch.stack(ref.twin_forward_ref(self.t1, self.t2, nobs, na))
            theta = torch.stack(ref.twin_forward_ref(self.q1, self.q2, obs, act))
            closs, _, T = soft_torch(theta, theta_t, rew.reshape(-1), done.reshape(-1), nlogp.reshape(-1), self.alpha(), hp.gamma ** hp.nstep,
                                     kappa, drop, wh)
            self.abs_td = TQ.tqc_abs_td_torch(theta.detach(), T)
            cp = [*self.q1, *self.q2]
            self.copt.apply(list(torch.autograd.grad(closs, cp)), hp.max_grad_norm)
            frozen1 = [p.detach() for p in self.q1]; frozen2 = [p.detach() for p in self.q2]
            a, logp = ref.squashed_gaussian_ref(self.actor, obs, eps_cur)
            lq = dpg_mean_torch(torch.stack(ref.twin_forward_ref(frozen1, frozen2, obs, a)))
            aloss = (self.alpha() * logp).mean() + lq
            self.aopt.apply(list(torch.autograd.grad(aloss, self.actor)), hp.max_grad_norm)
            alpha_loss = None
            if self.fixed_alpha is None:
                alpha_loss = (self.log_alpha.exp() * (-logp - self.target_entropy).detach()).mean()
                self.alpha_opt.apply(list(torch.autograd.grad(alpha_loss, [self.log_alpha])), hp.max_grad_norm)
            ref.polyak_ref([*self.t1, *self.t2], [p.detach() for p in cp], hp.tau)
            return float(closs.detach()), float(aloss.detach()), None if alpha_loss is None else float(alpha_loss.detach())

    return TqcSACRef(O, A, hp, cap, actor, q1, q2, alpha_lr=alpha_lr, alpha=alpha)
