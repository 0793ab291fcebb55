"""The truncated pooled target of the quantile critic (include/pqlk.h, "Truncated pooled targets") as a float64 reference written
from the prose, a literal torch formulation for autograd, the inputs the kernel tests run on, the error bounds those tests hold the
kernel to, and CPU autograd learners for the learner tests.  Nothing here runs on a GPU; tests/test_tqc_cpu.py checks the reference
against torch.autograd.  Conventions (u, SLOP, f32, taus, the fold) are those of tests/quantile_cases.py.
"""
import numpy as np
import torch

import quantile_cases as Q

U, SLOP = Q.U, Q.SLOP


def drops_for(N):
    """The d values the kernel tests run at N quantiles: 0, 1, N / 2, N - 1 where valid (0 <= d <= N - 1), without repeats."""
    return sorted({d for d in (0, 1, N // 2, N - 1) if 0 <= d <= N - 1})


# ------------------------------------------------------------------------------------------------ the law, float64
def tqc_base(theta, theta_t, rew, done, gamma_n, kappa, drops, terms=False, chunk=256):
    """The law for every d of `drops` at once, without the weights: the pool, its ranks, the targets, and per d the sums over the kept
    atoms that the loss, the gradient and the bounds are made of.  theta, theta_t: (2, B, N); rew, done: (B,).  The (i, b, j, p)
    terms are formed in float64 for `chunk` rows at a time (torch on the CPU, for its threads) and only their sums over the kept p are
    held; terms=True (small cases) also holds u and the gradient's terms p_ijp = |tau_j - 1{u < 0}| clamp(u)."""
    th, tt = np.asarray(theta, np.float64), np.asarray(theta_t, np.float64)
    r, d = np.asarray(rew, np.float64), np.asarray(done, np.float64)
    g, kap = Q.f32(gamma_n), Q.f32(kappa)
    _, B, N = th.shape
    drops = [int(x) for x in drops]
    assert all(0 <= x <= N - 1 for x in drops)
    z = np.concatenate([tt[0], tt[1]], axis=1)                                   # z_p, p = i N + k: (B, 2 N)
    idx = np.arange(2 * N)
    rank = np.zeros((B, 2 * N), np.int64)
    for q in range(2 * N):                                                       # rank(p) = #{q: z_q < z_p} + #{q < p: z_q = z_p}
        zq = z[:, q: q + 1]
        rank += (zq < z) | ((zq == z) & (q < idx)[None, :])
    keep = np.stack([rank < 2 * (N - x) for x in drops], axis=2)                 # the kept sets: (B, 2 N, d)
    m = (1.0 - d) * g                                                            # c of the prose
    T = r[:, None] + m[:, None] * z                                              # T_p
    dT = U * (3.0 * np.abs(m[:, None] * z) + np.abs(r)[:, None])                 # (for the bounds: see tqc_bounds)
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
        out["G"][:, sl] = torch.matmul(p, K)                                     # sum over the kept p of the gradient's terms
        out["RHO"][:, sl] = torch.matmul(wgt * H, K)                             # ... of the loss's terms (before / kappa)
        out["absG"][:, sl] = torch.matmul(p.abs(), K)
        out["E"][:, sl] = torch.matmul(du + 3.0 * U * c.abs(), K)
        out["AMP"][:, sl] = torch.matmul(wgt * c.abs() * du, K)
        if terms:
            full["u"].append(u.numpy()); full["p"].append(p.numpy())
    res = dict(th=th, z=z, rank=rank, keep=keep, m=m, r=r, T=T, dT=dT, B=B, N=N, kappa=kap, drops=drops,
               **{k: v.numpy() for k, v in out.items()})
    if terms:
        res.update(u=np.concatenate(full["u"], axis=1), p=np.concatenate(full["p"], axis=1))
    return res


def tqc_ref(base, drop, w=None, wmax=None):
    """-> dict: loss, dy (2, B, N), keep (B, 2 N) bool, abs_td (B,), G (the gradient's chain sums, (2, B, N)), and the pieces the bounds
    need, for d = drop (one of base's drops) and the weights w / wmax[0]."""
    s = base
    B, N, kap = s["B"], s["N"], s["kappa"]
    k = s["drops"].index(int(drop))
    M = 2 * (N - int(drop))
    keep = s["keep"][:, :, k]
    assert (keep.sum(axis=1) == M).all()
    wh = np.ones(B) if w is None else np.asarray(w, np.float64) / float(np.asarray(wmax, np.float64).reshape(-1)[0])
    rho_row = s["RHO"][..., k].sum(axis=2) / kap                                 # (2, B): sum over j and the kept p of rho
    loss = float((rho_row * wh[None]).sum() / (B * M))
    G = s["G"][..., k]
    dy = -(wh[None, :, None] / (B * M)) * G / kap
    mT = (s["T"] * keep).sum(axis=1) / M
    abs_td = np.abs(mT[None] - s["th"].mean(axis=2)).max(axis=0)
    return dict(loss=loss, dy=dy, keep=keep, abs_td=abs_td, G=G, wh=wh, M=M, mT=mT, k=k, base=s)


def tqc_ref_of(theta, theta_t, rew, done, gamma_n, kappa, drop, w=None, wmax=None):
    return tqc_ref(tqc_base(theta, theta_t, rew, done, gamma_n, kappa, [drop], terms=True), drop, w, wmax)


# ------------------------------------------------------------------------------------------------ the law, torch (autograd), literal
def tqc_torch(theta, theta_t, rew, done, gamma_n, kappa, drop, wh=None):
    """Sort the pool with a stable sort, take the first M, apply the Huber quantile loss: one differentiable expression in theta's
    dtype.  -> (loss, the kept pool indices (B, M), T of the kept atoms (B, M))."""
    _, B, N = theta.shape
    M = 2 * (N - int(drop))
    z = torch.cat([theta_t[0], theta_t[1]], dim=1)
    zs, order = torch.sort(z, dim=1, stable=True)
    T = rew[:, None] + ((1.0 - done) * gamma_n)[:, None] * zs[:, :M]
    u = T[None, :, None, :] - theta[:, :, :, None]
    tau = ((2.0 * torch.arange(N, dtype=theta.dtype) + 1.0) / (2.0 * N))[None, None, :, None]
    a = u.abs()
    H = torch.where(a <= kappa, 0.5 * u * u, kappa * (a - 0.5 * kappa))
    rho = (tau - (u.detach() < 0).to(theta.dtype)).abs() * H / kappa
    row = rho.sum(dim=(2, 3))
    if wh is not None:
        row = row * wh[None]
    return row.sum() / (B * M), order[:, :M], T


def tqc_abs_td_torch(theta, T):
    return (T.mean(dim=1)[None] - theta.mean(dim=2)).abs().max(dim=0).values


# ------------------------------------------------------------------------------------------------ inputs
def dyadic_case(B, N, seed):
    """quantile_cases.dyadic_case's data (multiples of 2^-4 in [-1.5, 1.5]; with gamma_n = 0.5 and kappa = 1 every T_p, u_ijp, term
    and partial sum of at most 2 N <= 128 terms is exact in fp32: a term is a multiple of 2^-6 / N of size <= 1, a partial sum below
    128, at most 19 significant bits) with rows made for the ranking:
      rows 0 ... 3   the pooled atoms take two (rows 0, 1) or three (rows 2, 3) values only, not done: whatever M, the cut falls
                     inside a group of equal atoms or at its edge;
      rows 4 ... 7   done = 1 (every T_p is r);
      rows 8 ... 11  the two target nets are identical, not done;
      row 12         net 1 = net 0 in reverse order."""
    assert B >= 16 and B & (B - 1) == 0 and N & (N - 1) == 0
    rng = np.random.default_rng(seed)
    q = lambda shape: (rng.integers(-24, 25, shape) / 16.0).astype(np.float32)   # noqa: E731
    theta, theta_t, rew = q((2, B, N)), q((2, B, N)), q((B,))
    done = (rng.random(B) < 0.25).astype(np.float32)
    done[:16] = 0.0
    done[4:8] = 1.0
    theta_t[:, 0:2] = rng.choice(np.array([-1.0, 0.5], np.float32), (2, 2, N))
    theta_t[:, 2:4] = rng.choice(np.array([-0.75, 0.25, 1.5], np.float32), (2, 2, N))
    theta_t[1, 8:12] = theta_t[0, 8:12]
    theta_t[1, 12] = theta_t[0, 12, ::-1]
    return dict(theta=theta, theta_t=theta_t, rew=rew, done=done)


def dy_tail_fp32(G, kappa, B, M, wh=None):
    """The tail of dy as the kernel evaluates it, in fp32, on exact chain sums G: (G / kappa) * (1.0f / ((float)B * (float)M)),
    (* wh), negated."""
    v = (np.asarray(G, np.float32) / np.float32(kappa)) * (np.float32(1.0) / (np.float32(B) * np.float32(M)))
    if wh is not None:
        v = np.asarray(wh, np.float32)[None, :, None] * v
    return -v


# ------------------------------------------------------------------------------------------------ bounds
def tqc_bounds(ref, blocks):
    """-> (dy_bound (2, B, N) absolute, loss_bound relative, abs_td_bound (B,) absolute) for tqc_ref's output `ref`: the derivation of
    quantile_cases.qr_bounds with the kept atoms in place of the N targets.

    The kept set itself is exact: the ranks compare raw fp32 inputs.
    T_p = fl(r + fl(fl((1 - d) gamma_n) z_p)): |dT_p| <= u (3 |m z_p| + |r|);  u_ijp = fl(T_p - theta_j): |du| <= dT_p + u |u_ijp|.
    dy.  A term wgt * clamp(u) moves by at most |du| (clamp is 1-Lipschitz, wgt <= 1, also across a sign change of u) plus 3 u |clamp|
    (tau's division, tau - 1, the product).  The M kept terms are added in sequence: (M - 1) u sum |terms|.  Then / kappa, 1 / (B M)
    (a product, a division) and its product, w / wmax and its product: six roundings of the result.
    loss.  All rho terms are >= 0; the longest path from a term to the loss has quantile_cases.loss_chain(B, M, blocks) adds (the
    lane's chain runs over the M kept atoms); each term carries 12 roundings of its own, and the error of u_ijp enters through H
    with slope <= |c| + |du|: sum wgt |c| |du| / (kappa B M), turned into a count of roundings by dividing by u * loss.
    abs_td.  mean_{kept p} T_p: one add per lane (its two atoms), the butterfly (6 adds deep), times fl(1 / M) (two roundings):
    (sum dT_p + 7 u sum |T_p|) / M + 2 u |mean|; a head's mean as in qr_bounds; their difference one more rounding."""
    s, k = ref["base"], ref["k"]
    B, N, kap, M, keep, dT = s["B"], s["N"], s["kappa"], ref["M"], ref["keep"], s["dT"]
    scale = ref["wh"][None, :, None] / (B * M * kap)
    dy_bound = SLOP * (scale * (s["E"][..., k] + (M - 1) * U * s["absG"][..., k]) + 6.0 * U * np.abs(ref["dy"]))
    amp = float((s["AMP"][..., k].sum(axis=2) * ref["wh"][None]).sum() / (kap * B * M)) / (U * ref["loss"])
    loss_bound = SLOP * (Q.loss_chain(B, M, blocks) + 12 + amp) * U
    mth = s["th"].mean(axis=2)
    e_T = ((dT * keep).sum(axis=1) + 7.0 * U * (np.abs(s["T"]) * keep).sum(axis=1)) / M + 2.0 * U * np.abs(ref["mT"])
    e_th = 6.0 * U * np.abs(s["th"]).sum(axis=2) / N + 2.0 * U * np.abs(mth)
    abs_td_bound = SLOP * (e_T[None] + e_th + U * np.abs(ref["mT"][None] - mth)).max(axis=0)
    return dy_bound, loss_bound, abs_td_bound


# ------------------------------------------------------------------------------------------------ CPU autograd learners
def _oracle():
    from oracle import pql_ref_cpu as ref
    return ref


def _heads(ref, self, idx, draw, clamp=True):
    hp = self.hp
    obs, act, rew, nobs, done = self.ring.gather(idx)
    if hp.obs_norm:
        obs = ref.normalize_ref(obs, self.norm, clamp=clamp); nobs = ref.normalize_ref(nobs, self.norm, clamp=clamp)
    with torch.no_grad():
        na = ref.target_noise_ref(ref.actor_forward_ref(self.actor, nobs), draw, hp.tgt_pol_std, hp.tgt_pol_noise_bound)
        theta_t = torch.stack(ref.twin_forward_ref(self.t1, self.t2, nobs, na))
    theta = torch.stack(ref.twin_forward_ref(self.q1, self.q2, obs, act))
    return obs, theta, theta_t, rew.reshape(-1), done.reshape(-1)


def make_v_ref(O, A, hp, cap, q1, q2, drop, kappa=1.0):
    ref = _oracle()

    class TqcVLearnerRef(ref.VLearnerRef):
        """VLearnerRef with the truncated pooled quantile Huber loss in place of the twin MSE; `wh` (B,), set before `learn`: the
        step's importance weights w / wmax (None: uniform)."""
        wh = None

        def loss_and_grads(self, idx=None, draw=None, generator=None):
            _, theta, theta_t, rew, done = _heads(ref, self, idx, draw)
            loss, _, T = tqc_torch(theta, theta_t, rew, done, self.hp.gamma ** self.hp.nstep, kappa, drop, self.wh)
            self.abs_td = tqc_abs_td_torch(theta.detach(), T)
            return loss, torch.autograd.grad(loss, [*self.q1, *self.q2])

    return TqcVLearnerRef(O, A, hp, cap, q1, q2)


def make_ddpg_ref(O, A, hp, cap, actor, q1, q2, drop, kappa=1.0):
    ref = _oracle()

    class TqcDDPGRef(ref.DDPGRef):
        def update_once(self, idx, draw, wh=None):
            hp = self.hp
            obs, theta, theta_t, rew, done = _heads(ref, self, idx, draw, clamp=False)
            closs, _, T = tqc_torch(theta, theta_t, rew, done, hp.gamma ** hp.nstep, kappa, drop, wh)
            self.abs_td = tqc_abs_td_torch(theta.detach(), T)
            cp = [*self.q1, *self.q2]
            self.copt.apply(list(torch.autograd.grad(closs, cp)), hp.max_grad_norm)
            frozen1 = [p.detach() for p in self.q1]; frozen2 = [p.detach() for p in self.q2]
            aloss = Q.dpg_quantile_torch(torch.stack(ref.twin_forward_ref(frozen1, frozen2, obs, ref.actor_forward_ref(self.actor, obs))))
            self.aopt.apply(list(torch.autograd.grad(aloss, self.actor)), hp.max_grad_norm)
            ref.polyak_ref([*self.t1, *self.t2], [p.detach() for p in cp], hp.tau)
            return float(closs.detach()), float(aloss.detach())

    return TqcDDPGRef(O, A, hp, cap, actor, q1, q2)


def _tied_case(B, N, seed):
    """Normal data with rows made for the ranking: row 0 two values only, row 1 all atoms equal, row 2 the two target nets identical,
    row 3 net 1 = net 0 reversed, row 4 done with ties; done elsewhere as drawn."""
    case = Q.normal_case(B, N, seed, per=True)
    rng = np.random.default_rng(seed + 1)
    tt = case["theta_t"]
    def two_values():   # N of the 2 N atoms low (3 of 4 at N = 2), anywhere in the pool: no cut M = 2 or 2 N - 2 falls on the edge
        pool = np.full(2 * N, 0.75, np.float32)
        pool[rng.permutation(2 * N)[: N if N > 2 else 3]] = np.float32(-0.5)
        return pool.reshape(2, N)

    tt[:, 0] = two_values()
    tt[:, 1] = np.float32(0.25)
    tt[1, 2] = tt[0, 2]
    tt[1, 3] = tt[0, 3, ::-1]
    tt[:, 4] = two_values()
    case["done"][:5] = np.array([0, 0, 0, 0, 1], np.float32)
    case["done"][5] = 1.0
    return case
