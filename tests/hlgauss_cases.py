"""The HL-Gauss law of the categorical critic (include/pqlk.h, "HL-Gauss loss for the categorical twin critic") as a float64
reference written from the prose, a torch float64 autograd form of it, the two designs the kernel tests run on -- an exact one whose
every output is known in closed form, and a generic one -- and the error bound the generic design is held to.  Nothing here runs on a
GPU; tests/test_hlgauss_cases_cpu.py proves the designs.

U = 2^-24 below is the unit roundoff of fp32 round-to-nearest: fl(x op y) = (x op y)(1 + e), |e| <= U; an ulp of a value in
[0.5, 1) is 2^-24 as well.
"""
import math

import numpy as np
import torch

from quantile_cases import SLOP, U, f32, survives_fp32  # noqa: F401  (re-exported)

F32 = np.float32
LOSS_MAX_BLOCKS, ROWS_PER_BLOCK = 1024, 4            # k_hlgauss_ce<NJ, PER>: loss_blocks(b, k > 1) of pql_amd/csrc/loss.hip
B_PAST_CAP = ROWS_PER_BLOCK * LOSS_MAX_BLOCKS + 7     # the first batch whose rows wrap round the capped grid
SIGMA = 0.75                                          # algo.hl_sigma's default
NORM_FLOOR = 1.44                                     # c(u_K) - c(u_0) >= this at SIGMA with y inside the support (proved on CPU)
# Accuracy of the device math functions.  The ROCm documentation at hand states none for erff, expf or logf, so these are the
# OpenCL 3.0 full-profile bounds (table 7.4): erf <= 16 ulp, exp <= 3 ulp, log <= 3 ulp.
E_ERF, E_EXP, E_LOG = 16.0, 3.0, 3.0
SLOPE_MARGIN = 0.01                                  # hl_bounds: the neighbourhood of u_k over which erf' is maximised
SAT_JUMP = 1.0 - math.erf(4.0)                        # c(u) steps by this at |u| = 4, where fp32 and float64 may take different sides

_erf = np.vectorize(math.erf, otypes=[np.float64])


def loss_blocks(B):
    return min(-(-B // ROWS_PER_BLOCK), LOSS_MAX_BLOCKS)


def bins(v_min, v_max, K, sigma_ratio):
    """-> (dz, inv, edges (K + 1,)) in fp32, each formed as the law forms it: dz and inv in double and rounded once, the edges
    e_k = v_min + ((float)k - 0.5f) * dz op by op in fp32."""
    dz = F32((np.float64(F32(v_max)) - np.float64(F32(v_min))) / np.float64(K - 1))
    inv = F32(1.0 / (np.float64(F32(sigma_ratio)) * np.float64(dz) * np.sqrt(2.0)))
    edges = F32(v_min) + (np.arange(K + 1, dtype=F32) - F32(0.5)) * dz
    assert edges.dtype == F32 and dz.dtype == F32 and inv.dtype == F32
    return dz, inv, edges


def cdf(u):
    """c(u) of the law on float64 u."""
    u = np.asarray(u, np.float64)
    return np.where(u >= 4.0, 1.0, np.where(u <= -4.0, -1.0, _erf(np.clip(u, -4.0, 4.0))))


# ------------------------------------------------------------------------------------------------ the law, float64
def hl_ref(logits, logits_t, rew, done, z, gamma_n, v_min, v_max, sigma_ratio, w=None, wmax=None):
    """logits, logits_t: (2, B, K); rew, done, w: (B,); z: (K,); wmax: (1,).  -> dict: t (B, K), dy (2, B, K), rows (B,) the row
    losses wh (l_0 + l_1), loss, abs_td (B,), y (B,), and the pieces the bound needs.  Every input is taken at its fp32 value, the
    edges and inv are the fp32 values of `bins`: only rounding inside the kernel separates it from this."""
    x, xt = np.asarray(logits, np.float64), np.asarray(logits_t, np.float64)
    r, d, z = np.asarray(rew, np.float64), np.asarray(done, np.float64), np.asarray(z, np.float64)
    _, B, K = x.shape
    dz, inv, edges = bins(v_min, v_max, K, sigma_ratio)
    inv, edges = np.float64(inv), edges.astype(np.float64)

    def softmax(a):
        m = a.max(axis=-1, keepdims=True)
        e = np.exp(a - m)
        s = e.sum(axis=-1, keepdims=True)
        return e / s, m[..., 0] + np.log(s[..., 0]), m

    pt, _, mt = softmax(xt)
    E = (pt * z).sum(axis=-1)                                   # (2, B)
    mult = (1.0 - d) * f32(gamma_n)
    Emin = np.minimum(E[0], E[1])
    y = np.clip(r + mult * Emin, f32(v_min), f32(v_max))
    u = (edges[None, :] - y[:, None]) * inv                      # (B, K + 1)
    c = cdf(u)
    norm = c[:, -1] - c[:, 0]
    t = (c[:, 1:] - c[:, :-1]) / norm[:, None]
    p, lse, m = softmax(x)
    gap = lse[:, :, None] - x                                    # lse - x_k >= 0
    terms = np.where(t[None] == 0.0, 0.0, t[None] * gap)
    l = terms.sum(axis=-1)                                       # (2, B)
    wh = np.ones(B) if w is None else np.asarray(w, np.float64) / float(np.asarray(wmax, np.float64).reshape(-1)[0])
    rows = wh * (l[0] + l[1])
    dy = (wh[None, :, None] / B) * (p - t[None])
    Q = (p * z).sum(axis=-1)
    abs_td = np.abs(Q - y[None]).max(axis=0)
    return dict(t=t, dy=dy, rows=rows, loss=float(rows.sum() / B), abs_td=abs_td, y=y, u=u, c=c, norm=norm, p=p, pt=pt, x=x, xt=xt, m=m, mt=mt,
                lse=lse, gap=gap, terms=terms, E=E, Emin=Emin, mult=mult, r=r, z=z, wh=wh, Q=Q, inv=float(inv), B=B, K=K)


# ------------------------------------------------------------------------------------------------ the law, torch (autograd)
def hl_target_torch(logits_t, rew, done, z, gamma_n, v_min, v_max, sigma_ratio):
    """The target pmf (B, K) as torch ops in logits_t's dtype (float64 in the tests), no gradient."""
    K = logits_t.shape[-1]
    _, inv, edges = bins(v_min, v_max, K, sigma_ratio)
    with torch.no_grad():
        E = (torch.softmax(logits_t, dim=-1) * z).sum(dim=-1)
        y = (rew + ((1.0 - done) * f32(gamma_n)) * torch.minimum(E[0], E[1])).clamp(f32(v_min), f32(v_max))
        u = (torch.from_numpy(edges.astype(np.float64)).to(logits_t.dtype)[None] - y[:, None]) * float(inv)
        c = torch.where(u >= 4.0, torch.ones_like(u), torch.where(u <= -4.0, -torch.ones_like(u), torch.erf(u)))
        return (c[:, 1:] - c[:, :-1]) / (c[:, -1:] - c[:, :1]), y


def hl_torch(logits, logits_t, rew, done, z, gamma_n, v_min, v_max, sigma_ratio, wh=None):
    """The loss as one differentiable torch expression: a soft-target cross-entropy of each net's logits against the HL-Gauss
    target, a (weighted) batch mean, the twin nets added.  logits carries the gradient."""
    t, _ = hl_target_torch(logits_t, rew, done, z, gamma_n, v_min, v_max, sigma_ratio)
    row = -(t[None] * torch.log_softmax(logits, dim=-1)).sum(dim=-1).sum(dim=0)     # (B,): l_0b + l_1b
    if wh is not None:
        row = row * wh
    return row.sum() / logits.shape[1]


def abs_td_torch(logits, logits_t, rew, done, z, gamma_n, v_min, v_max, sigma_ratio):
    with torch.no_grad():
        _, y = hl_target_torch(logits_t, rew, done, z, gamma_n, v_min, v_max, sigma_ratio)
        return ((torch.softmax(logits, dim=-1) * z).sum(dim=-1) - y[None]).abs().max(dim=0).values


# ------------------------------------------------------------------------------------------------ the exact design
EXACT_SIGMA, EXACT_GAMMA, COLD = 0.05, 0.5, -200.0
EXACT_SUPPORTS = [(-10.0, 10.0, 2), (-10.0, 10.0, 5), (-10.0, 10.0, 33), (-10.0, 10.0, 65), (-10.0, 10.0, 129), (0.0, 255.0, 256)]
EXACT_KS = [K for _, _, K in EXACT_SUPPORTS]
EXACT_B = [1, 5, 263, B_PAST_CAP]
ROW_PERIOD = 48   # terminal x (inside, past v_min, past v_max) x which net is smaller x net 0 hot on the target bin x net 1


def exact_support(K):
    return next(s for s in EXACT_SUPPORTS if s[2] == K)


def exact_case(B, K, per=False):
    """-> dict of fp32 inputs and the closed-form outputs.  Logits are 0 on one atom and COLD elsewhere (an exactly one-hot softmax
    in fp32: expf(-200) = 0), sigma_ratio = 0.05 (every edge at |u| >= 7.07: every c is +-1), gamma_n = 0.5, dz dyadic; the reward
    makes y a bin centre, or sends it three bins past an end, where the clamp puts it on the end's centre.  Row i:
    terminal = i % 2; placement = (i // 2) % 3; net 1 has the smaller expectation iff (i // 6) % 2; net n's hot logit is the target
    bin iff (i // (12 << n)) % 2 == 1."""
    v_min, v_max, _ = exact_support(K)
    dz = (v_max - v_min) / (K - 1)
    z = v_min + dz * np.arange(K, dtype=np.float64)
    i = np.arange(B)
    term, place, swap = i % 2, (i // 2) % 3, (i // 6) % 2
    hot_on = np.stack([(i // 12) % 2, (i // 24) % 2])
    a = (7 * i + 3) % K
    b = (a + 1 + i % (K - 1)) % K                               # another atom, whatever K
    lo, hi = np.minimum(a, b), np.maximum(a, b)
    tgt_atoms = np.stack([np.where(swap == 1, hi, lo), np.where(swap == 1, lo, hi)])     # the hot atom of target net 0 / 1
    c = np.where(term == 1, 0.0, EXACT_GAMMA)
    inside = (5 * i + 1) % K
    y_raw = np.where(place == 0, z[inside], np.where(place == 1, v_min - 3.0 * dz, v_max + 3.0 * dz))
    j = np.where(place == 0, inside, np.where(place == 1, 0, K - 1))                      # the target bin
    rew = y_raw - c * z[lo]
    other = (j + 1 + i % (K - 1)) % K
    hot = np.where(hot_on == 1, j[None], other[None])                                      # (2, B)

    def onehot_logits(atoms):
        out = np.full((2, B, K), COLD, F32)
        np.put_along_axis(out, atoms[:, :, None], F32(0.0), axis=2)
        return out

    w = np.array([0.25, 0.5, 1.0])[i % 3] if per else np.ones(B)
    g = (w.astype(F32) / F32(1.0)) * (F32(1.0) / F32(B))         # fl(wh * fl(1 / B)): wh a power of two, the product is exact
    t = np.zeros((B, K), F32)
    t[i, j] = 1.0
    p = np.zeros((2, B, K), F32)
    np.put_along_axis(p, hot[:, :, None], F32(1.0), axis=2)
    dy = g[None, :, None] * (p - t[None])
    rows = w * (-COLD) * (hot != j[None]).sum(axis=0)             # wh * (l_0 + l_1), each l in {0, 200}
    parts = np.zeros(loss_blocks(B), np.float64)
    np.add.at(parts, (i % (ROWS_PER_BLOCK * loss_blocks(B))) // ROWS_PER_BLOCK, rows)
    loss = F32(F32(parts.sum()) * (F32(1.0) / F32(B)))
    out = dict(logits=onehot_logits(hot), logits_t=onehot_logits(tgt_atoms), rew=rew.astype(F32), done=term.astype(F32), z=z.astype(F32),
               gamma_n=EXACT_GAMMA, v_min=v_min, v_max=v_max, sigma=EXACT_SIGMA, K=K, B=B, j=j, hot=hot, tgt_atoms=tgt_atoms, place=place,
               t=t, dy=dy.astype(F32), rows=rows, parts=parts.astype(F32), loss=loss, abs_td=np.abs(z[hot] - z[j][None]).max(axis=0).astype(F32),
               w=w.astype(F32), wmax=np.ones(1, F32), y=z[j])
    for name, exact in (("rew", rew), ("z", z), ("dy", dy), ("parts", parts), ("abs_td", np.abs(z[hot] - z[j][None]).max(axis=0))):
        assert survives_fp32(exact), name
    assert parts.sum() < 2.0 ** 24 and (parts == np.round(parts)).all()   # exact integers: the fold's order cannot matter
    return out


# ------------------------------------------------------------------------------------------------ the generic design
GENERIC_KS, GENERIC_B, V_MIN, V_MAX, GAMMA_N = [51, 101, 256], 263, -10.0, 10.0, 0.99 ** 3


def generic_case(B, K, seed, per=False):
    """Gaussian logits (standard deviation 2) and rewards that place y, by row i % 5: anywhere inside the support; within one bin
    of v_min; within one bin of v_max; past v_min; past v_max (the last two clamp).  A quarter of the rows is terminal."""
    rng = np.random.default_rng(seed)
    logits = (2.0 * rng.standard_normal((2, B, K))).astype(F32)
    logits_t = (2.0 * rng.standard_normal((2, B, K))).astype(F32)
    z = torch.linspace(V_MIN, V_MAX, K).numpy()
    done = (rng.random(B) < 0.25).astype(F32)
    xt = logits_t.astype(np.float64)
    e = np.exp(xt - xt.max(axis=-1, keepdims=True))
    Emin = ((e / e.sum(axis=-1, keepdims=True)) * z.astype(np.float64)).sum(axis=-1).min(axis=0)
    dz = (V_MAX - V_MIN) / (K - 1)
    kind = np.arange(B) % 5
    want = np.choose(kind, [rng.uniform(V_MIN, V_MAX, B), V_MIN + rng.uniform(0.0, 1.0, B) * dz, V_MAX - rng.uniform(0.0, 1.0, B) * dz,
                            V_MIN - rng.uniform(0.1, 3.0, B), V_MAX + rng.uniform(0.1, 3.0, B)])
    rew = (want - (1.0 - done) * f32(GAMMA_N) * Emin).astype(F32)
    out = dict(logits=logits, logits_t=logits_t, rew=rew, done=done, z=z, gamma_n=GAMMA_N, v_min=V_MIN, v_max=V_MAX, sigma=SIGMA, K=K, B=B,
               kind=kind)
    if per:
        out["w"] = rng.uniform(0.05, 1.0, B).astype(F32)
        out["wmax"] = np.array([out["w"].max()], F32)
    return out


def ref_of(case, per=False):
    return hl_ref(case["logits"], case["logits_t"], case["rew"], case["done"], case["z"], case["gamma_n"], case["v_min"], case["v_max"],
                  case["sigma"], *((case["w"], case["wmax"]) if per else ()))


# ------------------------------------------------------------------------------------------------ the bound
def hl_bounds(ref, blocks):
    """-> dict of absolute first-order forward bounds for hl_ref's output `ref`: t (B, K), dy (2, B, K), loss (scalar), abs_td (B,).
    NJ = ceil(K / 64) atoms per lane; a row reduction is NJ - 1 adds in the lane and a butterfly 6 adds deep: `chain` = NJ + 5.

    softmax.  expf(x_k - m): the subtraction rounds (U |x_k - m| in the argument, so as much relative error in the result) and expf
      is good to E_EXP ulp = 2 E_EXP U: rho_e = U max_k |x_k - m| + 2 E_EXP U.  s is a sum of positive terms, chain deep:
      rho_s = rho_e + chain U.  p_k = fl(e_k / s): rho_p = rho_e + rho_s + U.
    dE.   E_i = sum_k fl(p_k z_k) along the same chain: |dE_i| <= (rho_p + (chain + 1) U) sum_k p_k |z_k|.
    dy_.  y = fl(r + fl(fl((1 - d) gamma_n) E)): three roundings, |.| <= U (3 |mult E| + |r|), plus mult max_i dE_i (min does
      not amplify); the clamp is 1-Lipschitz and exact.  This is `delta y`.
    du.   u_k = fl(fl(e_k - y) inv) on the reference's own fp32 e_k and inv: delta y * inv + 2 U |u_k|.
    dc.   erf'(v) = (2 / sqrt pi) exp(-v^2): du times the largest slope within SLOPE_MARGIN of u_k (du is asserted to be smaller
      than that margin), so `delta y * inv * (2 / sqrt pi)` at the mode and less in the tails, where a constant slope would charge
      every empty bin with the error of the mode; the evaluation itself E_ERF ulp of 2^-24 (|c| <= 1); SAT_JUMP where |u| may cross 4.
    dt.   t_k = fl(fl(c_{k+1} - c_k) / fl(c_K - c_0)): two erf evaluations over the normaliser, the normaliser's own two scaled by t_k,
      and the three fp32 ops of the quotient, 3 U t_k.  The normaliser enters at its floor NORM_FLOOR or its value, whichever is less.
    dy.   dy = fl(g fl(p_k - t_k)), g = fl(fl(w / wmax) fl(1 / B)): g (rho_p p_k + dt_k) + 5 U |dy|.
    loss. lse = fl(m + logf(s)): rho_s + 2 E_LOG U |log s| + U |lse|; a term t_k fl(lse - x_k) moves by dt_k gap_k + t_k (dlse + U gap_k)
      + U term_k; the terms are >= 0, so the sums along the row's chain, the two nets, the wave's row loop, the block sum and the fold
      (quantile_cases.loss_chain's count with chain for N) and the roundings of wh and of the scale add `adds + 4` U loss.
    abs_td.  |sum_k p_k z_k - y|: dE of the current nets, delta y, one rounding of the difference; max does not amplify."""
    B, K, inv = ref["B"], ref["K"], ref["inv"]
    chain = -(-K // 64) + 5
    sq = 2.0 / math.sqrt(math.pi)

    def rho(x, m):
        e = U * np.abs(x - m).max(axis=-1) + 2.0 * E_EXP * U                    # (2, B)
        s = e + chain * U
        return e, s, e + s + U

    _, _, rho_pt = rho(ref["xt"], ref["mt"])
    _, rho_s, rho_p = rho(ref["x"], ref["m"])
    absz = np.abs(ref["z"])
    dE_t = (rho_pt + (chain + 1) * U) * (ref["pt"] * absz).sum(axis=-1)          # (2, B)
    d_y = ref["mult"] * dE_t.max(axis=0) + U * (3.0 * np.abs(ref["mult"] * ref["Emin"]) + np.abs(ref["r"]))     # (B,)
    u = ref["u"]
    d_u = d_y[:, None] * inv + 2.0 * U * np.abs(u)
    assert d_u.max() < SLOPE_MARGIN
    slope = sq * np.exp(-np.maximum(np.abs(u) - SLOPE_MARGIN, 0.0) ** 2)         # the largest erf' within SLOPE_MARGIN of u_k
    d_c = slope * d_u + E_ERF * U + SAT_JUMP                                     # (B, K + 1)
    norm = np.minimum(ref["norm"], NORM_FLOOR)[:, None]
    t = ref["t"]
    d_t = (d_c[:, 1:] + d_c[:, :-1]) / norm + t * (d_c[:, -1:] + d_c[:, :1]) / norm + 3.0 * U * t              # (B, K)
    g = ref["wh"][None, :, None] / B
    d_dy = g * (rho_p[:, :, None] * ref["p"] + d_t[None]) + 5.0 * U * np.abs(ref["dy"])
    d_lse = rho_s + 2.0 * E_LOG * U * np.abs(ref["lse"] - ref["m"][..., 0]) + U * np.abs(ref["lse"])            # (2, B)
    d_terms = d_t[None] * ref["gap"] + t[None] * (d_lse[:, :, None] + U * ref["gap"]) + U * ref["terms"]
    adds = chain + 1 + -(-B // (ROWS_PER_BLOCK * blocks)) + 8 + -(-blocks // 256) + 8
    d_loss = float((ref["wh"] * d_terms.sum(axis=(0, 2))).sum() / B) + (adds + 4) * U * ref["loss"]
    dE = (rho_p + (chain + 1) * U) * (ref["p"] * absz).sum(axis=-1)
    d_td = (dE + d_y[None] + U * np.abs(ref["Q"] - ref["y"][None])).max(axis=0)
    return dict(t=SLOP * d_t, dy=SLOP * d_dy, loss=SLOP * d_loss, abs_td=SLOP * d_td, d_y=d_y)


# ------------------------------------------------------------------------------------------------ CPU autograd learners
def _oracle():
    from oracle import pql_ref_cpu as ref
    return ref


def _hl_step_loss(self, ref, obs, act, rew, nobs, done, draw, wh, sigma):
    """The HL-Gauss critic loss of one batch on a reference learner's nets (fp32 torch, as the oracle's other losses); leaves the
    row's new priority in self.abs_td."""
    hp = self.hp
    gn = hp.gamma ** hp.nstep
    z = torch.linspace(hp.v_min, hp.v_max, hp.num_atoms)
    with torch.no_grad():
        na = ref.target_noise_ref(ref.actor_forward_ref(self.actor, nobs), draw, hp.tgt_pol_std, hp.tgt_pol_noise_bound)
        logits_t = torch.stack(ref.twin_forward_ref(self.t1, self.t2, nobs, na))
    logits = torch.stack(ref.twin_forward_ref(self.q1, self.q2, obs, act))
    args = (logits_t, rew.reshape(-1), done.reshape(-1), z, gn, hp.v_min, hp.v_max, sigma)
    self.abs_td = abs_td_torch(logits.detach(), *args)
    return hl_torch(logits, *args, wh=wh)


def make_v_ref(O, A, hp, cap, q1, q2, sigma=SIGMA):
    ref = _oracle()

    class HLGaussVLearnerRef(ref.VLearnerRef):
        """VLearnerRef (hp.distl=True: K logits, the support z) with the HL-Gauss loss in place of C51's; `wh` (B,): w / wmax."""

        def loss_and_grads(self, idx=None, draw=None, generator=None, wh=None):
            obs, act, rew, nobs, done = self.ring.gather(idx)
            if self.hp.obs_norm:
                obs = ref.normalize_ref(obs, self.norm); nobs = ref.normalize_ref(nobs, self.norm)
            loss = _hl_step_loss(self, ref, obs, act, rew, nobs, done, draw, wh, sigma)
            return loss, torch.autograd.grad(loss, [*self.q1, *self.q2])

    return HLGaussVLearnerRef(O, A, hp, cap, q1, q2)


def make_ddpg_ref(O, A, hp, cap, actor, q1, q2, sigma=SIGMA):
    ref = _oracle()

    class HLGaussDDPGRef(ref.DDPGRef):
        def update_once(self, idx, draw, wh=None):
            hp = self.hp
            z = torch.linspace(hp.v_min, hp.v_max, hp.num_atoms)
            obs, act, rew, nobs, done = self.ring.gather(idx)
            if hp.obs_norm:
                obs = ref.normalize_ref(obs, self.norm, clamp=False); nobs = ref.normalize_ref(nobs, self.norm, clamp=False)
            closs = _hl_step_loss(self, ref, obs, act, rew, nobs, done, draw, wh, sigma)
            cp = [*self.q1, *self.q2]
            self.copt.apply(list(torch.autograd.grad(closs, cp)), hp.max_grad_norm)
            frozen1 = [p.detach() for p in self.q1]; frozen2 = [p.detach() for p in self.q2]
            aloss = -ref.qmin_ref(frozen1, frozen2, obs, ref.actor_forward_ref(self.actor, obs), z).mean()
            self.aopt.apply(list(torch.autograd.grad(aloss, self.actor)), hp.max_grad_norm)
            ref.polyak_ref([*self.t1, *self.t2], [p.detach() for p in cp], hp.tau)
            return float(closs.detach()), float(aloss.detach())

    return HLGaussDDPGRef(O, A, hp, cap, actor, q1, q2)


# ------------------------------------------------------------------------------------------------ the learner tests' toy shape
O, A, B, STEPS, HID, CAP = 8, 2, 64, 4, (64, 64), 1024
HL = ("algo.distl=True", "algo.distl_loss=hl_gauss")


def learner_cfg(K, *extra, graph=False, memory=CAP, algo="pql_algo", distl=True):
    from pql_amd.utils.cfg import load_cfg
    base = [f"algo={algo}", "task.name=Toy", f"algo.batch_size={B}", f"algo.memory_size={memory}", f"algo.num_atoms={K}"]
    if distl:
        base.append("algo.distl=True")
    if algo == "pql_algo":
        base += ["algo.v_learner_gpu=0", "algo.p_learner_gpu=0", "algo.num_gpus=1", f"algo.prefetch_steps={STEPS}", f"algo.graph={graph}"]
    else:
        base += ["num_envs=64", "device=cuda:0", "sim_device=cuda:0"]
    cfg = load_cfg(base + list(extra))
    cfg.algo.hidden_layers = list(HID)
    return cfg
