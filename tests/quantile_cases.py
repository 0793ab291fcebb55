"""The quantile-regression critic's laws (include/pqlk.h, "Quantile-regression twin critic") as float64 references written from
the prose, the inputs the kernel tests run on, the error bounds those tests hold the kernels to, and CPU autograd learners for the
learner tests.  Nothing here runs on a GPU; tests/test_quantile_cpu.py checks the references against torch.autograd.

u = 2^-24 below is the unit roundoff of fp32 round-to-nearest: fl(x op y) = (x op y)(1 + e), |e| <= u.
"""
import functools

import numpy as np
import torch

import detdata as dd
import learner_harness as lh
from support import T

U = 2.0 ** -24
SLOP = 1.0 + 1e-3   # covers the second-order terms (products of two roundings, each <= u ~ 6e-8) dropped in the bounds below


def f32(x):
    """The fp32 value a C float argument takes."""
    return float(np.float32(x))


def taus(N):
    return (2.0 * np.arange(N) + 1.0) / (2.0 * N)


# ------------------------------------------------------------------------------------------------ the laws, float64
def qr_huber_ref(theta, theta_t, rew, done, gamma_n, kappa, w=None, wmax=None, force_net=None):
    """theta, theta_t: (2, B, N); rew, done, w: (B,); wmax: (1,).  -> dict: loss, dy (2, B, N), istar (B,), T (B, N), abs_td (B,),
    and the pieces the bounds need.  force_net: an int array (B,) to take as i* instead of the law's choice."""
    th, tt = np.asarray(theta, np.float64), np.asarray(theta_t, np.float64)
    r, d = np.asarray(rew, np.float64), np.asarray(done, np.float64)
    g, kap = f32(gamma_n), f32(kappa)
    _, B, N = th.shape
    S = tt.sum(axis=2)                                            # S_i
    istar = (S[1] < S[0]).astype(np.int64) if force_net is None else np.asarray(force_net, np.int64)   # a tie takes net 0
    tsel = np.where(istar[:, None] == 1, tt[1], tt[0])            # (B, N)
    m = (1.0 - d) * g
    T = r[:, None] + m[:, None] * tsel                            # T_k
    u = T[None, :, None, :] - th[:, :, :, None]                   # u_ijk: (2, B, j, k)
    wgt = np.abs(taus(N)[None, None, :, None] - (u < 0))
    a = np.abs(u)
    H = np.where(a <= kap, 0.5 * u * u, kap * (a - 0.5 * kap))
    c = np.clip(u, -kap, kap)
    wh = np.ones(B) if w is None else np.asarray(w, np.float64) / float(np.asarray(wmax, np.float64).reshape(-1)[0])
    rho_row = (wgt * H).sum(axis=(2, 3)) / kap                    # (2, B): sum over j, k of rho
    loss = float((rho_row * wh[None]).sum() / (B * N))
    p = wgt * c                                                   # the gradient's k terms
    dy = -(wh[None, :, None] / (B * N)) * p.sum(axis=3) / kap
    abs_td = np.abs(T.mean(axis=1)[None] - th.mean(axis=2)).max(axis=0)
    return dict(loss=loss, dy=dy, istar=istar, T=T, S=S, abs_td=abs_td, u=u, wgt=wgt, c=c, p=p, wh=wh, m=m, tsel=tsel, r=r, th=th,
                B=B, N=N, kappa=kap)


def dpg_quantile_ref(theta):
    """theta (2, B, N) -> dict: loss, dy (2, B, N), share (2, B), Q (2, B)."""
    th = np.asarray(theta, np.float64)
    _, B, N = th.shape
    Q = th.sum(axis=2) * (1.0 / N)
    share = np.where(Q[0] == Q[1], 0.5, np.stack([Q[0] < Q[1], Q[1] < Q[0]]).astype(np.float64))
    loss = float(-(1.0 / B) * np.minimum(Q[0], Q[1]).sum())
    dy = np.broadcast_to((-share / (B * N))[:, :, None], th.shape).copy()
    return dict(loss=loss, dy=dy, share=share, Q=Q, th=th, B=B, N=N)


# ------------------------------------------------------------------------------------------------ the laws, torch (autograd)
def qr_huber_torch(theta, theta_t, rew, done, gamma_n, kappa, wh=None):
    """The loss of the law as one differentiable torch expression in theta's dtype (theta_t, rew, done carry no gradient)."""
    N = theta.shape[2]
    S = theta_t.sum(dim=2)
    tsel = torch.where((S[1] < S[0])[:, None], theta_t[1], theta_t[0])
    T = rew[:, None] + ((1.0 - done) * gamma_n)[:, None] * tsel
    u = T[None, :, None, :] - theta[:, :, :, None]
    tau = ((2.0 * torch.arange(N, dtype=theta.dtype) + 1.0) / (2.0 * N))[None, None, :, None]
    a = u.abs()
    H = torch.where(a <= kappa, 0.5 * u * u, kappa * (a - 0.5 * kappa))
    rho = (tau - (u.detach() < 0).to(theta.dtype)).abs() * H / kappa
    row = rho.sum(dim=(2, 3))
    if wh is not None:
        row = row * wh[None]
    return row.sum() / (theta.shape[1] * N)


def dpg_quantile_torch(theta):
    return -torch.min(theta[0].mean(dim=1), theta[1].mean(dim=1)).mean()


# ------------------------------------------------------------------------------------------------ inputs
def _margin_ok(a0, a1):
    return np.abs(a1 - a0) >= 1e-3 * (np.abs(a0) + np.abs(a1) + 1.0)


def normal_case(B, N, seed, per=False):
    """Random normal heads, rewards and done flags (fp32), with every row's S_0 / S_1 (target heads) and Q_0 / Q_1 (current heads)
    apart by the margin the tests assert: a row that falls short gets net 1 shifted by 0.25 until it does not."""
    rng = np.random.default_rng(seed)
    theta = rng.standard_normal((2, B, N)).astype(np.float32)
    theta_t = rng.standard_normal((2, B, N)).astype(np.float32)
    for arr in (theta, theta_t):
        for _ in range(64):
            s = arr.astype(np.float64).sum(axis=2)
            bad = ~_margin_ok(s[0], s[1]) | ~_margin_ok(s[0] / N, s[1] / N)
            if not bad.any():
                break
            arr[1, bad] += np.float32(0.25)
    out = dict(theta=theta, theta_t=theta_t, rew=rng.standard_normal(B).astype(np.float32),
               done=(rng.random(B) < 0.25).astype(np.float32))
    if per:
        out["w"] = rng.uniform(0.05, 1.0, B).astype(np.float32)
        out["wmax"] = np.array([out["w"].max()], np.float32)
    return out


def margins_hold(theta):
    s = np.asarray(theta, np.float64).sum(axis=2)
    return bool(_margin_ok(s[0], s[1]).all() and _margin_ok(s[0] / theta.shape[2], s[1] / theta.shape[2]).all())


DYADIC_GAMMA, DYADIC_KAPPA = 0.5, 1.0


def dyadic_case(B, N, seed):
    """B, N powers of two; theta, theta_t and r multiples of 2^-4 in [-1.5, 1.5]: with gamma_n = 0.5 and kappa = 1 every T_k and
    u_ijk is a multiple of 2^-5 below 4, every weight a multiple of 1 / (2 N), every k term of dy a multiple of 2^-6 / N of size
    <= 1 and every partial sum of at most N <= 64 of them below 64: at most 19 significant bits, exact in fp32.  1 / (B N) is a
    power of two.  Rows 0 ... 3 are ties of S_0 and S_1 between target heads that differ (net 1 = net 0 with 1 moved from quantile 1 to quantile 0); rows 4 ... 7
    have S_1 below S_0 by exactly 2^-4 (net 1 = net 0 with one quantile lowered); in rows 8 ... 11 the CURRENT heads tie in
    the same way (Q_0 == Q_1), in rows 12 ... 15 Q_1 is below Q_0 by 2^-4 / N."""
    assert B >= 16 and B & (B - 1) == 0 and N & (N - 1) == 0
    rng = np.random.default_rng(seed)
    q = lambda shape: (rng.integers(-24, 25, shape) / 16.0).astype(np.float32)   # noqa: E731
    theta, theta_t, rew = q((2, B, N)), q((2, B, N)), q((B,))
    done = (rng.random(B) < 0.25).astype(np.float32)
    done[:8] = 0.0   # (a terminal row's targets do not depend on the net)
    for arr, base in ((theta_t, 0), (theta, 8)):
        for row in range(base, base + 4):
            arr[0, row, 0], arr[0, row, 1] = np.float32(0.25), np.float32(0.0)
            arr[1, row] = arr[0, row]
            arr[1, row, 0], arr[1, row, 1] = np.float32(1.25), np.float32(-1.0)   # (the same sum from other values: no permutation)
        for row in range(base + 4, base + 8):
            arr[0, row, 1] = np.float32(0.5)
            arr[1, row] = arr[0, row]
            arr[1, row, 1] = np.float32(0.5 - 1.0 / 16.0)
    return dict(theta=theta, theta_t=theta_t, rew=rew, done=done)


def survives_fp32(x):
    x = np.asarray(x, np.float64)
    return bool((x.astype(np.float32).astype(np.float64) == x).all())


# ------------------------------------------------------------------------------------------------ bounds
def loss_chain(B, N, blocks):
    """Adds on the longest path from one rho term to the loss, from the reduction order documented in pql_amd/csrc/loss.hip:
    N (the k chain of a lane and net) + 1 (the two nets) + ceil(B / (4 blocks)) (the wave's row loop) + 6 + 2 (block_sum_256: the
    butterfly, then (w0 + w1) + (w2 + w3)) + ceil(blocks / 256) + 6 + 2 (the fold of the partials: strided per-thread sums, then the
    same block sum)."""
    return N + 1 + -(-B // (4 * blocks)) + 8 + -(-blocks // 256) + 8


def qr_bounds(ref, blocks):
    """-> (dy_bound (2, B, N) absolute, loss_bound relative, abs_td_bound (B,) absolute) for qr_huber_ref's output `ref`.

    T_k.  The kernel forms fl(r + fl(fl((1 - d) gamma_n) theta_t)): three roundings, so |dT_k| <= u (3 |m theta_t| + |r|), m = (1 - d)
    gamma_n.  u_ijk = fl(T_k - theta_j) adds one: |du| <= dT_k + u |u_ijk|.
    dy.  A k term is wgt * clamp(u).  clamp is 1-Lipschitz, so the term moves by at most wgt |du| <= |du|; where the sign of u
    differs between fp32 and float64, |u| <= |du| on both sides and the term moves by at most |du| as well.  wgt itself carries two
    roundings (tau's division, tau - 1) and the product one: 3 u |clamp(u)|.  The N terms are added in sequence: the classic
    (N - 1) u sum |terms|.  Then one division by kappa, 1 / (B N) (a product, a division) and its product, the weight w / wmax
    and its product: six roundings of the result.
    loss.  All rho terms are >= 0, so a sum of them along a chain of `a` adds has relative error <= a u; each term carries
    12 roundings of its own (wgt 2, H at most 3, wgt H 1, / kappa 1, wh 2, the scale 3) and the error of u_ijk, which enters through
    H with slope |clamp(u)| <= |c| + |du|: that part is sum wgt |c| |du| / (kappa B N) in absolute terms, turned into a count of
    roundings by dividing it by u * loss.  The count (chain + 12 + that) is returned times u.
    abs_td.  A mean is a butterfly (6 adds deep) times fl(1 / N): mean_k T_k errs by (sum dT_k + 6 u sum |T_k|) / N + 2 u |mean|, a
    head's mean by 6 u sum |theta_j| / N + 2 u |mean|, their difference by one more rounding; max does not amplify."""
    B, N, kap = ref["B"], ref["N"], ref["kappa"]
    dT = U * (3.0 * np.abs(ref["m"][:, None] * ref["tsel"]) + np.abs(ref["r"])[:, None])        # (B, k)
    du = dT[None, :, None, :] + U * np.abs(ref["u"])                                              # (2, B, j, k)
    absc, absp = np.abs(ref["c"]), np.abs(ref["p"])
    scale = ref["wh"][None, :, None] / (B * N * kap)
    dy_bound = SLOP * (scale * ((du + 3.0 * U * absc).sum(axis=3) + (N - 1) * U * absp.sum(axis=3)) + 6.0 * U * np.abs(ref["dy"]))
    amp = float(((ref["wgt"] * absc * du).sum(axis=(2, 3)) * ref["wh"][None]).sum() / (kap * B * N)) / (U * ref["loss"])
    loss_bound = SLOP * (loss_chain(B, N, blocks) + 12 + amp) * U
    mT, mth = ref["T"].mean(axis=1), ref["th"].mean(axis=2)
    e_T = (dT.sum(axis=1) + 6.0 * U * np.abs(ref["T"]).sum(axis=1)) / N + 2.0 * U * np.abs(mT)
    e_th = 6.0 * U * np.abs(ref["th"]).sum(axis=2) / N + 2.0 * U * np.abs(mth)
    abs_td_bound = SLOP * (e_T[None] + e_th + U * np.abs(mT[None] - mth)).max(axis=0)
    return dy_bound, loss_bound, abs_td_bound


def dpg_loss_bound(ref, blocks):
    """Absolute bound on the DPG loss.  Q_i = butterfly sum (6 adds deep) times fl(1 / N): |dQ| <= 6 u sum_j |theta| / N + 2 u |Q|;
    min does not amplify.  The row minima are added along ceil(B / (4 blocks)) + 8 + ceil(blocks / 256) + 8 adds and scaled by
    fl(-1 / B) (two roundings): that many roundings of sum |min Q| / B."""
    B, N = ref["B"], ref["N"]
    dQ = (6.0 * U * np.abs(ref["th"]).sum(axis=2) / N + 2.0 * U * np.abs(ref["Q"])).max(axis=0)
    chain = -(-B // (4 * blocks)) + 8 + -(-blocks // 256) + 8 + 2
    return SLOP * float(dQ.sum() / B + chain * U * np.abs(np.minimum(ref["Q"][0], ref["Q"][1])).sum() / B)


# ------------------------------------------------------------------------------------------------ CPU autograd learners
def _oracle():
    from oracle import pql_ref_cpu as ref
    return ref


def make_v_ref(O, A, hp, cap, q1, q2, kappa=1.0):
    ref = _oracle()

    class QuantileVLearnerRef(ref.VLearnerRef):
        """VLearnerRef with the quantile Huber loss in place of the twin MSE; `wh` (B,): importance weights w / wmax."""

        def loss_and_grads(self, idx=None, draw=None, generator=None, wh=None):
            hp = self.hp
            obs, act, rew, nobs, done = self.ring.gather(idx)
            if hp.obs_norm:
                obs = ref.normalize_ref(obs, self.norm); nobs = ref.normalize_ref(nobs, self.norm)
            gn = hp.gamma ** hp.nstep
            with torch.no_grad():
                na = ref.target_noise_ref(ref.actor_forward_ref(self.actor, nobs), draw, hp.tgt_pol_std, hp.tgt_pol_noise_bound)
                theta_t = torch.stack(ref.twin_forward_ref(self.t1, self.t2, nobs, na))
            theta = torch.stack(ref.twin_forward_ref(self.q1, self.q2, obs, act))
            loss = qr_huber_torch(theta, theta_t, rew.reshape(-1), done.reshape(-1), gn, kappa, wh)
            with torch.no_grad():   # the row's new priority
                S = theta_t.sum(dim=2)
                tsel = torch.where((S[1] < S[0])[:, None], theta_t[1], theta_t[0])
                T = rew.reshape(-1, 1) + ((1.0 - done.reshape(-1, 1)) * gn) * tsel
                self.abs_td = (T.mean(dim=1)[None] - theta.mean(dim=2)).abs().max(dim=0).values
            return loss, torch.autograd.grad(loss, [*self.q1, *self.q2])

    return QuantileVLearnerRef(O, A, hp, cap, q1, q2)


def make_p_ref(O, A, hp, cap, actor):
    ref = _oracle()

    class QuantilePLearnerRef(ref.PLearnerRef):
        def learn(self, idx=None, generator=None):
            hp = self.hp
            obs = self.ring.gather(idx)
            if hp.obs_norm:
                obs = ref.normalize_ref(obs, self.norm)
            a = ref.actor_forward_ref(self.actor, obs)
            loss = dpg_quantile_torch(torch.stack(ref.twin_forward_ref(self.q1, self.q2, obs, a)))
            self.opt.apply(list(torch.autograd.grad(loss, self.actor)), hp.max_grad_norm)
            self.update_count += 1
            return float(loss.detach())

    return QuantilePLearnerRef(O, A, hp, cap, actor)


def make_ddpg_ref(O, A, hp, cap, actor, q1, q2, kappa=1.0):
    ref = _oracle()

    class QuantileDDPGRef(ref.DDPGRef):
        def update_once(self, idx, draw, wh=None):
            hp = self.hp
            obs, act, rew, nobs, done = self.ring.gather(idx)
            if hp.obs_norm:
                obs = ref.normalize_ref(obs, self.norm, clamp=False); nobs = ref.normalize_ref(nobs, self.norm, clamp=False)
            gn = hp.gamma ** hp.nstep
            with torch.no_grad():
                na = ref.target_noise_ref(ref.actor_forward_ref(self.actor, nobs), draw, hp.tgt_pol_std, hp.tgt_pol_noise_bound)
                theta_t = torch.stack(ref.twin_forward_ref(self.t1, self.t2, nobs, na))
            theta = torch.stack(ref.twin_forward_ref(self.q1, self.q2, obs, act))
            closs = qr_huber_torch(theta, theta_t, rew.reshape(-1), done.reshape(-1), gn, kappa, wh)
            with torch.no_grad():
                S = theta_t.sum(dim=2)
                tsel = torch.where((S[1] < S[0])[:, None], theta_t[1], theta_t[0])
                T = rew.reshape(-1, 1) + ((1.0 - done.reshape(-1, 1)) * gn) * tsel
                self.abs_td = (T.mean(dim=1)[None] - theta.mean(dim=2)).abs().max(dim=0).values
            cp = [*self.q1, *self.q2]
            self.copt.apply(list(torch.autograd.grad(closs, cp)), hp.max_grad_norm)
            frozen1 = [p.detach() for p in self.q1]; frozen2 = [p.detach() for p in self.q2]
            aloss = dpg_quantile_torch(torch.stack(ref.twin_forward_ref(frozen1, frozen2, obs, ref.actor_forward_ref(self.actor, obs))))
            self.aopt.apply(list(torch.autograd.grad(aloss, self.actor)), hp.max_grad_norm)
            ref.polyak_ref([*self.t1, *self.t2], [p.detach() for p in cp], hp.tau)
            return float(closs.detach()), float(aloss.detach())

    return QuantileDDPGRef(O, A, hp, cap, actor, q1, q2)


# ------------------------------------------------------------------------------------------------ the fold of the partials, fp32
def fold_ref(parts, scale):
    """What one block of 256 threads makes of the per-block partials (k_sum_partials, and the optimiser launch that folds them): thread
    t adds parts[t], parts[t + 256], ... in sequence from 0, each wave of 64 runs the xor butterfly (offsets 32 ... 1), then
    ((w0 + w1) + (w2 + w3)) * scale -- all in fp32."""
    parts = np.asarray(parts, np.float32)
    s = np.zeros(256, np.float32)
    for i in range(0, len(parts), 256):
        chunk = parts[i: i + 256]
        s[: len(chunk)] = s[: len(chunk)] + chunk
    v = s.reshape(4, 64)
    lanes = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[:, lanes ^ o]
    w = v[:, 0]
    return np.float32(np.float32(np.float32(w[0] + w[1]) + np.float32(w[2] + w[3])) * np.float32(scale))


# ------------------------------------------------------------------------------------------------ shared by the kernel tests
def _heads(dev, a, ld):
    """(2, B, N) -> a device (2, B, ld) block whose pad columns hold NaN: a kernel that read them would show it."""
    _, B, N = a.shape
    t = torch.full((2, B, ld), float("nan"), dtype=torch.float32, device=dev)
    t[:, :, :N] = T(a).to(dev)
    return t


def _check_buffers(got, per=False):
    assert got["intact"], "a guard word behind dy, scratch or abs_td was overwritten"
    assert (got["pad"] == 0).all(), "pad columns of dy must be written as zero"
    assert np.isfinite(got["dy"]).all() and np.isfinite(got["parts"]).all()
    assert np.isfinite(got["abs_td"]).all() if per else np.isnan(got["abs_td"]).all()   # the plain instance never touches abs_td


# ------------------------------------------------------------------------------------------------ the learner tests' toy shape
O, A, B, K, HID = 8, 2, 256, 4, (64, 64)
QR = "algo.cri_class=QuantileDoubleQ"


def _cfg(N, *extra, graph=False, memory=4096, algo="pql_algo"):
    from pql_amd.utils.cfg import load_cfg
    base = [f"algo={algo}", "task.name=Toy", f"algo.batch_size={B}", f"algo.memory_size={memory}", QR, f"algo.num_quantiles={N}"]
    if algo == "pql_algo":
        base += ["algo.v_learner_gpu=0", "algo.p_learner_gpu=0", "algo.num_gpus=1", f"algo.prefetch_steps={K}", f"algo.graph={graph}"]
    else:
        base += ["num_envs=64", "device=cuda:0", "sim_device=cuda:0"]
    cfg = load_cfg(base + list(extra))
    cfg.algo.hidden_layers = list(HID)
    return cfg


def _weights(N):
    return dd.doubleq_state(O, A, N, 21 + N, HID), dd.mlp_state(O, A, 11, HID)


_fill = functools.partial(lh._fill, O, A, rew=0.5)
_rows = functools.partial(lh._rows, O, A)
_run = functools.partial(lh._run, n=K)


def _learner(N, *extra, graph, cap=4096, rows=1500, seed=11):
    return lh._learner(lambda: _cfg(N, *extra, graph=graph, memory=cap), O, A, rows, seed)
