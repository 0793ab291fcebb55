"""`CriticHead`: THE place where a critic's head is told apart -- what its output columns mean (scalar | categorical | quantile),
how wide it is, which loss entry of include/pqlk.h a critic step and an actor step take on it and with which arguments, and what
divides its loss.  The learners and the baseline agents hold one and ask it; a new head is taught to this file (and to its kernels).
Every entry is looked up as `L.lib.<name>` when it is called: tests spy on those attributes.
"""
from __future__ import annotations

from pql_amd import _lib as L
from pql_amd.algo.learner import LOSS_RING, distl_loss, f32_recip, hl_sigma, qr_drop, qr_targets


class CriticHead:
    def __init__(self, critic, algo):
        """critic: anything with `head` (absent: scalar -- the LayerNorm and BatchNorm critics) and `num_atoms` + `z_atoms` or
        `num_quantiles`; algo: `cfg.algo`, read when a loss is issued (qr_drop, v_min, v_max, distl_loss, hl_sigma)."""
        self.critic, self.algo = critic, algo
        self.kind = getattr(critic, "head", "scalar")
        if self.kind not in ("scalar", "categorical", "quantile"):
            raise ValueError(f"unknown critic head {self.kind!r}")
        # the k of pqlk_loss_parts(B, k)
        self.width = 1 if self.kind == "scalar" else int(critic.num_atoms if self.kind == "categorical" else critic.num_quantiles)

    @property
    def hl_gauss(self):
        """The categorical head is trained with the HL-Gauss law (algo.distl_loss=hl_gauss), not with C51's: read when a loss is issued."""
        return self.kind == "categorical" and distl_loss(self.algo) == "hl_gauss"

    def loss_parts(self, B):
        """Partials a loss launch on this head leaves in its scratch."""
        return L.lib.pqlk_loss_parts(B, self.width)

    def critic_scale(self, B):
        """What the fold multiplies the critic loss's partials by: 1 / B (scalar, HL-Gauss), 1 / (B K) (C51), or 1 / (B * the target atoms a
        row is regressed on)."""
        if self.kind == "scalar" or self.hl_gauss:
            return f32_recip(B)
        return f32_recip(B, qr_targets(self.algo, self.width) if self.kind == "quantile" else self.width)

    def critic_loss(self, q, qt, ld, rew, done, gamma_n, B, dy, loss_out, step, scratch, device, per=None, soft=None, kappa=1.0):
        """The loss of the twin heads q against the target heads qt (both (2, B, ld)): d loss / d q -> dy, the partials -> scratch, the
        loss -> slot `step` of the ring `loss_out` (None: the partials are folded later).  scalar: twin MSE against r + (1 - d) gamma^n
        min(qt); categorical: C51 projection + BCE or, with algo.distl_loss=hl_gauss, the Gaussian histogram of that scalar target over
        the bins + cross-entropy; quantile: the quantile Huber loss (`kappa`) against the target net with the smaller mean
        or, with algo.qr_drop, against the pooled atoms of both target nets without the 2 * qr_drop largest.
        per = (w, wmax, abs_td), prioritized replay: the weights w / wmax lie on the loss and its gradient, |TD| goes to abs_td.
        soft = (logp, log_alpha): every target atom lowered by alpha logp -- the truncated law only."""
        drop = qr_drop(self.algo) if self.kind == "quantile" else None
        if soft is not None and drop is None:
            raise ValueError(f"no soft target on the {self.kind} head without algo.qr_drop: the entropy shift rides in the truncated quantile loss only")
        hl = self.hl_gauss
        if per is not None and self.kind == "categorical" and not hl:
            raise ValueError("no weighted C51 loss: prioritized replay cannot run on the categorical head")
        out = (B, L.ptr(dy), L.ptr(loss_out), L.ptr(step), LOSS_RING)
        if self.kind == "categorical":
            args = (L.ptr(q), L.ptr(qt), ld, self.width, L.ptr(rew), L.ptr(done), L.ptr(self.critic.z_atoms), gamma_n,
                    float(self.algo.v_min), float(self.algo.v_max))
            if not hl:
                L.check(L.lib.pqlk_c51_bce_loss(*args, *out, None, L.ptr(scratch), L.stream(device)))
                return
            # the same head under the HL-Gauss law: sigma in bin widths behind the support's ends, the weights behind scratch
            entry = L.lib.pqlk_hlgauss_ce_loss if per is None else L.lib.pqlk_hlgauss_ce_loss_per
            L.check(entry(*args, hl_sigma(self.algo), *out, None, L.ptr(scratch), *(L.ptr(t) for t in per or ()), L.stream(device)))
            return
        if self.kind == "scalar":
            name, args = "pqlk_td_mse_loss", (L.ptr(q), L.ptr(qt), ld, L.ptr(rew), L.ptr(done), gamma_n)
        else:
            name = "pqlk_qr_huber_loss" if drop is None else "pqlk_tqc_huber_loss" if soft is None else "pqlk_tqc_huber_loss_soft"
            args = (L.ptr(q), L.ptr(qt), ld, self.width, L.ptr(rew), L.ptr(done), gamma_n, float(kappa))
        # behind scratch: the weights, then logp and log_alpha, then drop
        tail = tuple(L.ptr(t) for t in (per or ()) + (soft or ())) + (() if drop is None else (int(drop),))
        L.check(getattr(L.lib, name + ("" if per is None else "_per"))(*args, *out, L.ptr(scratch), *tail, L.stream(device)))

    def actor_loss(self, q, ld, B, dy, loss_out, step, scratch, device, owner=None, mean=False):
        """-mean_b of the heads' Q: d loss / d q -> dy, the value -> the ring as in `critic_loss`.  Q is min(Q1, Q2) -- of a categorical
        head the expectations, of a quantile head the means -- or, mean=True (quantile only), the mean over all atoms of both nets.
        owner (scalar / categorical): the uint8 tensor of the `_owner` entry, which writes into it which net(s) attained a scalar min."""
        if (mean and self.kind != "quantile") or (owner is not None and self.kind == "quantile"):
            raise ValueError(f"the {self.kind} head's actor loss takes no " + ("mean-of-critics objective" if mean else "owner partition"))
        out = (B, L.ptr(dy), L.ptr(loss_out), L.ptr(step), LOSS_RING, L.ptr(scratch))
        if self.kind == "quantile":
            entry = L.lib.pqlk_dpg_loss_quantile_mean if mean else L.lib.pqlk_dpg_loss_quantile
            L.check(entry(L.ptr(q), ld, self.width, *out, L.stream(device)))
        else:
            z = self.critic.z_atoms if self.kind == "categorical" else None
            name, tail = ("pqlk_dpg_loss", ()) if owner is None else ("pqlk_dpg_loss_owner", (L.ptr(owner),))
            L.check(getattr(L.lib, name)(L.ptr(q), ld, self.width, L.ptr(z), *out, *tail, L.stream(device)))
