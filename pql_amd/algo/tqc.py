"""Synchronous TQC (Truncated Quantile Critics, Kuznetsov et al. 2020) on the PQL kernels: the maximum-entropy actor-critic the
truncated quantile critic was designed for.  The reference has no such algorithm; the laws are written out in include/pqlk.h ("TQC as
the paper defines it").

`AgentTQC` is `AgentSAC` -- its squashed-Gaussian policy, its temperature on the device, its RNG order (replay indices, the rsample
draw of the critic step, the rsample draw of the actor step), its workspace, its temperature step, Polyak and checkpoint state -- on
the twin quantile critic, and differs in two launches:

  critic step   the entropy term alpha log pi(a'|s') sits inside every atom of the truncated pooled target.  The shift rides in the loss
                launch (`pqlk_tqc_huber_loss_soft{,_per}`): no `pqlk_sac_entropy_shift` pass over the target heads, so the step has the
                launch count of DDPG's on the same critic;
  actor step    the Q term is the mean over all atoms of both nets (`pqlk_dpg_loss_quantile_mean`), not the smaller of the two heads'
                means: the overestimation control is the truncation, not a min.

Two critic nets (the paper uses five: the arena layout is twin); `algo.qr_drop` atoms dropped per net.
"""
from __future__ import annotations

from pql_amd.algo.sac import AgentSAC


class AgentTQC(AgentSAC):
    # (the refusals -- another cri_class, qr_drop null -- are check_critic_class's, raised by the base class before anything is allocated)

    def _soft_td_loss(self, ws, q, qt, ld):
        """The truncated quantile Huber loss against T_p = r + c (z_p - alpha log pi(a'|s')): d loss / d theta -> ws["dy"], the loss ->
        the critic's ring; prioritized: the importance weights in, |TD| back into the tree."""
        self._td_mse_loss(ws, q, qt, ld, soft=(ws["logp_next"], self.log_alpha))

    def _actor_q_loss(self, ws, q, ld):
        """-mean_b of the mean over all 2 N atoms: d loss / d theta -> ws["dy"], the value -> the actor's ring."""
        self._dpg_loss(ws, q, ld, mean=True)
