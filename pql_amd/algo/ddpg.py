"""Synchronous DDPG on the same kernels (BASELINE config #1 plumbing).

Mirrors the hot part of `pql/algo/ddpg.py`: `AgentDDPG.update_net(memory)` = `update_times` x {sample,
obs_rms.normalize (NO clamp, ddpg.py:124-126), critic step (:147-157), actor step (:159-166), Polyak of the critic target and,
with `no_tgt_actor=False`, of the target actor (:134-135; `no_tgt_actor=True`, the shipped default: the target actor IS the actor, :22).  It is the V- and P-learner launch sequences
run back to back on one shared replay sample; the ActorCriticBase plumbing of the fork (bidex, success
trackers) is out of scope.
"""
from __future__ import annotations

import torch

from pql_amd import _lib as L
from pql_amd.algo.ac_base import ActorCriticBase
from pql_amd.models.mlp import mlp_backward_raw, mlp_forward_raw, output_view


class AgentDDPG(ActorCriticBase):
    def _own_tiles(self, ws, zeros, empty):
        super()._own_tiles(ws, zeros, empty)
        ws["draw"], ws["dz_a"] = zeros((ws["B"], self.action_dim)), zeros((1, ws["B"], ws["ld_a"]))

    @torch.no_grad()
    def update_once(self, memory, indices=None, noise=None):
        """One inner iteration of update_net; returns nothing (losses land in device rings)."""
        algo, dev = self.cfg.algo, self.device
        B = int(algo.batch_size)
        ws = self._workspace(B)
        O, A = self.obs_dim[0], self.action_dim
        al, cl = self.actor.layout, self.critic.layout
        with torch.cuda.device(dev):
            self._sample(memory, ws, indices)
            draw = ws["draw"].normal_() if noise is None else noise.to(dev, torch.float32).contiguous()
            # ---- critic step (ddpg.py:147-157)
            mlp_forward_raw(al, self.actor_target.arena.data, ws["xn_obs"], L.ACT_TANH_NOISE, draw, algo.noise.tgt_pol_std,
                            algo.noise.tgt_pol_noise_bound, ws["acts_a"], ws["xn_sa"][:, O:])
            mlp_forward_raw(cl, self.critic_target.arena.data, ws["xn_sa"], L.ACT_NONE, acts=ws["acts_t"])
            mlp_forward_raw(cl, self.critic.arena.data, ws["x_sa"], L.ACT_NONE, acts=ws["acts_c"])
            self._td_mse_loss(ws, output_view(cl, ws["acts_c"], B), output_view(cl, ws["acts_t"], B), cl.ld_out)
            mlp_backward_raw(cl, self.critic.arena.data, ws["x_sa"], ws["acts_c"], ws["dy"], ws["bwd_c"], ws["gc"], ws["splits"])
            self._critic_step(ws)
            # ---- actor step through the UPDATED critic (ddpg.py:159-166)
            mlp_forward_raw(al, self.actor.arena.data, ws["x_obs"], L.ACT_TANH, acts=ws["acts_a"], out2=ws["x_pi"][:, O:])
            mlp_forward_raw(cl, self.critic.arena.data, ws["x_pi"], L.ACT_NONE, acts=ws["acts_c"])
            self._dpg_loss(ws, output_view(cl, ws["acts_c"], B), cl.ld_out)
            # the critic's input gradient, action columns only, through the actor's tanh: the gradient at its pre-activation output
            mlp_backward_raw(cl, self.critic.arena.data, ws["x_pi"], ws["acts_c"], ws["dy"], ws["bwd_c"], dx=ws["dz_a"], dx_col0=O,
                             dx_cols=A, dx_tanh_of=output_view(al, ws["acts_a"], B))
            self._actor_step(ws, ws["dz_a"])
            # ---- soft_update(critic_target, critic, tau) and, with a target actor, of it (ddpg.py:134-135)
            self._update_targets()
