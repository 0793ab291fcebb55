"""Synchronous CrossQ on the PQL kernels.

Mirrors `pql/algo/crossQ.py`: `AgentCrossQ.update_net(memory)` = `update_times` x {sample, `obs_rms.normalize` (no
clamp), `update_critic` (:144-157: ONE joint forward of [obs; next_obs] with [action; target-policy action] through the
BatchNorm critic in training mode -- batch statistics over all 2B rows -- current Q from the first half, the target from the
detached second half, twin MSE), `update_actor` (:159-166: DPG through the critic, which stays in training mode: its
batch statistics are those of the B actor rows and the running statistics move again)}.  There is no target critic and,
with `no_tgt_actor=True` (the default), no target actor either (`False`: a Polyak-averaged copy supplies the target-policy actions).  The critic is `pql_amd.models.batchnorm.DoubleQBatchNorm` (one-layer GEMM
calls + the BatchNorm/ELU kernels of pql_amd/csrc/bn.hip); gather, actor, losses and the optimiser are the launches the
DDPG baseline uses.  RNG order per update: replay indices, then the target-policy noise draw.
"""
from __future__ import annotations

import torch

from pql_amd import _lib as L
from pql_amd.algo.ac_base import ActorCriticBase
from pql_amd.models.mlp import mlp_forward_raw, output_view


class AgentCrossQ(ActorCriticBase):
    TARGET_CRITIC = False

    def _own_state(self):
        extra, opts = super()._own_state()   # stats: BatchNorm running moments
        return dict(extra, critic_stats=self.critic.stats, critic_batches=self.critic.num_batches_tracked), opts

    def _own_tiles(self, ws, zeros, empty):   # (the BatchNorm critic keeps its activations and backward workspace itself)
        B = ws["B"]
        ws["x_all"] = zeros((2 * B, ws["ld_sa"]))          # [obs | action] rows, then [next_obs | target action] rows
        ws["x_sa"], ws["xn_sa"] = ws["x_all"][:B], ws["x_all"][B:]
        for k, shape in dict(draw=(B, self.action_dim), q=(2, B, 32), qt=(2, B, 32), dy=(2, B, 32), dq_all=(2, 2 * B, 32),
                             dz_a=(1, B, ws["ld_a"])).items():
            ws[k] = zeros(shape)

    @torch.no_grad()
    def update_once(self, memory, indices=None, noise=None):
        """One inner iteration of update_net (losses land in device rings).  indices / noise: injected draws for parity tests."""
        algo, dev = self.cfg.algo, self.device
        B = int(algo.batch_size)
        ws = self._workspace(B)
        O, A = self.obs_dim[0], self.action_dim
        al = self.actor.layout
        with torch.cuda.device(dev):
            self._sample(memory, ws, indices)
            draw = ws["draw"].normal_() if noise is None else noise.to(dev, torch.float32).contiguous()
            # ---- critic step (crossQ.py:144-157)
            mlp_forward_raw(al, self.actor_target.arena.data, ws["xn_obs"], L.ACT_TANH_NOISE, draw, algo.noise.tgt_pol_std,
                            algo.noise.tgt_pol_noise_bound, ws["acts_a"], ws["xn_sa"][:, O:])
            q_all = self.critic.forward_raw(ws["x_all"], training=True)          # (2, 2B, 32): batch statistics over all 2B rows
            ws["q"].copy_(q_all[:, :B]); ws["qt"].copy_(q_all[:, B:])            # current / (detached) next halves
            self._td_mse_loss(ws, ws["q"], ws["qt"], 32)
            ws["dq_all"][:, :B].copy_(ws["dy"])                                  # the next-state rows carry no loss gradient
            self.critic.backward_raw(ws["x_all"], ws["dq_all"], grads=ws["gc"])
            self._critic_step(ws)
            # ---- actor step (crossQ.py:159-166): the critic is still in training mode there
            mlp_forward_raw(al, self.actor.arena.data, ws["x_obs"], L.ACT_TANH, acts=ws["acts_a"], out2=ws["x_pi"][:, O:])
            self._dpg_loss(ws, self.critic.forward_raw(ws["x_pi"], training=True), 32)
            dx = self.critic.backward_raw(ws["x_pi"], ws["dy"], grads=None, need_dx=True)
            a_out = output_view(al, ws["acts_a"], B)[0]
            ws["dz_a"][0, :, :A] = dx[:, O:O + A] * (1.0 - a_out[:, :A] * a_out[:, :A])       # through the actor's tanh
            self._actor_step(ws, ws["dz_a"])
            self._update_targets()   # the target actor's Polyak, when there is one (crossQ.py:132-133)
