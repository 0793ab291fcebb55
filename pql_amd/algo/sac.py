"""Synchronous SAC on the PQL kernels.

Mirrors the hot part of `pql/algo/sac.py`: `AgentSAC.update_net(memory)` = `update_times` x {sample, `obs_rms.normalize`
(no clamp), `update_critic` (:138-146: entropy-regularised n-step target through the squashed-Gaussian policy, twin MSE),
`update_actor` (:148-161: mean(alpha log pi - min Q) through the UPDATED critic, then the temperature step on
`log_alpha`), Polyak on the critic (and on the otherwise unused target policy when `no_tgt_actor=False`)}.  Everything the DDPG baseline already runs (gather,
fp32-MFMA MLP forward/backward, TD loss, clip+AdamW, Polyak) is reused; the new math is four small launches
(`pql_amd/csrc/sac.hip`): the policy head forward / backward and the two temperature kernels.  `log_alpha` lives on the
device and is read there by the kernels that need alpha, so an update has no host round trip and is graph-capturable.
RNG order per update = the reference's: replay indices, the rsample draw of the critic step, the rsample draw of the
actor step.
"""
from __future__ import annotations

import math

import torch

from pql_amd import _lib as L
from pql_amd.algo.ac_base import ActorCriticBase
from pql_amd.algo.learner import LOSS_RING, _AdamState, apply_optimizer
from pql_amd.models.mlp import mlp_forward_raw, output_view


class AgentSAC(ActorCriticBase):
    def __init__(self, env, cfg):
        # (with no_tgt_actor=False the reference keeps a Polyak-averaged copy of the policy, sac.py:19,104-105; its critic target
        # (sac.py:138-146) samples the next action from `self.actor` either way, so the copy is state only: checkpoints)
        super().__init__(env, cfg)
        if self.actor.layout.dims[-1] != 2 * self.action_dim:
            raise ValueError("SAC needs a policy with a [mu | log_std] head (act_class: TanhDiagGaussianMLPPolicy)")
        algo = cfg.algo
        # temperature (sac.py:22-26,32-42): learned log_alpha starting at 0, or a fixed alpha from the config
        self.learn_alpha = algo.alpha is None
        self.log_alpha = torch.full((1,), 0.0 if self.learn_alpha else math.log(float(algo.alpha)), dtype=torch.float32, device=self.device)
        self.alpha_opt = _AdamState(self.log_alpha)
        self.target_entropy = -float(self.action_dim)
        self.alpha_loss = torch.zeros(1, device=self.device)

    # ---- acting ------------------------------------------------------------------------------------
    def get_alpha(self, detach=True, scalar=False):
        alpha = self.log_alpha.exp()
        return float(alpha) if scalar else alpha

    def get_actions(self, obs, sample=True):
        x = self.obs_rms.normalize(obs) if self.cfg.algo.obs_norm else obs
        return self.actor.get_actions(x, sample=sample)

    def _own_state(self):
        extra, opts = super()._own_state()
        return dict(extra, log_alpha=self.log_alpha, alpha_loss=self.alpha_loss), dict(opts, alpha_opt=self.alpha_opt)

    def _extra_log(self):
        return {"train/alpha": self.get_alpha(scalar=True)}

    # ---- learning ----------------------------------------------------------------------------------
    def _own_tiles(self, ws, zeros, empty):
        super()._own_tiles(ws, zeros, empty)
        B, A = ws["B"], self.action_dim
        for k, shape in dict(eps_next=(B, A), eps_cur=(B, A), logp_next=(B,), logp=(B,), dx_pi=(B, ws["ld_sa"]),
                             dy_a=(1, B, self.actor.layout.ld_out), g_alpha=(1,)).items():
            ws[k] = zeros(shape)

    # ---- the two places a maximum-entropy agent on another critic head differs (AgentTQC)
    def _soft_td_loss(self, ws, q, qt, ld):
        """The critic loss against the entropy-regularised target: the target heads lowered in place by alpha log pi(a'|s'), then the
        twin loss of the base class."""
        B = ws["B"]
        L.check(L.lib.pqlk_sac_entropy_shift(L.ptr(qt), ld, B * ld, 2, L.ptr(ws["logp_next"]), L.ptr(self.log_alpha), B, L.stream(self.device)))
        self._td_mse_loss(ws, q, qt, ld)

    def _actor_q_loss(self, ws, q, ld):
        """The Q term of the actor loss, -mean(min Q): d loss / d q -> ws["dy"], the value -> the actor's ring."""
        self._dpg_loss(ws, q, ld)

    @torch.no_grad()
    def update_once(self, memory, indices=None, eps_next=None, eps_cur=None):
        """One inner iteration of update_net (losses land in device rings).  indices / eps_*: injected draws for parity tests."""
        algo, dev = self.cfg.algo, self.device
        B = int(algo.batch_size)
        ws = self._workspace(B)
        O, A = self.obs_dim[0], self.action_dim
        al = self.actor.layout
        with torch.cuda.device(dev):
            st = L.stream(dev)
            self._sample(memory, ws, indices)
            e_next = ws["eps_next"].normal_() if eps_next is None else eps_next.to(dev, torch.float32).contiguous()
            e_cur = ws["eps_cur"].normal_() if eps_cur is None else eps_cur.to(dev, torch.float32).contiguous()
            # ---- critic step (sac.py:138-146): y = r + (1-d) gamma^n (min Q_t(s', a') - alpha log pi(a'|s')), a' ~ pi(.|s')
            mlp_forward_raw(al, self.actor.arena.data, ws["xn_obs"], L.ACT_NONE, acts=ws["acts_a"])
            y_a = output_view(al, ws["acts_a"], B)[0]
            L.check(L.lib.pqlk_sg_head_forward(L.ptr(y_a), al.ld_out, L.ptr(e_next), B, A, L.ptr(ws["xn_sa"][:, O:]), ws["ld_sa"],
                                               L.ptr(ws["logp_next"]), st))
            qt, _ = self._critic_forward(ws, self.critic_target, ws["xn_sa"], "t")
            q, ld = self._critic_forward(ws, self.critic, ws["x_sa"], "c")
            self._soft_td_loss(ws, q, qt, ld)
            self._critic_grads(ws, ws["x_sa"])
            self._critic_step(ws)
            # ---- actor step through the UPDATED critic (sac.py:148-153): L = mean(alpha log pi(a|s) - min Q(s, a)), a ~ pi(.|s)
            mlp_forward_raw(al, self.actor.arena.data, ws["x_obs"], L.ACT_NONE, acts=ws["acts_a"])
            L.check(L.lib.pqlk_sg_head_forward(L.ptr(y_a), al.ld_out, L.ptr(e_cur), B, A, L.ptr(ws["x_pi"][:, O:]), ws["ld_sa"],
                                               L.ptr(ws["logp"]), st))
            self._actor_q_loss(ws, *self._critic_forward(ws, self.critic, ws["x_pi"], "c"))
            # temperature terms with the alpha the actor loss uses (before its own update): actor loss += alpha mean(log pi),
            # g_alpha = alpha * mean(-log pi - target_entropy)
            L.check(L.lib.pqlk_sac_alpha_terms(L.ptr(ws["logp"]), B, L.ptr(self.log_alpha), self.target_entropy, L.ptr(ws["g_alpha"]),
                                               L.ptr(self.alpha_loss), L.ptr(self.aloss), L.ptr(self.aopt.step), LOSS_RING, st))
            # dL/da = -(1/B) d minQ / da : the critic's input gradient, action columns [O, O+A) of dx_pi
            self._critic_dx(ws, ws["x_pi"], ws["dx_pi"])
            L.check(L.lib.pqlk_sg_head_backward(L.ptr(y_a), al.ld_out, L.ptr(e_cur), L.ptr(ws["x_pi"][:, O:]), ws["ld_sa"],
                                                L.ptr(ws["dx_pi"][:, O:]), ws["ld_sa"], L.ptr(self.log_alpha), 1.0 / B, B, A,
                                                L.ptr(ws["dy_a"]), st))
            self._actor_step(ws, ws["dy_a"])
            if self.learn_alpha:   # sac.py:155-157: AdamW (torch defaults, incl. weight decay) on the single scalar, clipped like the rest
                apply_optimizer(self.log_alpha, ws["g_alpha"], self.alpha_opt, None, algo.alpha_lr, algo.max_grad_norm, 0.0, 1.0, dev)
            # ---- soft_update(critic_target, critic, tau) and, with a target policy, of it (sac.py:104-105)
            self._update_targets()
