"""`ActorCriticBase`: what the synchronous replay baselines (DDPG, SAC, CrossQ) share -- the counterpart of the reference's
`pql/algo/ac_base.py`.  The nets, their optimiser moments and loss rings, the checkpoint state, the rollout, the workspace, the
replay sample and the launch blocks every one of them runs (TD-MSE loss, DPG loss, optimiser steps, Polyak).  An agent keeps its
`update_once`: the algorithm, in the order of the reference's lines.
"""
from __future__ import annotations

import ctypes as C
from copy import deepcopy

import numpy as np
import torch

from pql_amd import _lib as L
from pql_amd.algo.heads import CriticHead
from pql_amd.algo.critics import check_critic_class, make_critic
from pql_amd.algo.diag import CriticProbe, diag_cfg
from pql_amd.algo.learner import LOSS_RING, _AdamState, apply_optimizer, check_per_refresh, make_actor
from pql_amd.algo.pql_actor import PQLActor
from pql_amd.models.mlp import default_splits, mlp_backward_raw, mlp_forward_raw, output_view
from pql_amd.replay.prioritized_replay import per_beta, per_cfg  # noqa: F401  (per_beta: imported from here by its users)
from pql_amd.replay.simple_replay import cfg_obs_dtype


class ActorCriticBase(PQLActor):
    TARGET_CRITIC = True   # False (CrossQ): the agent has no `critic_target` attribute at all

    def __init__(self, env, cfg):
        check_critic_class(cfg, agent=True)   # before anything is allocated
        check_per_refresh(cfg, f"algo={cfg.algo.name}")
        diag = diag_cfg(cfg)   # algo.diag.enabled=True is refused here for every agent but DDPG
        cfg.algo.v_learner_gpu = cfg.algo.get("v_learner_gpu", 0) or 0
        cfg.algo.p_learner_gpu = cfg.algo.get("p_learner_gpu", 0) or 0
        super().__init__(env, cfg)
        self.device = self.sim_device
        algo = cfg.algo
        self.replay_obs_dtype = cfg_obs_dtype(algo)   # algo.replay_obs_dtype: storage format of the replay ring built for this agent
        self.actor = make_actor(cfg, self.obs_dim, self.action_dim, self.device)   # actor first: both consume the CPU generator
        self.critic = make_critic(cfg, self.obs_dim, self.action_dim, self.device)
        self.head = CriticHead(self.critic, algo)   # which loss entries the critic's output columns take
        if self.TARGET_CRITIC:
            self.critic_target = deepcopy(self.critic)
        # a Polyak-averaged copy of the actor, or (no_tgt_actor=True, every shipped config) the actor itself
        self.actor_target = self.actor if algo.no_tgt_actor else deepcopy(self.actor)
        self.aopt, self.copt = _AdamState(self.actor.arena.data), _AdamState(self.critic.arena.data)
        self.closs = torch.zeros(LOSS_RING, device=self.device)
        self.aloss = torch.zeros(LOSS_RING, device=self.device)
        self._ws = None
        self.per = per_cfg(algo)   # algo.per when prioritized replay is on (None: every launch below is the plain one)
        self.per_calls = 0         # calls of update_net so far: the position on the beta schedule (host side, saved)
        # algo.diag.enabled: the probe at the end of `update_net` (pql_amd/algo/diag.py); None = off
        self._diag = None if diag is None else CriticProbe(self.head, *diag, len(self._elu_layers()), self.device)

    # ---- training state ----------------------------------------------------------------------------
    def _own_state(self):
        """(extra named tensors, {name: _AdamState}) of this agent's checkpoint; a subclass extends either."""
        return {}, {"aopt": self.aopt, "copt": self.copt}

    def _state_tensors(self):
        out = super()._state_tensors()   # (the policy itself is the base class's "actor")
        out.update(critic=self.critic.arena.data, closs=self.closs, aloss=self.aloss)
        if self.TARGET_CRITIC:
            out["critic_target"] = self.critic_target.arena.data
        if self.actor_target is not self.actor:
            out["actor_target"] = self.actor_target.arena.data
        extra, opts = self._own_state()
        out.update(extra)
        for name, opt in opts.items():
            out.update({f"{name}.m": opt.m, f"{name}.v": opt.v, f"{name}.step": opt.step})
        return out

    def training_state(self):
        st = super().training_state()
        if self.per is not None:
            st["per_calls"] = int(self.per_calls)
        for name, net in self._drop_nets().items():   # the dropout critic's mask state: seed, call counter, stream id
            st.setdefault("drop", {})[name] = net.drop_state()
        return st

    def load_training_state(self, st, nstep=True):
        super().load_training_state(st, nstep=nstep)
        if self.per is not None:
            self.per_calls = int(st.get("per_calls", 0))
        for name, net in self._drop_nets().items():
            net.load_drop_state(st["drop"][name])

    def _drop_nets(self):
        """The critics that carry dropout state (DoubleQDropoutLayerNorm: the critic and its target), by their training-state name."""
        nets = {"critic": self.critic, **({"critic_target": self.critic_target} if self.TARGET_CRITIC else {})}
        return {k: v for k, v in nets.items() if hasattr(v, "drop_state")}

    def explore_env(self, env, timesteps, random=False):
        _, cri_data, steps = super().explore_env(env, timesteps, random)
        return cri_data, steps

    def beta(self):
        return per_beta(self.per.beta0, int(self.per.beta_iters), self.per_calls) if self.per is not None else 1.0

    # ---- learning ----------------------------------------------------------------------------------
    def _own_tiles(self, ws, zeros, empty):
        """The agent's tiles, put into `ws` before the common ones (a common name set here is kept: CrossQ's x_sa / xn_sa).
        Here: what a critic that is one MLP arena needs (a critic with `forward_raw` / `backward_raw` keeps its activations and its
        backward workspace itself)."""
        B = ws["B"]
        if not self._one_layout:
            ws["dy"] = zeros((2, B, 32))
            return
        cl = self.critic.layout
        ws["dy"] = zeros((2, B, cl.ld_out))
        ws["acts_t"], ws["acts_c"] = empty(cl.acts_floats(B)), empty(cl.acts_floats(B))
        ws["bwd_c"] = empty(cl.bwd_ws_floats(B, ws["splits"]))

    def _workspace(self, B):
        if self._ws is not None and self._ws["B"] == B:
            return self._ws
        f = dict(dtype=torch.float32, device=self.device)
        O, A = self.obs_dim[0], self.action_dim
        al = self.actor.layout
        ws = dict(B=B, ld_sa=L.ld(O + A), ld_o=L.ld(O), ld_a=L.ld(A), splits=default_splits(B))
        self._own_tiles(ws, lambda shape: torch.zeros(shape, **f), lambda n: torch.empty(n, **f))
        # zeroed: nothing writes the pad columns afterwards, and the GEMMs read them
        for k, shape in dict(x_sa=(B, ws["ld_sa"]), xn_sa=(B, ws["ld_sa"]), xn_obs=(B, ws["ld_o"]), x_obs=(B, ws["ld_o"]),
                             x_pi=(B, ws["ld_sa"]), rew=(B,), done=(B,), gc=(self.critic.arena.numel(),), ga=(al.total,),
                             scratch=(2048,)).items():
            if k not in ws:
                ws[k] = torch.zeros(shape, **f)
        ws["acts_a"] = torch.empty(al.acts_floats(B), **f)
        ws["bwd_a"] = torch.empty(al.bwd_ws_floats(B, ws["splits"]), **f)
        self._ws = ws
        return ws

    def _sample(self, memory, ws, indices=None):
        """Draw (or take) B replay indices and gather: [obs | action] -> x_sa, normalised next obs -> xn_sa / xn_obs, reward, done;
        obs_rms.normalize WITHOUT clamp.  x_obs (= norm(obs), the actor-step input) and x_pi's observation columns are copies."""
        B, O = ws["B"], self.obs_dim[0]
        ws["per"] = memory if getattr(memory, "prioritized", False) else None
        if ws["per"] is not None:   # the weights at this call's beta ride with the indices: drawn with them, or computed for injected ones
            memory.beta = self.beta()
        idx = memory.draw_indices(B) if indices is None else indices.to(self.device, torch.int64).contiguous()
        if ws["per"] is not None:
            ws["w"], ws["wmax"] = (memory.w, memory.wmax) if indices is None else memory.weights_for(idx)
            ws["idx"] = idx
            if "abs_td" not in ws:
                ws["abs_td"] = torch.zeros(B, dtype=torch.float32, device=self.device)
        mean = var = None
        eps = 0.0
        if self.cfg.algo.obs_norm:
            mean, var, eps = self.obs_rms.get_states()
            mean, var = mean.contiguous(), var.contiguous()
        L.check(L.lib.pqlk_replay_gather_fused(C.byref(memory.ring.desc), L.ptr(idx), B, L.ptr(mean), L.ptr(var), float(eps), 0,
                                               L.ptr(ws["x_sa"]), ws["ld_sa"], L.ptr(ws["xn_sa"]), L.ptr(ws["xn_obs"]), ws["ld_o"],
                                               L.ptr(ws["rew"]), L.ptr(ws["done"]), L.stream(self.device)))
        ws["x_obs"][:, :O].copy_(ws["x_sa"][:, :O])
        ws["x_pi"][:, :O].copy_(ws["x_sa"][:, :O])
        return idx

    # ---- the critic's launches: THE place where its kind is told apart.  A critic that is one MLP arena (`layout`: DoubleQ) runs
    # the fused-MLP calls; a per-layer critic (`forward_raw` / `backward_raw`: DoubleQLayerNorm) runs its own.
    @property
    def _one_layout(self):
        return hasattr(self.critic, "layout")

    def _critic_forward(self, ws, net, x, slot, probe=False):
        """Q of `net` (the critic or its target) on x (B, ld_sa) -> ((2, B, ld) output, ld).  slot: "c" (the stash `_critic_grads` /
        `_critic_dx` read) or "t" (the target's).  probe (the diagnostics): a stash of the probe's own, and a dropout critic runs
        without dropout and leaves its call counter alone."""
        if self._one_layout:
            cl = net.layout
            key = ("diag_" if probe else "acts_") + slot
            if key not in ws:
                ws[key] = torch.empty(cl.acts_floats(ws["B"]), dtype=torch.float32, device=self.device)
            mlp_forward_raw(cl, net.arena.data, x, L.ACT_NONE, acts=ws[key])
            return output_view(cl, ws[key], ws["B"]), cl.ld_out
        if probe and hasattr(net, "drop_state"):
            return net.forward_raw(x, drop=False), 32
        return net.forward_raw(x), 32

    def _elu_layers(self):
        """The critic's hidden layers that end in an ELU (0-based), whose outputs the diagnostics' unit statistics read."""
        if self._one_layout:
            return list(range(self.critic.layout.n_layers - 1))
        return self.critic.elu_layers()

    def _probe(self):
        """The diagnostics of the critic as `update_net` leaves it, on the last batch it was trained on (ws["xn_sa"] holds a' in its
        action columns): pql_amd/algo/diag.py.  Runs after the last `update_once`, when no backward is waiting for a stash."""
        d, ws, algo = self._diag, self._ws, self.cfg.algo
        B = ws["B"]
        with torch.cuda.device(self.device):
            qt, _ = self._critic_forward(ws, self.critic_target, ws["xn_sa"], "t", probe=True)
            q, ld = self._critic_forward(ws, self.critic, ws["x_sa"], "c", probe=True)
            d.critic_stats(q, qt, ld, ws["rew"], ws["done"], float(algo.gamma) ** int(algo.nstep), B)
            for net in range(2):
                for k, layer in enumerate(self._elu_layers()):
                    if self._one_layout:
                        cl = self.critic.layout
                        off, ldh = cl.act_offset(B, net, layer)
                        d.unit_stats(net, k, ws["diag_c"][off:], ldh, B, cl.dims[layer + 1])
                    else:
                        y = self.critic.elu_output(B, self.device, net, layer)
                        d.unit_stats(net, k, y, y.stride(0), B, self.critic.dims[layer + 1])
            d.ship()

    def _critic_grads(self, ws, x):
        """Backward of the critic's last forward on x from ws["dy"]: the parameter gradient -> ws["gc"]."""
        if self._one_layout:
            mlp_backward_raw(self.critic.layout, self.critic.arena.data, x, ws["acts_c"], ws["dy"], ws["bwd_c"], ws["gc"], ws["splits"])
        else:
            self.critic.backward_raw(x, ws["dy"], grads=ws["gc"])

    def _critic_dx(self, ws, x, dx, tanh_of=None):
        """Backward of the critic's last forward on x from ws["dy"] to its input, parameters frozen.  tanh_of None: all of
        d loss / d x -> dx (B, ld_sa).  tanh_of (1, B, ld): the actor's tanh output -- the action columns, taken through that tanh
        -> dx (1, B, ld_a), the gradient at the actor's pre-activation output."""
        O, A = self.obs_dim[0], self.action_dim
        if self._one_layout:
            cl = self.critic.layout
            if tanh_of is None:
                mlp_backward_raw(cl, self.critic.arena.data, x, ws["acts_c"], ws["dy"], ws["bwd_c"], dx=dx)
            else:
                mlp_backward_raw(cl, self.critic.arena.data, x, ws["acts_c"], ws["dy"], ws["bwd_c"], dx=dx, dx_col0=O, dx_cols=A,
                                 dx_tanh_of=tanh_of)
            return
        g = self.critic.backward_raw(x, ws["dy"], grads=None, need_dx=True)
        if tanh_of is None:
            dx.copy_(g)
        else:
            a = tanh_of[0]
            dx[0, :, :A] = g[:, O:O + A] * (1.0 - a[:, :A] * a[:, :A])

    def _td_mse_loss(self, ws, q, qt, ld, soft=None):
        """The head's critic loss (`CriticHead.critic_loss`; scalar: twin MSE against the TD target): d loss / d q -> ws["dy"], the loss -> the critic's ring."""
        algo = self.cfg.algo
        memory = ws.get("per")
        # with prioritized replay: the importance weights on the loss and its gradient, then |TD| back into the tree
        per = None if memory is None else (ws["w"], ws["wmax"], ws["abs_td"])
        self.head.critic_loss(q, qt, ld, ws["rew"], ws["done"], float(algo.gamma) ** int(algo.nstep), ws["B"], ws["dy"], self.closs, self.copt.step,
                              ws["scratch"], self.device, per=per, soft=soft, kappa=float(algo.get("huber_kappa", 1.0)))
        if memory is not None:
            memory.update_priorities(ws["idx"], ws["abs_td"])

    def _dpg_loss(self, ws, q, ld, mean=False):
        """-mean(min q) (mean=True: see `CriticHead.actor_loss`): d loss / d q -> ws["dy"], the loss -> the actor's ring."""
        self.head.actor_loss(q, ld, ws["B"], ws["dy"], self.aloss, self.aopt.step, ws["scratch"], self.device, mean=mean)

    def _critic_step(self, ws):
        algo = self.cfg.algo
        apply_optimizer(self.critic.arena.data, ws["gc"], self.copt, None, algo.critic_lr, algo.max_grad_norm, 0.0, 1.0, self.device)

    def _actor_step(self, ws, dy_a):
        """The policy MLP's backward from `dy_a` (the gradient at its pre-activation output), then clip + AdamW."""
        algo = self.cfg.algo
        mlp_backward_raw(self.actor.layout, self.actor.arena.data, ws["x_obs"], ws["acts_a"], dy_a, ws["bwd_a"], ws["ga"], ws["splits"])
        apply_optimizer(self.actor.arena.data, ws["ga"], self.aopt, None, algo.actor_lr, algo.max_grad_norm, 0.0, 1.0, self.device)

    def _update_targets(self):
        """soft_update(target, net, tau) of whichever targets exist."""
        pairs = [(self.critic_target, self.critic)] if self.TARGET_CRITIC else []
        if self.actor_target is not self.actor:
            pairs.append((self.actor_target, self.actor))
        for tgt, net in pairs:
            L.check(L.lib.pqlk_polyak(L.ptr(tgt.arena.data), L.ptr(net.arena.data), net.arena.numel(), float(self.cfg.algo.tau),
                                      L.stream(self.device)))

    def _extra_log(self):
        return self.diagnostics()

    def diagnostics(self):
        """The `diag/*` values of the last probe whose copy has reached the host ({}: algo.diag.enabled off, or none has landed yet)."""
        return {} if self._diag is None else self._diag.diagnostics()

    def update_net(self, memory):
        n = int(self.cfg.algo.update_times)
        for _ in range(n):
            self.update_once(memory)
        self.per_calls += 1
        if self._diag is not None and self._diag.due() and n > 0:
            self._probe()
        c, a = self.closs.tolist(), self.aloss.tolist()
        k = min(n, LOSS_RING)
        return {"train/critic_loss": float(np.mean(c[:k])), "train/actor_loss": float(np.mean(a[:k])),
                "train/return": self.return_tracker.mean(), "train/episode_length": self.step_tracker.mean(), **self._extra_log()}
