"""On-policy PPO baseline on the PQL kernels (`algo=ppo_algo`; reference pql/algo/ppo.py).

Rollout (`explore_env`): per env step obs_rms update, the raw obs into the (T, N) trajectory slab, the policy MLP and the
diagonal-Gaussian head (`pqlk_ppo_gauss_head`: action + log-prob straight into the slab), the critic MLP, the optional
value_rms update, `env.step`, the device-side episode trackers.  Then `compute_adv`: critic on the last obs and one `pqlk_gae`
launch over the whole horizon.  Update (`update_net`): `update_times` epochs of the reference's cumulative `np.random.shuffle`
of one index array (global NumPy stream), each minibatch = gather (+ advantage partials) -> actor forward -> policy head ->
actor backward -> clip + AdamW (actor MLP and `logstd` in one flat buffer) -> critic forward -> value head -> critic backward
-> clip + AdamW.  The losses land in device rings; the host reads them once, at the end of `update_net`.
"""
from __future__ import annotations

import numpy as np
import torch

from pql_amd import _lib as L
from pql_amd.algo.critics import make_critic
from pql_amd.algo.diag import diag_cfg
from pql_amd.algo.learner import _AdamState, _cfg_get, apply_optimizer, make_actor
from pql_amd.algo.pql_actor import DeviceTracker, PQLActor
from pql_amd.models.mlp import default_splits, mlp_backward_raw, mlp_forward_raw, output_view
from pql_amd.utils.info_track import InfoTrackers
from pql_amd.utils.noise import noise_color
from pql_amd.utils.torch_util import RunningMeanStd

TIMEOUT_KEYS = ("TimeLimit.truncated", "time_outs")


class AgentPPO:
    def __init__(self, env, cfg):
        diag_cfg(cfg)   # algo.diag.enabled=True is refused before anything is allocated: the critic diagnostics are the Q learners'
        noise_color(cfg)   # algo.noise.color != white likewise: PPO samples its own Gaussian policy
        self.env, self.cfg = env, cfg
        self.obs_dim = env.observation_space.shape
        self.action_dim = env.action_space.shape[0]
        dev = torch.device(f"{cfg.sim_device}")
        if dev.type == "cuda" and dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        self.device = self.sim_device = dev
        algo = cfg.algo
        self.actor = make_actor(cfg, self.obs_dim, self.action_dim, dev)   # actor first: both consume the CPU generator
        self.critic = make_critic(cfg, self.obs_dim, self.action_dim, dev)
        if not hasattr(self.actor, "logstd_block") or self.critic.layout.dims[-1] != 1:
            raise ValueError("PPO needs act_class: DiagGaussianMLPPolicy and cri_class: MLPCritic")
        self.aopt, self.copt = _AdamState(self.actor.arena.data), _AdamState(self.critic.arena.data)
        n = cfg.num_envs
        self.return_tracker = DeviceTracker(algo.tracker_len, dev)
        self.step_tracker = DeviceTracker(algo.tracker_len, dev)
        self.success_tracker = DeviceTracker(algo.tracker_len, dev)
        self.info_trackers = InfoTrackers.from_cfg(cfg, env, n, algo.tracker_len, dev)   # ac_base.py:54-59 (empty without info_track_keys)
        self.current_returns = torch.zeros(n, dtype=torch.float32, device=dev)
        self.current_lengths = torch.zeros(n, dtype=torch.float32, device=dev)
        self.obs_rms = RunningMeanStd(shape=self.obs_dim, device=dev) if algo.obs_norm else None
        self.value_rms = RunningMeanStd(shape=(1,), device=dev) if algo.value_norm else None
        self.obs, self.dones = None, None
        self.timeout_info = None
        self._roll, self._ws = None, None
        self.aloss = self.closs = None

    # ---- small API kept from the reference ---------------------------------------------------------
    def reset_agent(self):
        self.obs = self.env.reset()
        n = self.cfg.num_envs
        self.dones = torch.zeros(n, dtype=torch.float32, device=self.device)
        self.current_returns.zero_()
        self.current_lengths.zero_()
        return self.obs

    def update_tracker(self, reward, done, info):
        PQLActor.update_tracker(self, reward, done, info)
        if isinstance(info, dict) and "success" in info:
            self.success_tracker.update(info["success"].to(torch.float32), done.bool())

    add_info_tracker_log = PQLActor.add_info_tracker_log   # ac_base.py:116-119

    def _layout(self):
        return self.actor.layout, self.critic.layout

    # ---- rollout -------------------------------------------------------------------------------------
    def _rollout_bufs(self, T):
        n, O, A, dev = self.cfg.num_envs, self.obs_dim[0], self.action_dim, self.device
        r = self._roll
        if r is not None and r["T"] == T:
            return r
        al, cl = self._layout()
        f = dict(dtype=torch.float32, device=dev)
        r = dict(T=T, obs=torch.zeros((T, n, O), **f), act=torch.zeros((T, n, A), **f), logp=torch.zeros((T, n), **f),
                 rew=torch.zeros((T, n), **f), done=torch.zeros((T, n), **f), val=torch.zeros((T, n), **f),
                 tmo=torch.zeros((T, n), **f), adv=torch.zeros((T, n), **f), ret=torch.zeros((T, n), **f),
                 x=torch.zeros((n, L.ld(O)), **f), acts_a=torch.empty(al.acts_floats(n), **f), acts_c=torch.empty(cl.acts_floats(n), **f))
        self._roll = r
        return r

    def _normalized_input(self, ob, x):
        if self.obs_rms is not None:
            self.obs_rms.normalize(ob.contiguous(), out=x)
        else:
            x[:, : ob.shape[1]].copy_(ob)
        return x

    def _value(self, x, r):
        """critic(x) -> (N, 1) (value_rms: update + unnormalise, ppo.py:25-27)."""
        cl = self.critic.layout
        n = x.shape[0]
        mlp_forward_raw(cl, self.critic.arena.data, x, L.ACT_NONE, acts=r["acts_c"])
        v = output_view(cl, r["acts_c"], n)[0][:, :1]
        if self.value_rms is not None:
            v = v.contiguous()
            self.value_rms.update(v)
            v = self.value_rms.unnormalize(v)
        return v

    def get_actions(self, obs, eps=None):
        """-> (actions, log_prob, value.flatten()) as ppo.py:19-28; eps: injected standard-normal draw."""
        r = self._rollout_bufs(1) if self._roll is None else self._roll
        if obs.shape[0] != r["x"].shape[0]:
            raise ValueError("get_actions takes one row per env")
        x = self._normalized_input(obs, r["x"])
        act, logp = self._policy(x, r, eps)
        return act, logp, self._value(x, r).flatten()

    def _policy(self, x, r, eps, act_out=None, logp_out=None):
        al = self.actor.layout
        n, A = x.shape[0], self.action_dim
        mlp_forward_raw(al, self.actor.arena.data, x, L.ACT_NONE, acts=r["acts_a"])
        y = output_view(al, r["acts_a"], n)[0]
        if eps is None:
            eps = torch.randn((n, A), dtype=torch.float32, device=self.device)
        eps = eps.to(self.device, torch.float32).contiguous()
        act = act_out if act_out is not None else torch.empty((n, A), dtype=torch.float32, device=self.device)
        logp = logp_out if logp_out is not None else torch.empty(n, dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            L.check(L.lib.pqlk_ppo_gauss_head(L.ptr(y), al.ld_out, L.ptr(self.actor.logstd_block(self.actor.arena.data)), L.ptr(eps), n, A,
                                              L.ptr(act), A, L.ptr(logp), None, L.stream(self.device)))
        return act, logp

    @torch.no_grad()
    def explore_env(self, env, timesteps: int, random: bool = False, draws=None):
        """ppo.py:30-77 -> ((b_obs, b_actions, b_logprobs, b_advantages, b_returns, b_values), env steps).  traj_dones[t] is the
        done flag BEFORE step t; `self.dones` carries across calls.  draws: optional (T, N, A) standard-normal samples."""
        algo, T = self.cfg.algo, int(timesteps)
        r = self._rollout_bufs(T)
        ob, dones = self.obs, self.dones
        tkey = None
        for t in range(T):
            if self.obs_rms is not None:
                self.obs_rms.update(ob)
            r["obs"][t].copy_(ob)
            r["done"][t].copy_(dones)
            x = self._normalized_input(ob, r["x"])
            self._policy(x, r, None if draws is None else draws[t], act_out=r["act"][t], logp_out=r["logp"][t])
            r["val"][t].copy_(self._value(x, r)[:, 0])
            next_ob, reward, done, info = env.step(r["act"][t])
            self.update_tracker(reward, done, info)
            r["rew"][t].copy_(reward)
            if algo.handle_timeout and isinstance(info, dict):
                if t == 0:
                    tkey = next((k for k in TIMEOUT_KEYS if k in info), None)
                if tkey is not None:
                    r["tmo"][t].copy_(info[tkey])
            ob, dones = next_ob, done.to(torch.float32)
        if tkey is not None:
            self.timeout_info = r["tmo"]
        self.obs, self.dones = ob, dones
        data = self.compute_adv(r, ob, dones, gae=algo.use_gae, timeout=self.timeout_info if algo.handle_timeout else None)
        return data, T * self.cfg.num_envs

    @torch.no_grad()
    def compute_adv(self, r, next_obs, next_done, gae=True, timeout=None):
        """ppo.py:79-139 on the rollout slabs: critic(next obs), one pqlk_gae launch, value_norm updates (returns, then values)."""
        algo = self.cfg.algo
        T, n, O = r["obs"].shape
        x = self._normalized_input(next_obs, r["x"])
        nv = self._value(x, r).reshape(-1).contiguous()
        nd = next_done.to(torch.float32).contiguous()
        with torch.cuda.device(self.device):
            L.check(L.lib.pqlk_gae(L.ptr(r["rew"]), L.ptr(r["done"]), L.ptr(r["val"]), L.ptr(nv), L.ptr(nd),
                                   L.ptr(timeout) if timeout is not None else None, T, n, float(algo.gamma), float(algo.lambda_gae_adv),
                                   1 if gae else 0, L.ptr(r["adv"]), L.ptr(r["ret"]), L.stream(self.device)))
        b_ret, b_val = r["ret"].reshape(-1), r["val"].reshape(-1)
        if self.value_rms is not None:
            self.value_rms.update(b_ret)
            b_ret = self.value_rms.normalize(b_ret)
            self.value_rms.update(b_val)
            b_val = self.value_rms.normalize(b_val)
        return (r["obs"].reshape(T * n, O), r["act"].reshape(T * n, self.action_dim), r["logp"].reshape(-1), r["adv"].reshape(-1),
                b_ret, b_val)

    # ---- learning ------------------------------------------------------------------------------------
    def _workspace(self, B):
        ws = self._ws
        if ws is not None and ws["B"] == B:
            return ws
        f = dict(dtype=torch.float32, device=self.device)
        O, A = self.obs_dim[0], self.action_dim
        al, cl = self._layout()
        ws = dict(B=B, ldx=L.ld(O), splits=default_splits(B, _cfg_get(self.cfg.algo, "dw_splits", 16)))
        for k, shape in dict(x=(B, ws["ldx"]), act=(B, A), logp=(B,), adv=(B,), ret=(B,), val=(B,),
                             adv_part=(3 * int(L.lib.pqlk_ppo_gather_parts(B)),), dy_a=(1, B, al.ld_out), dy_c=(1, B, cl.ld_out),
                             ga=(self.actor.arena.numel(),), gc=(self.critic.arena.numel(),),
                             sc_a=(int(L.lib.pqlk_ppo_scratch_floats(B, A)),), sc_c=(int(L.lib.pqlk_ppo_scratch_floats(B, 1)),),
                             eps_discard=(B, A)).items():
            ws[k] = torch.zeros(shape, **f)
        ws["acts_a"] = torch.empty(al.acts_floats(B), **f)
        ws["acts_c"] = torch.empty(cl.acts_floats(B), **f)
        ws["bwd_a"] = torch.empty(al.bwd_ws_floats(B, ws["splits"]), **f)
        ws["bwd_c"] = torch.empty(cl.bwd_ws_floats(B, ws["splits"]), **f)
        self._ws = ws
        return ws

    def _ensure(self, ws, key, n):
        if ws[key].numel() < n:
            ws[key] = torch.empty(n, dtype=torch.float32, device=self.device)
        return ws[key]

    def _loss_rings(self, k):
        if self.aloss is None or self.aloss.numel() != k:
            self.aloss = torch.zeros(k, dtype=torch.float32, device=self.device)
            self.closs = torch.zeros(k, dtype=torch.float32, device=self.device)

    @torch.no_grad()
    def update_minibatch(self, data, idx, ring_len):
        """One minibatch of ppo.py:149-176 from the device permutation slice `idx` (int64, mb <= batch_size rows)."""
        algo, dev = self.cfg.algo, self.device
        b_obs, b_act, b_logp, b_adv, b_ret, b_val = data
        mb, rows = idx.numel(), b_obs.shape[0]
        ws = self._workspace(min(int(algo.batch_size), rows))
        O, A = self.obs_dim[0], self.action_dim
        al, cl = self._layout()
        splits = default_splits(mb, _cfg_get(algo, "dw_splits", 16))
        x, ldx = ws["x"][:mb], ws["ldx"]
        acts_a = self._ensure(ws, "acts_a", al.acts_floats(mb))
        acts_c = self._ensure(ws, "acts_c", cl.acts_floats(mb))
        bwd_a = self._ensure(ws, "bwd_a", al.bwd_ws_floats(mb, splits))
        bwd_c = self._ensure(ws, "bwd_c", cl.bwd_ws_floats(mb, splits))
        mean = var = None
        eps = 0.0
        if self.obs_rms is not None:
            mean, var, eps = self.obs_rms.get_states()
            mean, var = mean.contiguous(), var.contiguous()
        with torch.cuda.device(dev):
            st = L.stream(dev)
            # ppo.py:154 `logprob_entropy` -> get_actions(state) draws an (mb, A) rsample from torch's generator and discards it: draw
            # the same amount so a seeded run's later rollout draws stay those of the reference
            ws["eps_discard"][:mb].normal_()
            L.check(L.lib.pqlk_ppo_gather(L.ptr(idx), mb, rows, L.ptr(b_obs), O, L.ptr(mean), L.ptr(var), float(eps), L.ptr(x), ldx,
                                          L.ptr(b_act), A, L.ptr(ws["act"]), L.ptr(b_logp), L.ptr(b_adv), L.ptr(b_ret), L.ptr(b_val),
                                          L.ptr(ws["logp"]), L.ptr(ws["adv"]), L.ptr(ws["ret"]), L.ptr(ws["val"]), L.ptr(ws["adv_part"]), st))
            # ---- actor: clipped surrogate - lambda_entropy * entropy, clip + AdamW over the MLP and logstd together
            mlp_forward_raw(al, self.actor.arena.data, x, L.ACT_NONE, acts=acts_a)
            y = output_view(al, acts_a, mb)[0]
            dy_a = ws["dy_a"][:, :mb]
            L.check(L.lib.pqlk_ppo_policy_loss(L.ptr(y), al.ld_out, L.ptr(self.actor.logstd_block(self.actor.arena.data)), L.ptr(ws["act"]),
                                               L.ptr(ws["logp"]), L.ptr(ws["adv"]), L.ptr(ws["adv_part"]), int(L.lib.pqlk_ppo_gather_parts(mb)),
                                               mb, A, float(algo.ratio_clip), float(algo.lambda_entropy), L.ptr(dy_a),
                                               L.ptr(self.actor.logstd_block(ws["ga"])), None, L.ptr(ws["sc_a"]), ws["sc_a"].numel(),
                                               L.ptr(self.aloss), L.ptr(self.aopt.step), ring_len, st))
            mlp_backward_raw(al, self.actor.arena.data, x, acts_a, dy_a, bwd_a, ws["ga"], splits, rows=mb)
            apply_optimizer(self.actor.arena.data, ws["ga"], self.aopt, None, algo.actor_lr, algo.max_grad_norm, 0.0, 1.0, dev)
            # ---- critic: (clipped) value loss
            mlp_forward_raw(cl, self.critic.arena.data, x, L.ACT_NONE, acts=acts_c)
            v = output_view(cl, acts_c, mb)[0]
            dy_c = ws["dy_c"][:, :mb]
            L.check(L.lib.pqlk_ppo_value_loss(L.ptr(v), cl.ld_out, L.ptr(ws["ret"]), L.ptr(ws["val"]), mb, 1 if algo.value_clip else 0,
                                              float(algo.ratio_clip), L.ptr(dy_c), cl.ld_out, L.ptr(ws["sc_c"]), ws["sc_c"].numel(),
                                              L.ptr(self.closs), L.ptr(self.copt.step), ring_len, st))
            mlp_backward_raw(cl, self.critic.arena.data, x, acts_c, dy_c, bwd_c, ws["gc"], splits, rows=mb)
            apply_optimizer(self.critic.arena.data, ws["gc"], self.copt, None, algo.critic_lr, algo.max_grad_norm, 0.0, 1.0, dev)

    def minibatch_plan(self, rows):
        B = int(self.cfg.algo.batch_size)
        return [(s, min(s + B, rows)) for s in range(0, rows, B)]

    @torch.no_grad()
    def update_net(self, data, perms=None):
        """ppo.py:141-190.  perms: optional (update_times, rows) permutations instead of the np.random.shuffle draws."""
        algo = self.cfg.algo
        rows = data[0].shape[0]   # the reference asserts rows >= batch_size; here a shorter trajectory is one minibatch
        plan = self.minibatch_plan(rows)
        epochs = int(algo.update_times)
        k = epochs * len(plan)
        self._loss_rings(k)
        b_inds = np.arange(rows)
        for ep in range(epochs):
            if perms is None:
                np.random.shuffle(b_inds)
                host = torch.from_numpy(b_inds.astype(np.int64))
            else:
                host = torch.as_tensor(np.asarray(perms[ep]), dtype=torch.int64)
            idx = host.pin_memory().to(self.device, non_blocking=True) if torch.cuda.is_available() else host.to(self.device)
            for s, e in plan:
                self.update_minibatch(data, idx[s:e], k)
        # one read of the host per update: the k slots step % k of this call's minibatches are k consecutive counter values
        c, a = self.closs.tolist(), self.aloss.tolist()
        return {"train/critic_loss": float(np.mean(c)), "train/actor_loss": float(np.mean(a)),
                "train/return": self.return_tracker.mean(), "train/episode_length": self.step_tracker.mean(),
                "train/success_rate": self.success_tracker.mean()}

    def loss_history(self):
        """(actor, critic) losses of the last update_net in minibatch order."""
        k = self.aloss.numel()
        start = (int(self.aopt.step.item()) - k) % k
        order = [(start + i) % k for i in range(k)]
        return self.aloss.cpu().numpy()[order], self.closs.cpu().numpy()[order]
