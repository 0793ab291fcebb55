"""P-learner: the policy side of Parallel Q-Learning on one MI355X.

Drop-in for `pql/algo/pql_p_learner.py`: `PQLPLearner(obs_dim, action_dim, cfg)` with `start()`, `learn()`,
`update(critic, obs, normalize_tuple, sleep_time)` and the pump `asyn_p_learner`.

learn()  (reference :47-64)  ->  one launch sequence
    randint -> fused obs gather+normalise -> actor fwd (tanh; action dropped into the critic input) ->
    frozen twin-critic fwd -> DPG loss -mean(min Q) + dL/dQ -> critic bwd, dX ONLY, both nets summed in
    one GEMM, chained through tanh' in the epilogue -> actor bwd (dW + dX) -> clip + AdamW.
`critic.requires_grad_(False)` of the reference (:54) is structural here: no dW GEMM is launched for the critic.
"""
from __future__ import annotations

import ctypes as C

import torch

from pql_amd import _lib as L
from pql_amd.algo.heads import CriticHead
from pql_amd.algo.critics import check_critic_class, make_critic
from pql_amd.algo.learner import (GATHER_FLAGS, Learner, _cfg_get, _cpu, apply_optimizer, apply_optimizer_fused, f32_recip, load_artifact,
                                  make_actor, pump, resident_norm)
from pql_amd.models.mlp import PackedWeights, default_splits, mlp_backward_raw, mlp_forward_raw, output_view
from pql_amd.replay.simple_replay import RecordRing, _obs_width, cfg_obs_dtype, ring_plan
from pql_amd.utils import handoff as H
from pql_amd.utils import rng as R


class PQLPLearner(Learner):
    PARTNER = "critic"   # the frozen critic: a resident replica of the V-learner's
    RESTORE_AFTER_CAPTURE = False

    def __init__(self, obs_dim, action_dim, cfg, process_group=None):
        check_critic_class(cfg, "PQLPLearner")
        if not torch.cuda.is_available():
            raise L.PqlkError("PQLPLearner needs an MI355X (no CPU path)")
        device = torch.device(f"cuda:{int(cfg.algo.p_learner_gpu)}")
        algo = cfg.algo
        self.actor = make_actor(cfg, obs_dim, int(action_dim), device)
        if cfg.artifact is not None:   # local warm start (pql_p_learner.py:27-28)
            load_artifact(cfg.artifact, actor=self.actor)
        super().__init__(obs_dim, action_dim, cfg, device, process_group, self.actor)
        self.pk_actor = PackedWeights(self.actor.layout, self.device) if self._fused else None
        self._head = None
        # obs-only replay (reference :32-37: a bare (memory_size, obs) tensor + inline pointer logic)
        self.memory_size = int(algo.memory_size)
        self.ring = RecordRing(self.memory_size, _obs_width(obs_dim), -1, self.device, obs_dtype=cfg_obs_dtype(algo))
        self.next_p = 0
        self.if_full = False
        self.cur_capacity = 0
        self.sleep_time = 0.01
        # (one randint per step; a run = the P-steps of one rollout iteration)
        ratio = max(1, int(_cfg_get(algo, "critic_sample_ratio", 8)) // max(1, int(_cfg_get(algo, "critic_actor_ratio", 2))))
        self._depth = max(1, int(_cfg_get(algo, "prefetch_steps_p", ratio)))

    @property
    def memory(self):
        """(memory_size, obs_dim) view of the ring, the reference's attribute name (:34)."""
        return self.ring.obs_view()

    @property
    def head(self):
        """The frozen critic's head, described once per replica."""
        if self._head is None or self._head.critic is not self.critic:
            self._head = CriticHead(self.critic, self.cfg.algo)
        return self._head

    def _bound(self):
        return self.cur_capacity

    def _captured(self):
        return (self.actor.arena.data, self.opt.m, self.opt.v, self.opt.step, self.loss_ring)

    def _data_stamp(self):
        """See PQLVLearner._data_stamp: ring contents, randint bound, identity of the statistics."""
        nt = self.normalize_tuple
        return (self.ring.version, self.cur_capacity, None if nt is None else (id(nt[0]), id(nt[1]), float(nt[2])))

    def _workspace(self, B):
        if self._ws is not None and self._ws["B"] == B:
            return self._ws
        f = dict(dtype=torch.float32, device=self.device)
        O, A = self.ring.O, self.action_dim
        al, cl = self.actor.layout, self.critic.layout
        # (the actor's input tile is 64-float aligned -- 128 wide for 88 observations: its layer-1 dW product then reads whole 64-column
        #  tiles of it and takes the LDS-DMA main loop like every other backward GEMM; the extra columns are never written and stay zero)
        ws = dict(B=B, ld_sa=L.ld(O + A), ld_o=(L.ld(O) + 63) // 64 * 64, ld_a=L.ld(A))
        want = self._want_ahead()   # draws + gathered tiles of the next K steps (see PQLVLearner._workspace)
        K = self._depth if want else 1
        self._ahead = R.DrawAhead(self.gen, self.device, B, None, K, R.verified(self.device)) if want else None
        self._slot_graphs, self._run_graph = {}, None
        ws["K"] = K
        # round 4: loss + partition + compact head in one launch, the actor's head backward inside the action-slice launch
        # (pqlk_dpg_backward_fused: 16 -> 13 launches per step); needs the loss fold of the optimiser launch and a fused critic forward
        ws["dpg_fused"] = bool(_cfg_get(self.cfg.algo, "dpg_fused", True) and self._fold_loss and self.head.kind == "scalar" and self.pk_critic is not None
                               and self.pk_critic.tensor is not None and self.pk_actor is not None and self.pk_actor.tensor is not None
                               and L.lib.pqlk_dpg_fused_ok(C.byref(cl.desc), C.byref(al.desc), B))
        # ... and then the critic reads its input where the two halves of torch.cat((obs, action)) already lie -- the actor's input
        # tile and the actor's output block (pqlk_mlp_forward_qc's second source) -- so the gather writes the observations ONCE
        # (no [obs | action] tile at all: 42 -> 24 MB moved per 4-step launch at cfg #2)
        ws["split_in"] = bool(ws["dpg_fused"] and O % 4 == 0 and _cfg_get(self.cfg.algo, "dpg_split_input", True))
        ws["x_sa_all"] = None if ws["split_in"] else torch.zeros((K, B, ws["ld_sa"]), **f)
        ws["x_obs_all"] = torch.zeros((K, B, ws["ld_o"]), **f)
        ws["slots"] = [dict(x_sa=None if ws["split_in"] else ws["x_sa_all"][k], x_obs=ws["x_obs_all"][k]) for k in range(K)]
        ws.update(ws["slots"][0])
        ws["idx"] = torch.zeros(B, dtype=torch.int64, device=self.device)
        ws["acts_a"] = torch.empty(al.acts_floats(B), **f)
        ws["acts_c"] = torch.empty(cl.acts_floats(B), **f)
        ws["dy_c"] = torch.zeros((2, B, cl.ld_out), **f)
        ws["dz_a"] = torch.zeros((1, B, ws["ld_a"]), **f)   # dL/d(actor pre-tanh); pad columns stay zero
        ws["grads"] = torch.zeros(al.total, **f)
        ws["splits"] = default_splits(B, _cfg_get(self.cfg.algo, "dw_splits", 16))
        ws["bwd_c"] = torch.empty(int(L.lib.pqlk_dpg_backward_ws_floats(C.byref(cl.desc), B)), **f)
        ws["owner"] = torch.zeros(B, dtype=torch.uint8, device=self.device)   # which net(s) own each sample's min(Q1, Q2)
        ws["bwd_a"] = torch.empty(al.bwd_ws_floats(B, ws["splits"]), **f)
        ws["scratch"] = torch.zeros(2048, **f)
        if ws["dpg_fused"]:
            ws["qc"] = torch.zeros((2, B), **f)
            ws["head_parts"] = int(L.lib.pqlk_dpg_fused_head_parts(B))
            ws["mn_ptr"] = C.c_void_p(ws["bwd_c"].data_ptr() + 4 * int(L.lib.pqlk_dpg_fused_mn_offset(C.byref(cl.desc), B)))
            ws["loss_parts"] = int(L.lib.pqlk_dpg_fused_loss_parts())
        self._ws = ws
        self.repack()
        return ws

    def repack(self):
        if self.pk_actor is not None:
            self.pk_actor.refresh(self.actor.arena.data)
        if self.pk_critic is not None:
            self.pk_critic.refresh(self.critic.arena.data)

    def _gather(self, ws, idx, rows, x_sa, x_obs):
        mean, var, eps = self._norm_ptrs()
        L.check(L.lib.pqlk_replay_gather_fused(C.byref(self.ring.desc), L.ptr(idx), rows, L.ptr(mean), L.ptr(var), eps, GATHER_FLAGS,
                                               L.ptr(x_sa), ws["ld_sa"], None, L.ptr(x_obs), ws["ld_o"], None, None,
                                               L.stream(self.device)))

    def _prefetch(self, ws, steps=None):
        """The next K steps' indices (torch's numbers, one launch) and ONE gather of their K x B observation rows (`steps` < K: of
        that many steps only, see PQLVLearner._prefetch)."""
        Kp = ws["K"] if steps is None else max(1, min(ws["K"], int(steps)))
        self._ahead.refill(self.cur_capacity, Kp)
        self._gather(ws, self._ahead.idx, Kp * ws["B"], ws["x_sa_all"], ws["x_obs_all"])
        self._ahead_stamp = self._data_stamp()

    def _step_kernels(self, ws, idx, upto_backward=False, tiles=None):
        algo, dev, B = self.cfg.algo, self.device, ws["B"]
        O, A = self.ring.O, self.action_dim
        st = L.stream(dev)
        if tiles is None:   # per-step path: gather `idx` into slot 0 here
            tiles = ws["slots"][0]
            self._gather(ws, idx, B, tiles["x_sa"], tiles["x_obs"])
        ws = dict(ws, **tiles)
        al, cl = self.actor.layout, self.critic.layout
        x_act = None if ws["split_in"] else ws["x_sa"][:, O:]   # (split input: the critic reads the action out of the actor's output block)
        mlp_forward_raw(al, self.actor.arena.data, ws["x_obs"], L.ACT_TANH, acts=ws["acts_a"], out2=x_act, packed=self.pk_actor,
                        stash_all=True)
        tail = self._fused_tail   # see PQLVLearner._step_kernels
        a_out = output_view(al, ws["acts_a"], B)  # (1, B, ld_a): tanh output, for the tanh' chain
        if ws["dpg_fused"]:
            if ws["split_in"]:
                L.check(L.lib.pqlk_mlp_forward_qc(C.byref(cl.desc), L.ptr(self.critic.arena.data), L.ptr(self.pk_critic.tensor), 1, L.ptr(ws["x_obs"]),
                                                  ws["ld_o"], L.ptr(a_out), ws["ld_a"], O, B, L.ptr(ws["acts_c"]), L.ptr(ws["qc"]), st))
            else:
                L.check(L.lib.pqlk_mlp_forward_qc(C.byref(cl.desc), L.ptr(self.critic.arena.data), L.ptr(self.pk_critic.tensor), 1, L.ptr(ws["x_sa"]),
                                                  ws["ld_sa"], None, 0, 0, B, L.ptr(ws["acts_c"]), L.ptr(ws["qc"]), st))
            L.check(L.lib.pqlk_dpg_backward_fused(C.byref(cl.desc), L.ptr(self.critic.arena.data), L.ptr(ws["x_sa"]), ws["ld_sa"], B,
                                                  L.ptr(ws["acts_c"]), L.ptr(ws["qc"]), L.ptr(ws["dz_a"]), ws["ld_a"], O, L.ptr(a_out), ws["ld_a"],
                                                  L.ptr(ws["scratch"]), L.ptr(ws["bwd_c"]), ws["bwd_c"].numel(), C.byref(al.desc),
                                                  L.ptr(self.actor.arena.data), L.ptr(ws["acts_a"]), L.ptr(ws["bwd_a"]), ws["bwd_a"].numel(),
                                                  ws["splits"], st))
            L.check(L.lib.pqlk_mlp_backward_tail(C.byref(al.desc), L.ptr(self.actor.arena.data), L.ptr(ws["x_obs"]), ws["ld_o"], B,
                                                 L.ptr(ws["acts_a"]), L.ptr(ws["grads"]), ws["splits"], L.ptr(ws["bwd_a"]), ws["bwd_a"].numel(),
                                                 L.ptr(self.opt.scratch) if tail else None, L.ptr(self.opt.step) if tail else None,
                                                 ws["head_parts"], ws["mn_ptr"], st))
            if upto_backward:
                return
            self._allreduce_grads(ws)
            self._step_post(ws)
            return
        mlp_forward_raw(cl, self.critic.arena.data, ws["x_sa"], L.ACT_NONE, acts=ws["acts_c"], packed=self.pk_critic,
                        stash_all=True)   # the dX chain through the frozen critic needs its activations (ELU')
        q = output_view(cl, ws["acts_c"], B)
        head = self.head   # -mean(min Q) and, of scalar heads, the owner partition (the quantile entry has none, the categorical one leaves it unwritten)
        head.actor_loss(q, cl.ld_out, B, ws["dy_c"], None if self._fold_loss else self.loss_ring, self.opt.step, ws["scratch"], dev,
                        owner=None if head.kind == "quantile" else ws["owner"])
        # dX-only chain through the frozen critic; with scalar Q heads it runs over the samples partitioned by the net that
        # attained min(Q1, Q2): the other net's rows of every dZ are exactly zero (csrc/minnet.h)
        L.check(L.lib.pqlk_dpg_critic_backward(C.byref(cl.desc), L.ptr(self.critic.arena.data), L.ptr(ws["x_sa"]), ws["ld_sa"], B,
                                               L.ptr(ws["acts_c"]), L.ptr(ws["dy_c"]), L.ptr(ws["dz_a"]), ws["ld_a"], O, A,
                                               L.ptr(a_out), ws["ld_a"], C.c_void_p(ws["owner"].data_ptr()) if head.width == 1 else None,
                                               L.ptr(ws["bwd_c"]), ws["bwd_c"].numel(), st))
        if tail:
            L.check(L.lib.pqlk_mlp_backward_norm(C.byref(al.desc), L.ptr(self.actor.arena.data), L.ptr(ws["x_obs"]), ws["ld_o"], B,
                                                 L.ptr(ws["acts_a"]), L.ptr(ws["dz_a"]), L.ptr(ws["grads"]), ws["splits"], None, 0, 0,
                                                 0, None, 0, L.ptr(ws["bwd_a"]), ws["bwd_a"].numel(), L.ptr(self.opt.scratch),
                                                 L.ptr(self.opt.step), st))
        else:
            mlp_backward_raw(al, self.actor.arena.data, ws["x_obs"], ws["acts_a"], ws["dz_a"], ws["bwd_a"], ws["grads"], ws["splits"])
        if upto_backward:
            return
        self._allreduce_grads(ws)
        self._step_post(ws)

    def _step_post(self, ws):
        algo = self.cfg.algo
        if self._fold_loss:
            apply_optimizer_fused(self.actor.layout, self.actor.arena.data, ws["grads"], self.opt, None, algo.actor_lr,
                                  algo.max_grad_norm, 0.0, self.pk_actor, None, ws["scratch"],
                                  ws["loss_parts"] if ws["dpg_fused"] else self.head.loss_parts(ws["B"]),
                                  f32_recip(ws["B"], sign=-1.0), self.loss_ring, self.device, norm_in_backward=self._fused_tail,
                                  grad_scale=1.0 / self.world)
            return
        apply_optimizer(self.actor.arena.data, ws["grads"], self.opt, None, algo.actor_lr, algo.max_grad_norm, 0.0,
                        1.0 / self.world, self.device, layout=self.actor.layout, packed=self.pk_actor)

    def _draws(self, ws):
        torch.randint(self.cur_capacity, (ws["B"],), generator=self.gen, out=ws["idx"])  # the only draw (:49), no copy launch

    def _step(self, ws, slot=None, upto_backward=False, part=None):
        """The step on the tiles `_prefetch` left in `slot`; None = on the per-step draw in ws["idx"]."""
        self._step_kernels(ws, ws["idx"] if slot is None else None, upto_backward, tiles=None if slot is None else ws["slots"][slot])

    def learn(self, indices=None):
        return self._learn(indices)

    def _learn_injected(self, ws, indices, home):
        self._inject(ws["idx"], indices, home)
        self._step_kernels(ws, ws["idx"])

    def _own_state(self):
        return {"actor": _cpu(self.actor.arena.data),
                "critic": None if self.critic is None else _cpu(self.critic.arena.data),   # lags the live critic by design
                "memory": {"ring": self.ring.training_state(), "next_p": int(self.next_p), "if_full": bool(self.if_full),
                           "cur_capacity": int(self.cur_capacity)}}   # (the rows: `ring.rows(cur_capacity)`)

    def _load_own_state(self, st, memory):
        self.actor.arena.data.copy_(st["actor"])
        self._load_partner(st["critic"], make_critic)
        if memory:
            m = st["memory"]
            self.ring.load_training_state(m["ring"])
            self.next_p, self.if_full, self.cur_capacity = int(m["next_p"]), bool(m["if_full"]), int(m["cur_capacity"])

    def set_critic(self, critic, home=None):
        self._adopt_partner(critic, home)

    def _new_partner(self, critic):
        if hasattr(critic, "z_atoms"):   # (a plain attribute: `.to(device)` of the module does not move it)
            critic.z_atoms = critic.z_atoms.to(self.device)
            critic.device = self.device

    @torch.no_grad()
    def update(self, critic, obs, normalize_tuple, sleep_time):
        """pql_p_learner.py:66-85, enqueued on this learner's stream behind event fences (see PQLVLearner.update)."""
        home = torch.cuda.current_stream(self.device)
        with self._lock, torch.cuda.device(self.device), self._on_stream():
            st = torch.cuda.current_stream(self.device)
            self.set_critic(critic, home)
            self.sleep_time = sleep_time
            self.normalize_tuple = resident_norm(self, normalize_tuple, home)
            with H.LOCK:
                lease = H.acquire(obs, st, home)
                obs = obs.reshape(-1, self.ring.O).to(self.device, torch.float32).contiguous()
                self.add_capacity = obs.shape[0]
                segs, self.next_p, self.if_full, self.cur_capacity = ring_plan(self.next_p, self.if_full, self.memory_size,
                                                                               obs.shape[0])
                self.ring.insert_segments(segs, obs)
                H.release(lease, st)
            self._drop_ahead()   # ring contents, the randint bound and the statistics changed: later steps sample afresh
            loss = self._lagged.poll(self.update_count)
            return self._published(), loss, self.update_count


def asyn_p_learner(learner, cfg, stop_event=None, max_in_flight=2):
    """Free-running pump (reference: a Ray task, :99-104).  Run it in a thread."""
    pump(learner, stop_event, max_in_flight)
