"""V-learner: the critic side of Parallel Q-Learning on one MI355X.

Drop-in for `pql/algo/pql_v_learner.py`: `PQLVLearner(obs_dim, action_dim, cfg)` with `start()`,
`learn()`, `update(actor, trajectory, normalize_tuple, sleep_time)` and the module-level pump
`asyn_v_learner(learner, cfg)`.  The reference wraps the class in a Ray actor (:21) and ships whole
nn.Modules through the object store; here it is a plain object that owns a HIP stream's worth of work:

learn()  (reference :73-115, ~150 ATen launches + 1 host sync)  ->  one fixed launch sequence
    randint -> fused gather+normalise+cat -> actor fwd (+target-policy noise, written straight into the
    target critic's input) -> target twin-critic fwd -> twin-critic fwd -> TD/MSE or C51/BCE loss + dL/dQ
    -> critic bwd (split-batch dW) -> clip + AdamW + Polyak over flat arenas.
No `.item()`: losses land in a device ring read lazily by `update()`.  With `cfg.algo.graph` the sequence
is captured once into a hipGraph (through torch.cuda.CUDAGraph) and replayed.
"""
from __future__ import annotations

import ctypes as C
from copy import deepcopy

import torch

from pql_amd import _lib as L
from pql_amd.algo.heads import CriticHead
from pql_amd.algo.critics import check_critic_class, check_target_dtype, make_critic
from pql_amd.algo.diag import CriticProbe, diag_cfg
from pql_amd.algo.learner import (GATHER_FLAGS, Learner, _cfg_get, _cpu, apply_optimizer, apply_optimizer_fused, distl_loss,
                                  graph_collective_enabled, load_artifact, make_actor, pump, resident_norm)
from pql_amd.models.mlp import (HIDDEN_DEFAULT, PackedWeights, PackedWeightsBf16, default_splits, mlp_backward_raw, mlp_forward_bf16_raw, mlp_forward_raw,
                                output_view)
from pql_amd.replay.prioritized_replay import PrioritizedReplayBuffer, per_beta, per_cfg
from pql_amd.replay.simple_replay import ReplayBuffer, cfg_obs_dtype
from pql_amd.utils import dp as DP
from pql_amd.utils import handoff as H
from pql_amd.utils import rng as R


class PQLVLearner(Learner):
    PARTNER = "actor"   # the target policy: a resident replica of the P-learner's actor

    def __init__(self, obs_dim, action_dim, cfg, process_group=None):
        check_critic_class(cfg, "PQLVLearner")
        diag = diag_cfg(cfg)   # algo.diag: refused or accepted before anything is allocated
        # algo.per.enabled=True with algo.per.refresh=run (anything else was refused above): prioritized replay whose distribution is
        # frozen for each run of prefetched steps.  What it cannot be combined with is refused before anything is allocated.
        self._per = per_cfg(cfg.algo)
        self._per_pending = 0   # steps taken since the last write-back: rows [0, n) of the |TD| slabs wait for `flush_priorities`
        if self._per is not None:
            if _cfg_get(cfg.algo, "distl", False) and distl_loss(cfg.algo) == "c51":   # (hl_gauss has a |TD| and a weighted entry)
                raise ValueError("algo.distl=True is not supported with algo.per.enabled=True (algo.per.refresh=run): there is no weighted C51 loss")
            if process_group is not None:
                raise ValueError("algo.per.enabled=True (algo.per.refresh=run) is single-GPU only: PQLVLearner was given a process group "
                                 "(data parallel), and the ranks' sum trees would have to agree on the priorities")
            if bool(_cfg_get(cfg.algo, "graph_rng", False)):
                raise ValueError("algo.graph_rng=True is not supported with algo.per.enabled=True (algo.per.refresh=run): the sample launch takes "
                                 "beta from the host and the rows in the ring, neither of which may be baked into a captured step")
        if not torch.cuda.is_available():
            raise L.PqlkError("PQLVLearner needs an MI355X (no CPU path)")
        device = torch.device(f"cuda:{int(cfg.algo.v_learner_gpu)}")
        algo = cfg.algo
        self.critic = make_critic(cfg, obs_dim, int(action_dim), device)
        self.head = CriticHead(self.critic, algo)   # which loss launch a step takes, and the parts and the scale of its fold
        if cfg.artifact is not None:   # local warm start (pql_v_learner.py:44-47): the target below is the copy of what was loaded
            load_artifact(cfg.artifact, critic=self.critic)
        super().__init__(obs_dim, action_dim, cfg, device, process_group, self.critic)
        self.critic_target = deepcopy(self.critic)
        self.pk_critic = PackedWeights(self.critic.layout, self.device) if self._fused else None
        self.pk_target = PackedWeights(self.critic.layout, self.device) if self._fused else None
        self._td_in_head = bool(_cfg_get(algo, "td_in_head", True))   # TD target + MSE inside the head's backward launch
        ring = dict(capacity=int(algo.memory_size), obs_dim=self.obs_dim, action_dim=self.action_dim, device=self.device,
                    obs_dtype=cfg_obs_dtype(algo))
        # (prioritized: `update()`'s add_to_buffer then gives new rows pmax^alpha, as in the baselines)
        self.memory = ReplayBuffer(**ring) if self._per is None else PrioritizedReplayBuffer(alpha=float(self._per.alpha),
                                                                                             eps=float(self._per.eps), **ring)
        self.sleep_time = 0
        # data parallel, algo.dp_buckets: "layer" = the gradient travels in per-layer buckets, each all-reduced as soon as its dW
        # slabs are summed, under the MFMA launches of the layers below (pql_amd/utils/dp.py); "one" = a single collective after
        # the whole backward; "auto" (default) = layer when the collectives are captured inside the step's hipGraph
        # (PQL_DP_GRAPH_COLLECTIVE=1), else one: with eager collectives every bucket ends a graph, and on the one rank this pool
        # can run those extra graph boundaries cost more (1114 vs 1164 steps/s) than a 1-rank collective can give back
        if self.dp and self.critic.layout.n_layers >= 3:
            mode = str(_cfg_get(algo, "dp_buckets", "auto"))
            if mode not in ("auto", "layer", "one"):
                raise ValueError(f"algo.dp_buckets must be auto, layer or one, got {mode!r}")
            if mode == "auto":
                mode = "layer" if self.use_graph and graph_collective_enabled(self.pg) else "one"
            if mode == "layer":
                self._buckets = DP.layer_buckets(self.critic.layout.n_layers)
                self._reducer = DP.BucketAllReduce(self.pg)
        self._depth = max(1, int(_cfg_get(algo, "prefetch_steps", _cfg_get(algo, "critic_sample_ratio", 8))))
        self.pk_target_bf16 = self.pk_actor_bf16 = None
        self._bf16 = False
        self.set_target_dtype(_cfg_get(algo, "target_dtype", "float32"))
        # algo.diag.enabled: the probe `update()` runs on the last trained batch (pql_amd/algo/diag.py); None = off, nothing below exists
        self._diag = None if diag is None else CriticProbe(self.head, *diag, self.critic.layout.n_layers - 1, self.device)
        self._diag_slot = None   # the slot of the last step taken since the last hand-off (None: no step since)

    def set_target_dtype(self, value):
        """algo.target_dtype: float32 (default) = the two no-gradient forwards of a step -- target policy, target twin critic --
        run on the fp32 kernels like everything else; bfloat16 = on the forward-only bf16-MFMA stack (pql_amd/csrc/fwd_bf16.hip:
        inputs, weights and hidden activations rounded to bf16, fp32 accumulation, biases and output).  Nothing that
        carries a gradient changes.  A shape the bf16 stack cannot take, or algo.fused=False, is an error: no silent fall-back."""
        value = str(value)
        if value not in ("float32", "bfloat16"):
            raise ValueError(f"algo.target_dtype must be float32 or bfloat16, got {value!r}")
        self.flush_priorities()   # (the workspace, and with it the |TD| slabs, is rebuilt below)
        if value == "bfloat16":
            check_target_dtype(self.cfg.algo, value)   # (the class's own rule, as `check_critic_class` applied it to the config's value)
            if not self._fused:
                raise ValueError("algo.target_dtype=bfloat16 needs the fused path (algo.fused=True)")
            hidden = _cfg_get(self.cfg.algo, "hidden_layers")
            O = self.obs_dim[0] if isinstance(self.obs_dim, (tuple, list)) else self.obs_dim
            a_dims = [int(O), *(HIDDEN_DEFAULT if hidden is None else hidden), self.action_dim]
            for name, desc, dims in (("critic", self.critic.layout.desc, self.critic.layout.dims), ("actor", L.mlp_desc(a_dims, 1), a_dims)):
                if not L.lib.pqlk_mlp_bf16_ok(C.byref(desc)):
                    raise ValueError(f"algo.target_dtype=bfloat16: the {name}'s layers {list(dims)} do not fit the bf16 forward (>= 2 "
                                     f"layers, hidden widths multiples of 32 and <= 1024, output width <= 64)")
            self.pk_target_bf16 = PackedWeightsBf16(self.critic.layout, self.device)
        else:
            self.pk_target_bf16 = None
        self.pk_actor_bf16 = None
        self._bf16 = value == "bfloat16"
        self._ws, self._graph, self._graph_post, self._graph_key, self._slot_graphs, self._run_graph = None, None, None, None, {}, None
        self._drop_ahead()
        if self._bf16:
            with torch.cuda.device(self.device):
                self._repack_bf16()

    def _repack_bf16(self):
        """The bf16 weight copies of the two target networks, re-derived from their arenas."""
        self.pk_target_bf16.refresh(self.critic_target.arena.data)
        if self.actor is not None:
            if self.pk_actor_bf16 is None or self.pk_actor_bf16.layout is not self.actor.layout:
                self.pk_actor_bf16 = PackedWeightsBf16(self.actor.layout, self.device)
            self.pk_actor_bf16.refresh(self.actor.arena.data)

    def _actor_in_sa(self):
        """Whether the target policy reads norm(next_obs) straight out of the target critic's input tile (its kernel masks
        everything past column O while staging): the fused fp32 forward and the bf16 forward do."""
        return self._bf16 or (self.pk_actor is not None and self.pk_actor.tensor is not None)

    def _bound(self):
        return self.memory.cur_capacity

    def _captured(self):
        return (self.critic.arena.data, self.critic_target.arena.data, self.opt.m, self.opt.v, self.opt.step, self.loss_ring)

    def _data_stamp(self):
        """What the tiles gathered ahead depend on besides the draws: the ring's contents (insert counter), the randint bound and
        the identity of the normalisation statistics.  `update()` drops the tiles itself; this catches every OTHER way the data can
        change under a learner that has steps prepared -- `memory.add_to_buffer(...)` called directly, `normalize_tuple` or
        `memory.cur_capacity` assigned from outside (tools/gen_golden-style drivers, tests) -- which would otherwise train up to
        K - 1 steps on stale rows, stale statistics or a stale bound without any error."""
        nt = self.normalize_tuple
        # (+ the target policy, whose actions for the prepared steps are computed at prefetch time: object and in-place version)
        pol = None if self.actor is None else (id(self.actor), self.actor.arena.data._version)
        return (self.memory.ring.version, self.memory.cur_capacity, None if nt is None else (id(nt[0]), id(nt[1]), float(nt[2])), pol)

    def _workspace(self, B):
        if self._ws is not None and self._ws["B"] == B:
            return self._ws
        self.flush_priorities()
        dev, f = self.device, dict(dtype=torch.float32, device=self.device)
        O, A = self.memory.ring.O, self.action_dim
        cl, al = self.critic.layout, self.actor.layout
        # leading dimension of the critic's input tiles: ld(O + A), and beyond 128 floats a multiple of 128, so that the layer-1 dW
        # product (X = these tiles) can read whole 128-column tiles of them on the LDS-DMA loop even when ld(O + A) is not a multiple of
        # the tile (Humanoid: 129 inputs -> ld 160 -> tiles 256 wide; the extra columns are never written and stay zero)
        ld_sa = L.ld(O + A)
        if ld_sa > 128:
            ld_sa = (ld_sa + 127) // 128 * 128
        ws = dict(B=B, ld_sa=ld_sa, ld_o=L.ld(O))
        # Draws and gathered input tiles of the next K steps (K = 1 without the fused draws): `x_sa` / `xn_sa` / `rew` / `done`
        # are slot 0, the tiles of the per-step path.  cfg #2: K = 8 -> 2 x 33.5 MB of tiles.
        want = self._want_ahead()
        K = self._depth if want else 1
        self._ahead = R.DrawAhead(self.gen, dev, B, (B, A), K, R.verified(dev)) if want else None
        self._slot_graphs, self._run_graph = {}, None
        ws["K"] = K
        ws["x_sa_all"] = torch.zeros((K, B, ws["ld_sa"]), **f)
        ws["xn_sa_all"] = torch.zeros((K, B, ws["ld_sa"]), **f)
        ws["rew_all"] = torch.zeros((K, B), **f)
        ws["done_all"] = torch.zeros((K, B), **f)
        ws["slots"] = [dict(x_sa=ws["x_sa_all"][k], xn_sa=ws["xn_sa_all"][k], rew=ws["rew_all"][k], done=ws["done_all"][k])
                       for k in range(K)]
        if self._per is not None:
            # prioritized replay: the rows, importance weights and their per-step maxima one sample launch leaves for the K steps of a
            # run, and the |TD| each step leaves for the run's one write-back
            ws["per_idx_all"] = torch.zeros((K, B), dtype=torch.int64, device=dev)
            ws["w_all"], ws["wmax_all"], ws["abs_td_all"] = torch.zeros((K, B), **f), torch.zeros(K, **f), torch.zeros((K, B), **f)
            for k, slot in enumerate(ws["slots"]):
                slot.update(per_idx=ws["per_idx_all"][k], w=ws["w_all"][k], wmax=ws["wmax_all"][k:k + 1], abs_td=ws["abs_td_all"][k])
        ws.update(ws["slots"][0])
        ws["xn_obs"] = torch.zeros((B, ws["ld_o"]), **f)
        ws["idx"] = torch.zeros(B, dtype=torch.int64, device=dev)
        ws["draw"] = torch.zeros((B, A), **f)
        ws["acts_a"] = torch.empty(al.acts_floats(B), **f)
        # The target policy does not change between two hand-offs (pql_v_learner.py:117-122 is the only place the reference assigns
        # it), its inputs for the next K steps are the tiles gathered ahead and its noise the draws made ahead: the K steps' target
        # actions come from ONE forward launch over K x B rows at prefetch time (64-row tiles on every CU, one launch's fixed cost
        # instead of K) and the step itself starts at the target critic (algo.actor_ahead).
        ws["actor_ahead"] = bool(want and K > 1 and _cfg_get(self.cfg.algo, "actor_ahead", True))
        if ws["actor_ahead"]:
            ws["a_out_all"] = torch.empty((K * B, L.ld(A)), **f)
        ws["acts_t"] = torch.empty(cl.acts_floats(B), **f)
        ws["acts_c"] = torch.empty(cl.acts_floats(B), **f)
        ws["dy"] = torch.zeros((2, B, cl.ld_out), **f)
        ws["grads"] = torch.zeros(cl.total, **f)
        ws["splits"] = default_splits(B, _cfg_get(self.cfg.algo, "dw_splits", 16))
        ws["bwd"] = torch.empty(cl.bwd_ws_floats(B, ws["splits"]), **f)
        ws["scratch"] = torch.zeros(2048, **f)
        # scalar twin heads: TD target + MSE + dL/dQ are formed inside the head's backward pass (one launch less)
        # (not with prioritized replay: the fused TD heads cannot weight rows, the step takes the separate weighted loss launch)
        ws["td_parts"] = int(L.lib.pqlk_td_head_loss_parts(C.byref(cl.desc), B)) if (self._fold_loss and self._td_in_head and self._per is None
                                                                                      and self.head.kind == "scalar") else 0
        # ... and with the fused forward the head's whole backward runs inside the critic's forward launch, off the activations still
        # in LDS: the head-backward launch and its second read of them disappear (algo.td_in_forward; not with gradient buckets)
        ws["td_fwd"] = 0
        if ws["td_parts"] > 0 and bool(_cfg_get(self.cfg.algo, "td_in_forward", True)) and self._buckets is None \
                and self.pk_critic is not None and self.pk_critic.tensor is not None:
            ws["td_fwd"] = int(L.lib.pqlk_td_forward_loss_parts(C.byref(cl.desc), B))
            if ws["td_fwd"] > 0:
                ws["td_parts"] = ws["td_fwd"]
        if ws["td_parts"] > ws["scratch"].numel():   # (batches past 65 536: one loss partial per row tile and net)
            ws["scratch"] = torch.zeros(ws["td_parts"], **f)
        if self._buckets is not None:
            ws["bucket_views"] = [DP.bucket_views(ws["grads"], cl, hi, lo) for hi, lo in self._buckets]
        self._ws = ws
        self.repack()
        return ws

    def _want_ahead(self):
        """Fused draws + batched gather: needs the fused actor forward (it reads norm(next_obs) out of the target critic's input
        tile, so a step's inputs are exactly two tiles), draws outside the graphs, and torch's numbers reproduced on this device."""
        return self._actor_in_sa() and super()._want_ahead()

    def repack(self):
        """Re-derive the fragment-ordered weight copies from the arenas (after loading a state_dict etc.)."""
        if self._fused:
            self.pk_critic.refresh(self.critic.arena.data)
            self.pk_target.refresh(self.critic_target.arena.data)
            if self.pk_actor is not None:
                self.pk_actor.refresh(self.actor.arena.data)
            if self._bf16:
                self._repack_bf16()

    def _gather(self, ws, idx, rows, x_sa, xn_sa, rew, done):
        """Fused replay gather (+ normalise + concat) of `rows` samples into the given tiles."""
        mean, var, eps = self._norm_ptrs()
        # the fused actor forward masks everything past column O while staging its tile, so it can read norm(next_obs)
        # straight out of the target critic's input tile: one gather output (B x ld(O) floats) less to write
        actor_in_sa = self._actor_in_sa()
        L.check(L.lib.pqlk_replay_gather_fused(C.byref(self.memory.ring.desc), L.ptr(idx), rows, L.ptr(mean), L.ptr(var), eps, GATHER_FLAGS,
                                               L.ptr(x_sa), ws["ld_sa"], L.ptr(xn_sa), None if actor_in_sa else L.ptr(ws["xn_obs"]),
                                               ws["ld_o"], L.ptr(rew), L.ptr(done), L.stream(self.device)))

    def _prefetch(self, ws, steps=None):
        """Draws of the next K steps in one launch (torch's own numbers, pql_amd/utils/rng.py) and ONE gather of their K x B
        rows: the ring does not change between two `update()` calls, so what the reference samples at the start of each of
        those steps (simple_replay.py:85-104) can be fetched together -- 102 MB per launch at cfg #2 instead of eight
        latency-bound 12.75-MB launches.  `steps` < K (learn_many of a partial run): only that many steps' draws, rows and
        target actions -- the rest would be dropped unused at the next `update()`."""
        K, B = ws["K"], ws["B"]
        Kp = K if steps is None else max(1, min(K, int(steps)))
        idx = self._ahead.idx
        if self._per is not None:
            # the run's rows come from the tree as it stands now, after the last run's |TD| went in: uniform draws in [0, 2^24) (the
            # same randint consumption per step as the plain learner's) -> Kp stratified batches and their weights in one launch
            self.flush_priorities()
            self._ahead.refill(1 << 24, Kp)
            idx = self._per_draw(ws, self._ahead.idx, Kp)
        else:
            self._ahead.refill(self.memory.cur_capacity, Kp)
        self._gather(ws, idx, Kp * B, ws["x_sa_all"], ws["xn_sa_all"], ws["rew_all"], ws["done_all"])
        if ws["actor_ahead"]:   # a' = clamp(tanh(actor(s')) + clamp(0.8 N(0,1), +-0.2), +-1) of all K steps -> action columns of their tiles
            algo, O = self.cfg.algo, self.memory.ring.O
            xn = ws["xn_sa_all"].view(K * B, ws["ld_sa"])[: Kp * B]
            draws = self._ahead.normal.view(K * B, -1)[: Kp * B]
            if self._bf16:
                mlp_forward_bf16_raw(self.actor.layout, self.actor.arena.data, self.pk_actor_bf16, xn, L.ACT_TANH_NOISE, draws,
                                     algo.noise.tgt_pol_std, algo.noise.tgt_pol_noise_bound, ws["a_out_all"], xn[:, O:])
            else:
                mlp_forward_raw(self.actor.layout, self.actor.arena.data, xn, L.ACT_TANH_NOISE, draws,
                                algo.noise.tgt_pol_std, algo.noise.tgt_pol_noise_bound, ws["a_out_all"], xn[:, O:], packed=self.pk_actor,
                                stash_all=L.STASH_OUTPUT_ONLY)
        self._ahead_stamp = self._data_stamp()

    def _per_draw(self, ws, r, steps):
        """`steps` prioritized batches from the draws `r` (steps x B integers below 2^24) into the first slots' rows / weights; beta
        is the schedule's value at this learner's step count, one value per launch (host side, outside every graph)."""
        beta = per_beta(self._per.beta0, int(self._per.beta_iters), self.update_count)
        self.memory.draw_steps(r, ws["B"], steps, beta, ws["per_idx_all"], ws["w_all"], ws["wmax_all"])
        return ws["per_idx_all"]

    def flush_priorities(self):
        """Write the |TD| of the steps taken since the last write-back into the tree (one `pqlk_per_update` over their n x B rows: a
        row drawn twice keeps the larger candidate), eagerly on this learner's stream.  Runs before the next sample launch, before the
        ring insert of `update()` (a sampled row the insert overwrites must end with pmax^alpha, not with the old row's |TD|), when
        what was prepared ahead is dropped, and before the state is saved."""
        n, self._per_pending = self._per_pending, 0
        if n > 0:
            with torch.cuda.device(self.device), self._on_stream():
                self.memory.update_priorities(self._ws["per_idx_all"][:n], self._ws["abs_td_all"][:n])

    def _drop_ahead(self):
        self.flush_priorities()
        super()._drop_ahead()

    def _after_step(self, ws, slot):
        if self._diag is not None:   # the tiles the weights were last trained on (a per-step or injected step: slot 0's)
            self._diag_slot = 0 if slot is None else slot
        if self._per is None:
            return
        if slot is not None:   # a slot of the run: its |TD| waits with the run's others
            self._per_pending = slot + 1
        else:                  # a per-step or injected step: sampled from the live tree, written back at once
            self._per_pending = 1
            self.flush_priorities()

    def _step_kernels(self, ws, idx, draw, upto_backward=False, tiles=None, part=None):
        """The launch sequence of one critic gradient step; everything asynchronous on the current stream.
        upto_backward=True stops after the gradient is formed (graph capture around the DP all-reduce).
        tiles: input tiles already gathered by `_prefetch` (a slot of ws["slots"]); None = gather `idx` into slot 0 here.
        part (data-parallel buckets, graph capture): only the forward passes + bucket 0 (part = 0) or bucket `part` of the
        backward, no collective."""
        algo, dev, B = self.cfg.algo, self.device, ws["B"]
        O = self.memory.ring.O
        st = L.stream(dev)
        actor_in_sa = self._actor_in_sa()
        tiles_ahead = tiles is not None
        if tiles is None:
            tiles = ws["slots"][0]
            if part in (None, 0):
                if self._per is not None:   # (per-step path: `_draws` / `_learn_injected` left the rows in slot 0)
                    idx = tiles["per_idx"]
                self._gather(ws, idx, B, tiles["x_sa"], tiles["xn_sa"], tiles["rew"], tiles["done"])
        ws = dict(ws, **tiles)   # the step below reads its inputs from `tiles`
        al, cl = self.actor.layout, self.critic.layout
        gamma_n = float(algo.gamma) ** int(algo.nstep)
        # single GPU: the loss fold and the gradient-norm pass ride in launches that exist anyway (backward's slab
        # reduction, the optimiser); data parallel keeps them apart because the all-reduce sits in between
        tail = self._fused_tail
        if part in (None, 0):
            # target policy smoothing (:63-71): a' written into the action columns of the target critic's input.
            # The two no-grad chains (actor, target critic) skip the activation stash; the critic keeps it for backward.
            xn_act = ws["xn_sa"][:, O:]
            if tiles_ahead and ws["actor_ahead"]:   # (tiles gathered ahead already hold a': _prefetch)
                pass
            elif self._bf16:   # (acts_a: only its first B x ld(A) floats, the output block, are written)
                mlp_forward_bf16_raw(al, self.actor.arena.data, self.pk_actor_bf16, ws["xn_sa"], L.ACT_TANH_NOISE, draw, algo.noise.tgt_pol_std,
                                     algo.noise.tgt_pol_noise_bound, ws["acts_a"], xn_act)
            else:
                mlp_forward_raw(al, self.actor.arena.data, ws["xn_sa"] if actor_in_sa else ws["xn_obs"], L.ACT_TANH_NOISE, draw, algo.noise.tgt_pol_std,
                                algo.noise.tgt_pol_noise_bound, ws["acts_a"], xn_act, packed=self.pk_actor, stash_all=False)
            if self._bf16:   # the target Q lands where the loss / the TD head read it: the output block of the target's stash
                mlp_forward_bf16_raw(cl, self.critic_target.arena.data, self.pk_target_bf16, ws["xn_sa"], L.ACT_NONE,
                                     out=output_view(cl, ws["acts_t"], B))
            else:
                mlp_forward_raw(cl, self.critic_target.arena.data, ws["xn_sa"], L.ACT_NONE, acts=ws["acts_t"], packed=self.pk_target,
                                stash_all=False)
            if ws["td_fwd"] > 0:
                L.check(L.lib.pqlk_mlp_forward_td(C.byref(cl.desc), L.ptr(self.critic.arena.data), L.ptr(self.pk_critic.tensor), L.ptr(ws["x_sa"]),
                                                  ws["ld_sa"], B, L.ptr(ws["acts_c"]), L.ptr(ws["acts_t"]), L.ptr(ws["rew"]), L.ptr(ws["done"]),
                                                  gamma_n, L.ptr(ws["scratch"]), L.ptr(ws["bwd"]), ws["bwd"].numel(), ws["splits"], st))
            else:
                mlp_forward_raw(cl, self.critic.arena.data, ws["x_sa"], L.ACT_NONE, acts=ws["acts_c"], packed=self.pk_critic,
                                stash_all=True)
            if ws["td_parts"] == 0:
                q = output_view(cl, ws["acts_c"], B)
                qt = output_view(cl, ws["acts_t"], B)
                # (with prioritized replay: importance weights on the loss and its gradient; |TD| -> the slot's slab)
                per = None if self._per is None else (ws["w"], ws["wmax"], ws["abs_td"])
                self.head.critic_loss(q, qt, cl.ld_out, ws["rew"], ws["done"], gamma_n, B, ws["dy"], None if self._fold_loss else self.loss_ring,
                                      self.opt.step, ws["scratch"], self.device, per=per, kappa=float(_cfg_get(algo, "huber_kappa", 1.0)))
        if self._buckets is not None:
            # data parallel: the chain in pieces, each ending with the sum of its layers' dW slabs; that piece's collective goes
            # out right behind it and runs under the launches of the layers below
            td = ws["td_parts"] > 0
            for k, (hi, lo) in enumerate(self._buckets):
                if part is not None and part != k:
                    continue
                L.check(L.lib.pqlk_mlp_backward_layers(C.byref(cl.desc), L.ptr(self.critic.arena.data), L.ptr(ws["x_sa"]), ws["ld_sa"], B,
                                                       L.ptr(ws["acts_c"]), None if td else L.ptr(ws["dy"]),
                                                       L.ptr(ws["acts_t"]) if td else None, L.ptr(ws["rew"]) if td else None,
                                                       L.ptr(ws["done"]) if td else None, gamma_n, L.ptr(ws["scratch"]) if td else None,
                                                       L.ptr(ws["grads"]), ws["splits"], L.ptr(ws["bwd"]), ws["bwd"].numel(), hi, lo, st))
                if part is None:
                    self._reducer.issue(ws["bucket_views"][k])
            if part is not None:
                return
            self._reducer.wait()
            self._step_post(ws)
            return
        if ws["td_fwd"] > 0:
            L.check(L.lib.pqlk_mlp_backward_td_tail(C.byref(cl.desc), L.ptr(self.critic.arena.data), L.ptr(ws["x_sa"]), ws["ld_sa"], B,
                                                    L.ptr(ws["acts_c"]), L.ptr(ws["grads"]), ws["splits"], L.ptr(ws["bwd"]), ws["bwd"].numel(),
                                                    L.ptr(self.opt.scratch) if tail else None, L.ptr(self.opt.step) if tail else None, st))
        elif ws["td_parts"] > 0:
            L.check(L.lib.pqlk_mlp_backward_td(C.byref(cl.desc), L.ptr(self.critic.arena.data), L.ptr(ws["x_sa"]), ws["ld_sa"], B,
                                               L.ptr(ws["acts_c"]), L.ptr(ws["acts_t"]), L.ptr(ws["rew"]), L.ptr(ws["done"]), gamma_n,
                                               L.ptr(ws["scratch"]), L.ptr(ws["grads"]), ws["splits"], L.ptr(ws["bwd"]),
                                               ws["bwd"].numel(), L.ptr(self.opt.scratch) if tail else None,
                                               L.ptr(self.opt.step) if tail else None, st))
        elif tail:
            L.check(L.lib.pqlk_mlp_backward_norm(C.byref(cl.desc), L.ptr(self.critic.arena.data), L.ptr(ws["x_sa"]), ws["ld_sa"], B,
                                                 L.ptr(ws["acts_c"]), L.ptr(ws["dy"]), L.ptr(ws["grads"]), ws["splits"], None, 0, 0,
                                                 0, None, 0, L.ptr(ws["bwd"]), ws["bwd"].numel(), L.ptr(self.opt.scratch),
                                                 L.ptr(self.opt.step), st))
        else:
            mlp_backward_raw(cl, self.critic.arena.data, ws["x_sa"], ws["acts_c"], ws["dy"], ws["bwd"], ws["grads"], ws["splits"])
        if upto_backward:
            return
        self._allreduce_grads(ws)
        self._step_post(ws)

    def _probe(self):
        """The diagnostics of the weights about to be handed out, on the tiles of the last step they took: one fp32 per-layer forward
        of the critic with its full stash (the last hidden layer is never stashed by the training step's own fused forward), one of
        the target critic on that step's xn_sa tile (its action columns hold a' in every mode), the two reductions.  Eager, on this
        learner's stream, under its lock; writes only the probe's own buffers."""
        d, ws, cl = self._diag, self._ws, self.critic.layout
        B, tiles = ws["B"], ws["slots"][self._diag_slot]
        if "diag_acts" not in ws:
            ws["diag_acts"] = [torch.empty(cl.acts_floats(B), dtype=torch.float32, device=self.device) for _ in range(2)]
        acts_c, acts_t = ws["diag_acts"]
        mlp_forward_raw(cl, self.critic.arena.data, tiles["x_sa"], L.ACT_NONE, acts=acts_c, stash_all=True)
        mlp_forward_raw(cl, self.critic_target.arena.data, tiles["xn_sa"], L.ACT_NONE, acts=acts_t, stash_all=True)
        gamma_n = float(self.cfg.algo.gamma) ** int(self.cfg.algo.nstep)
        d.critic_stats(output_view(cl, acts_c, B), output_view(cl, acts_t, B), cl.ld_out, tiles["rew"], tiles["done"], gamma_n, B)
        for net in range(2):
            for layer in range(cl.n_layers - 1):
                off, ld = cl.act_offset(B, net, layer)
                d.unit_stats(net, layer, acts_c[off:], ld, B, cl.dims[layer + 1])
        d.ship()

    def diagnostics(self):
        """The `diag/*` values of the last probe whose copy has reached the host: {} when algo.diag.enabled is off or before the
        first one lands.  Never synchronises.  They describe the weights handed out at that hand-off on the last batch they were
        trained on (the TD residual is that batch's after its step); under data parallel this rank's own shard."""
        if self._diag is None:
            return {}
        with self._lock:
            return self._diag.diagnostics()

    def _step_post(self, ws):
        self._optimizer(ws)
        if self._bf16:   # the Polyak step moved the target: its bf16 copy follows in one launch, inside the captured step
            self.pk_target_bf16.refresh(self.critic_target.arena.data)

    def _optimizer(self, ws):
        algo, dev = self.cfg.algo, self.device
        if self._fold_loss:
            apply_optimizer_fused(self.critic.layout, self.critic.arena.data, ws["grads"], self.opt, self.critic_target.arena.data,
                                  algo.critic_lr, algo.max_grad_norm, algo.tau, self.pk_critic, self.pk_target, ws["scratch"],
                                  ws["td_parts"] or self.head.loss_parts(ws["B"]), self.head.critic_scale(ws["B"]),
                                  self.loss_ring, dev, norm_in_backward=self._fused_tail, grad_scale=1.0 / self.world)
            return
        # optimiser + Polyak + refresh of the fragment-ordered weight copies (critic and target) in one launch pair
        apply_optimizer(self.critic.arena.data, ws["grads"], self.opt, self.critic_target.arena.data, algo.critic_lr,
                        algo.max_grad_norm, algo.tau, 1.0 / self.world, dev, layout=self.critic.layout,
                        packed=self.pk_critic, packed_target=self.pk_target)

    def _draws(self, ws):
        # RNG consumption order of the reference: one randint(cur_capacity,(B,)) then one
        # N(0,1) draw of shape (B, A) on the learner's device generator.
        # (prioritized: the same one randint, over [0, 2^24), turned into a stratified batch from the live tree)
        torch.randint(self._randint_bound(), (ws["B"],), generator=self.gen, out=ws["idx"])   # straight into the workspace: no copy launch
        ws["draw"].normal_(generator=self.gen)
        if self._per is not None:
            self._per_draw(ws, ws["idx"], 1)

    def _randint_bound(self):
        return self.memory.cur_capacity if self._per is None else 1 << 24

    def _step(self, ws, slot=None, upto_backward=False, part=None):
        """The step on the draws / tiles `_prefetch` left in `slot`; None = on the per-step draws in ws["idx"] / ws["draw"]."""
        if slot is None:
            self._step_kernels(ws, ws["idx"], ws["draw"], upto_backward, part=part)
        else:
            self._step_kernels(ws, None, self._ahead.normal[slot], upto_backward, tiles=ws["slots"][slot], part=part)

    def learn(self, indices=None, noise=None):
        """One critic gradient step.  `indices` (B,) int64 and `noise` (B,A) N(0,1) draws may be injected
        for parity tests; otherwise they are drawn exactly like the reference draws them."""
        return self._learn(None if indices is None and noise is None else (indices, noise))

    def _learn_injected(self, ws, injected, home):
        indices, noise = injected
        if indices is None or noise is None:
            self._drop_ahead()   # the generator is about to be used directly: what was drawn ahead is off the stream now
        if indices is not None:
            self._inject(ws["idx"], indices, home)
            if self._per is not None:   # injected rows: their weights at this step's beta
                ws["per_idx_all"][0].copy_(ws["idx"])
                self.memory.beta = per_beta(self._per.beta0, int(self._per.beta_iters), self.update_count)
                w, wmax = self.memory.weights_for(ws["per_idx_all"][0])
                ws["w_all"][0].copy_(w)
                ws["wmax_all"][:1].copy_(wmax)
        else:
            torch.randint(self._randint_bound(), (ws["B"],), generator=self.gen, out=ws["idx"])
            if self._per is not None:
                self._per_draw(ws, ws["idx"], 1)
        if noise is not None:
            self._inject(ws["draw"], noise, home)
        else:
            ws["draw"].normal_(generator=self.gen)
        self._step_kernels(ws, ws["idx"], ws["draw"])

    def training_state(self):
        with self._lock:
            if self._per_pending:   # the saved leaves hold every step taken so far
                self.flush_priorities()
                self.synchronize()
            return super().training_state()

    def _own_state(self):
        return {"critic": _cpu(self.critic.arena.data), "critic_target": _cpu(self.critic_target.arena.data),
                "actor": None if self.actor is None else _cpu(self.actor.arena.data),   # lags the live policy by design
                "memory": self.memory.training_state()}   # (the ring's header; the rows: `memory.rows()`)

    def _load_own_state(self, st, memory):
        self.critic.arena.data.copy_(st["critic"])
        self.critic_target.arena.data.copy_(st["critic_target"])
        self._load_partner(st["actor"], make_actor)
        self._per_pending = 0   # (|TD| of steps taken before the load does not belong to the loaded tree)
        if memory:
            self.memory.load_training_state(st["memory"])

    def set_actor(self, actor, home=None):
        self._adopt_partner(actor, home)
        if self._bf16:
            self._repack_bf16()

    @torch.no_grad()
    def update(self, actor, trajectory, normalize_tuple, sleep_time):
        """pql_v_learner.py:117-122.  Everything is enqueued on this learner's stream behind event fences
        (pql_amd.utils.handoff): the stream waits for the producers of `actor`, `trajectory` and the statistics, the
        producers' buffers are released when the copies / the ring insert have read them, and the critic handed back
        is a snapshot (double-buffered) that later optimiser steps do not touch."""
        home = torch.cuda.current_stream(self.device)   # the caller's stream, before we switch to ours
        with self._lock, torch.cuda.device(self.device), self._on_stream():
            st = torch.cuda.current_stream(self.device)
            if self._diag is not None and self._diag.due() and self._diag_slot is not None and self._ws is not None:
                self._probe()   # before the actor, the ring and the statistics move: the batch is the one the weights last saw
            self._diag_slot = None
            self.set_actor(actor, home)
            self.flush_priorities()   # before the insert: a sampled row it overwrites must end with pmax^alpha
            with H.LOCK:
                lease = H.acquire(trajectory, st, home)
                self.memory.add_to_buffer(trajectory)
                H.release(lease, st)
            self.normalize_tuple = resident_norm(self, normalize_tuple, home)
            self._drop_ahead()   # ring contents, the randint bound and the statistics changed: later steps sample afresh
            loss = self._lagged.poll(self.update_count)
            self.sleep_time = sleep_time
            return self._published(), loss, self.update_count


def asyn_v_learner(learner, cfg, stop_event=None, max_in_flight=2):
    """Free-running pump (reference: a Ray task looping forever, :136-141).  Run it in a thread."""
    pump(learner, stop_event, max_in_flight)
