"""What the V-learner and the P-learner share: the helpers around a gradient step (the baseline agents use them too) and the
base class `Learner` -- everything around a learner's launch sequence: the stream, the lock and the private generator, the
draws made ahead, hipGraph capture and replay (per step, per slot, per run, split around a collective), the loss ring and the
checkpoint state.  The launch sequences themselves are pql_amd/algo/pql_v_learner.py and pql_amd/algo/pql_p_learner.py.
"""
from __future__ import annotations

import contextlib
import functools
import os
import ctypes as C
import threading
import time
from collections import deque
from copy import deepcopy

import torch

from pql_amd import _lib as L
from pql_amd.models import model_name_to_path
from pql_amd.models.mlp import PackedWeights
from pql_amd.replay.prioritized_replay import per_cfg, per_refresh
from pql_amd.utils import dp as DP
from pql_amd.utils import handoff as H
from pql_amd.utils import rng as R
from pql_amd.utils.common import Tracker, load_class_from_path

LOSS_RING = 5  # Tracker(5) of the reference (:54)
# gather: +-5 clamp (bit 0); the learners' input tiles are allocated zeroed and nothing else writes their pad columns (bit 1)
# (PQL_GATHER_FLAGS: A/B switch for the launch-shape / cache-policy bits of include/pqlk.h, tools/ab_bench.sh)
GATHER_FLAGS = int(os.environ.get("PQL_GATHER_FLAGS", L.GATHER_CLAMP5 | L.GATHER_PADS_ZERO))
# From this bound on torch.randint draws 64-bit indices (another Philox consumption per sample), which the draws made ahead
# (pql_amd/utils/rng.py) do not reproduce: a ring that large takes the per-step torch draws.
DRAWS_AHEAD_BOUND = 1 << 28


def _cfg_get(node, name, default=None):
    try:
        v = getattr(node, name)
    except (AttributeError, KeyError):
        return default
    return default if v is None else v


class _AdamState:
    """m, v, step counter and scratch for one parameter arena."""

    def __init__(self, arena: torch.Tensor):
        self.m = torch.zeros_like(arena)
        self.v = torch.zeros_like(arena)
        self.step = torch.zeros(1, dtype=torch.int32, device=arena.device)
        self.gnorm = torch.zeros(1, dtype=torch.float32, device=arena.device)
        self.scratch = torch.zeros(2048, dtype=torch.float32, device=arena.device)


def apply_optimizer(arena, grads, st: _AdamState, target, lr, max_grad_norm, tau, grad_scale=1.0, device=None, layout=None,
                    packed=None, packed_target=None):
    """clip_grad_norm_ + AdamW(torch defaults: betas .9/.999, eps 1e-8, wd 1e-2) + optional Polyak.
    With `layout` + `packed` (PackedWeights with a tensor) the same launch also refreshes the fragment-ordered weight
    copies of the fused forward path."""
    mn = float(max_grad_norm) if max_grad_norm is not None else 0.0
    if layout is not None and packed is not None and packed.tensor is not None:
        pt = packed_target.tensor if packed_target is not None else None
        L.check(L.lib.pqlk_clip_adamw_polyak_pack(C.byref(layout.desc), L.ptr(arena), L.ptr(grads), L.ptr(st.m), L.ptr(st.v),
                                                  L.ptr(target), L.ptr(packed.tensor), L.ptr(pt), float(grad_scale), mn, float(lr),
                                                  0.9, 0.999, 1e-8, 1e-2, float(tau), L.ptr(st.step), L.ptr(st.gnorm),
                                                  L.ptr(st.scratch), L.stream(device)))
        return
    L.check(L.lib.pqlk_clip_adamw_polyak(L.ptr(arena), L.ptr(grads), L.ptr(st.m), L.ptr(st.v), L.ptr(target),
                                         arena.numel(), float(grad_scale), mn, float(lr), 0.9, 0.999, 1e-8, 1e-2, float(tau),
                                         L.ptr(st.step), L.ptr(st.gnorm), L.ptr(st.scratch), L.stream(device)))


def apply_optimizer_fused(layout, arena, grads, st: _AdamState, target, lr, max_grad_norm, tau, packed, packed_target,
                          loss_part, loss_parts, loss_scale, loss_ring, device, norm_in_backward=True, grad_scale=1.0):
    """Tail of a fused learner step: AdamW (+ Polyak + re-pack) whose launch also folds the loss partials into the loss ring.
    norm_in_backward (single GPU): the squared-norm partials and the step increment were left in `st.scratch` / `st.step` by
    `pqlk_mlp_backward_norm` -- same bits as apply_optimizer + the stand-alone folds, two launches fewer.  Data parallel
    (norm_in_backward=False, grad_scale = 1 / world): the norm pass runs here, on the all-reduced gradient; one launch fewer."""
    mn = float(max_grad_norm) if max_grad_norm is not None else 0.0
    pk = packed.tensor if packed is not None else None
    pt = packed_target.tensor if packed_target is not None else None
    L.check(L.lib.pqlk_adamw_polyak_fused(C.byref(layout.desc), L.ptr(arena), L.ptr(grads), L.ptr(st.m), L.ptr(st.v), L.ptr(target),
                                          L.ptr(pk), L.ptr(pt), float(grad_scale), mn, float(lr), 0.9, 0.999, 1e-8, 1e-2, float(tau),
                                          L.ptr(st.step), L.ptr(st.gnorm), L.ptr(st.scratch),
                                          int(L.lib.pqlk_mlp_norm_parts(C.byref(layout.desc))) if norm_in_backward else 0,
                                          L.ptr(loss_part), int(loss_parts),
                                          float(loss_scale), L.ptr(loss_ring), LOSS_RING, L.stream(device)))


def qr_drop(algo):
    """`algo.qr_drop` as the loss entries take it: None (the key absent or null: one whole target net per row) or the int d."""
    d = _cfg_get(algo, "qr_drop", None)
    return None if d is None else int(d)


def qr_targets(algo, n):
    """Target atoms a quantile head of n quantiles is regressed on per row, the divisor of its loss: n, or 2 (n - algo.qr_drop)."""
    d = qr_drop(algo)
    return int(n) if d is None else 2 * (int(n) - d)


def distl_loss(algo):
    """`algo.distl_loss`, the law the categorical head is trained with: "c51" (also for a config without the key) or "hl_gauss"."""
    return str(_cfg_get(algo, "distl_loss", "c51"))


def hl_sigma(algo):
    """`algo.hl_sigma` as the HL-Gauss entries take it: sigma in bin widths (0.75 for a config without the key)."""
    return float(_cfg_get(algo, "hl_sigma", 0.75))


def f32_recip(*factors, sign=1.0):
    """sign / (f0 * f1 ...) evaluated in fp32, like the kernels' `1.0f / ((float)b * (float)k)`."""
    import numpy as np
    d = np.float32(1.0)
    for f in factors:
        d = np.float32(d * np.float32(f))
    return float(np.float32(sign) / d)


def allreduce_sum(t, pg):
    """Sum-all-reduce of the flat gradient arena.  RCCL ("nccl") reduces in place on the device over xGMI; the
    gloo rehearsal path (CPU tests / one-GPU dry runs) stages through host memory."""
    if torch.distributed.get_backend(pg) == "gloo" and t.is_cuda:
        h = t.cpu()
        torch.distributed.all_reduce(h, group=pg)
        t.copy_(h)
    else:
        torch.distributed.all_reduce(t, group=pg)


class LaggedLoss:
    """Mean of the last LOSS_RING losses without stalling the stream: each call enqueues an async copy of the
    device ring to pinned host memory and returns the value of the last copy that has completed (one hand-off
    behind).  Replaces the reference's per-step `loss.item()` + Tracker(5) (pql_v_learner.py:111)."""

    def __init__(self, ring: torch.Tensor):
        self.ring = ring
        self.host = torch.zeros(ring.numel(), dtype=torch.float32).pin_memory()
        self.event = None
        self.count_at_copy = 0
        self.value = 0.0

    @staticmethod
    def mean_of(vals, count):
        n = min(count, LOSS_RING)
        window = [vals[t % LOSS_RING] for t in range(count - n, count)]
        return float(sum(window) / LOSS_RING)   # Tracker(5) is zero-filled: always divides by its length

    def poll(self, count):
        if self.event is not None and self.event.query():
            self.value = self.mean_of(self.host.tolist(), self.count_at_copy)
            self.event = None
        if self.event is None:
            self.host.copy_(self.ring, non_blocking=True)
            self.event = torch.cuda.Event()
            self.event.record()
            self.count_at_copy = count
        return self.value


def graph_collective_enabled(pg):
    """PQL_DP_GRAPH_COLLECTIVE=1 captures the gradient all-reduce inside the learner's hipGraph.  Only RCCL can be
    captured (the gloo rehearsal path stages through the host); rehearsed with a 1-rank group only -- unverified for
    world > 1, scaling was not measurable on this pool."""
    if os.environ.get("PQL_DP_GRAPH_COLLECTIVE", "0") != "1":
        return False
    if torch.distributed.get_backend(pg) != "nccl":
        raise L.PqlkError("PQL_DP_GRAPH_COLLECTIVE=1 needs the RCCL ('nccl') backend: a gloo all-reduce cannot be graph-captured")
    return True


def _norm_buffers(owner, mean, var):
    """The (mean, var) buffers that live as long as `owner`, allocated when absent or of another width."""
    cur = getattr(owner, "_norm_buf", None)
    if cur is None or cur[0].shape != mean.reshape(-1).shape:
        cur = (torch.empty(mean.numel(), dtype=torch.float32, device=owner.device),
               torch.empty(var.numel(), dtype=torch.float32, device=owner.device))
        owner._norm_buf = cur
    return cur


def resident_norm(owner, normalize_tuple, home=None):
    """Copy (mean, var, eps) into buffers that live as long as the learner, so kernels (and captured
    graphs) always read the same addresses; the producer may hand over fresh tensors every iteration.
    Runs on the learner's stream (current), fenced against the stream the tensors were produced on."""
    if normalize_tuple is None:
        return None
    mean, var, eps = normalize_tuple
    cur = _norm_buffers(owner, mean, var)
    st = torch.cuda.current_stream(owner.device)
    for dst, src in zip(cur, (mean, var)):
        with H.LOCK:
            lease = H.acquire(src, st, home)
            dst.copy_(src.reshape(-1), non_blocking=True)
            H.release(lease, st)
    return cur[0], cur[1], float(eps)


def adopt_arena(dst_module, src_module, device, home=None, pipe="params"):
    """Fenced copy of `src_module`'s flat arena into `dst_module`'s on the CURRENT stream of `device`: waits for the
    producer (a published snapshot's event, or the caller's stream for a plain module) and releases the source
    afterwards.  From another GPU the bytes first land in a double-buffered block through the copy streams (peer copy
    over xGMI), so the learner's compute stream only ever does the local arena copy."""
    st = torch.cuda.current_stream(device)
    with H.LOCK:
        if H.crosses(src_module.arena.device, device):
            blk = H.shipper(src_module.arena.device, device, pipe).ship((src_module.arena.data,), H.lease_of(src_module))
            lease = H.acquire(blk, st)
            dst_module.arena.data.copy_(blk[0], non_blocking=True)
        else:
            lease = H.acquire(src_module, st, home)
            dst_module.arena.data.copy_(src_module.arena.data, non_blocking=True)
        H.release(lease, st)


def pump(learner, stop_event=None, max_in_flight=2):
    """Free-running learner loop shared by asyn_v_learner / asyn_p_learner.  The host enqueues a step in ~15 us and the
    GPU takes ~0.7 ms to run it, so without back-pressure the queue would run thousands of steps ahead of the device and
    every `update()` would land behind them: at most `max_in_flight` steps are kept enqueued (event wait, GIL released)."""
    pending = deque()
    while stop_event is None or not stop_event.is_set():
        if not learner.ready_to_learn():
            time.sleep(0.0005)
            continue
        sleep_time = learner.learn()
        pending.append(learner.fence())
        while len(pending) > max_in_flight:
            pending.popleft().synchronize()
        if sleep_time:
            time.sleep(sleep_time)
    while pending:
        pending.popleft().synchronize()


def check_per_refresh(cfg, where):
    """The synchronous baselines sample from the live tree every step: `algo.per.refresh=run` is refused, naming the key."""
    per = per_cfg(cfg.algo)
    if per is not None and per_refresh(per) != "step":
        raise ValueError(f"algo.per.refresh=run cannot run in {where}: it samples from the live tree and writes priorities back every step "
                         f"(algo.per.refresh=step); run is the PQL V-learner's mode (scripts/train_pql.py)")


def make_actor(cfg, obs_dim, action_dim, device):
    """The policy `cfg.algo` names, freshly initialised on `device`."""
    act_class = load_class_from_path(cfg.algo.act_class, model_name_to_path[cfg.algo.act_class])
    hidden = _cfg_get(cfg.algo, "hidden_layers")
    hidden = list(hidden) if hidden is not None else None
    with torch.cuda.device(device):
        return act_class(obs_dim, action_dim, hidden_layers=hidden).to(device)


ARTIFACT_ERROR = "W&B artifact download is out of scope (no network); load a local state_dict instead"


def load_artifact(path, actor=None, critic=None, obs_rms=None):
    """`cfg.artifact` as a local warm start: a file in the reference's checkpoint format (what `Evaluator` writes as
    model.pth, pql_amd.utils.model_util) -> the given modules.  Anything that is not an existing file is a W&B artifact name."""
    import os
    from pql_amd.utils.model_util import load_model
    if not os.path.isfile(str(path)):
        raise NotImplementedError(ARTIFACT_ERROR)
    if actor is not None:
        load_model(actor, "actor", str(path))
    if critic is not None:
        load_model(critic, "critic", str(path))
    if obs_rms is not None:
        load_model(obs_rms, "obs_rms", str(path))


def _cpu(t):
    return t.detach().cpu()


def adam_state(st):
    return {"m": _cpu(st.m), "v": _cpu(st.v), "step": _cpu(st.step)}


def load_adam_state(st, saved):
    st.m.copy_(saved["m"])
    st.v.copy_(saved["v"])
    st.step.copy_(saved["step"])


def lagged_state(lag):
    """(count, value) a `LaggedLoss` reports once the copy it has in flight has landed (the caller has synchronised)."""
    if lag.event is not None:
        return {"count": int(lag.count_at_copy), "value": LaggedLoss.mean_of(lag.host.tolist(), lag.count_at_copy)}
    return {"count": int(lag.count_at_copy), "value": float(lag.value)}


def load_lagged_state(lag, saved):
    lag.event, lag.count_at_copy, lag.value = None, int(saved["count"]), float(saved["value"])


def norm_state(learner):
    nt = learner.normalize_tuple
    return None if nt is None else (_cpu(nt[0]), _cpu(nt[1]), float(nt[2]))


def load_norm_state(learner, saved):
    """Into the learner's resident buffers (`resident_norm`): captured graphs keep reading the same addresses."""
    if saved is None:
        learner.normalize_tuple = None
        return
    mean, var, eps = saved
    cur = _norm_buffers(learner, mean, var)
    cur[0].copy_(mean.reshape(-1))
    cur[1].copy_(var.reshape(-1))
    learner.normalize_tuple = (cur[0], cur[1], float(eps))


class Learner:
    """Base of PQLVLearner / PQLPLearner.  A subclass trains its own network against a replica of its partner's, and provides
    `_bound` (the randint bound: rows in its ring), `_captured` (the tensors a step writes), `_workspace`, `_data_stamp`, `repack`,
    `_gather`, `_prefetch`, `_step`, `_step_kernels`, `_step_post`, `_draws`, `_learn_injected`, `_own_state`, `_load_own_state`."""

    PARTNER = None                  # "actor" (V) / "critic" (P): the attribute that holds the replica; "pk_" + it = its packed copy
    RESTORE_AFTER_CAPTURE = True    # False (P): after capturing a step, which executes nothing, only the generator is put back

    def __init__(self, obs_dim, action_dim, cfg, device, process_group, model):
        """`model` is built by the subclass BEFORE this runs: its constructor (and a warm start) consume the CPU generator, and
        the device generator's seed below is the next draw from it."""
        self.cfg = cfg
        self.obs_dim = obs_dim
        self.action_dim = int(action_dim)
        self.device = device
        self.pg = process_group  # data-parallel group (RCCL); None = single GPU
        self.world = torch.distributed.get_world_size(process_group) if process_group is not None else 1
        # dp: the collective is issued even for a 1-rank group, so the RCCL path can be rehearsed on one GPU
        self.dp = process_group is not None
        self._buckets = None   # (data-parallel gradient buckets: V-learner)
        setattr(self, self.PARTNER, None)   # the replica and its packed copy arrive with the first update()
        setattr(self, "pk_" + self.PARTNER, None)
        algo = cfg.algo
        self.opt = _AdamState(model.arena.data)
        self._fused = bool(_cfg_get(algo, "fused", True))
        self._fold_loss = bool(_cfg_get(algo, "fused_tail", True))   # loss partials folded by the optimiser launch
        self._fused_tail = not self.dp and self._fold_loss            # ... and the gradient norm's partials by backward's reduction
        self.loss_tracker = Tracker(LOSS_RING)
        self.loss_ring = torch.zeros(LOSS_RING, dtype=torch.float32, device=self.device)
        self._lagged = LaggedLoss(self.loss_ring)
        self.update_count = 0
        self.normalize_tuple = None
        self.use_graph = bool(_cfg_get(algo, "graph", False))
        # RNG draws inside the hipGraph or in front of it.  In front (default): torch hands a captured generator its seed and
        # Philox offset through two 1-element fill launches per replay (~9 us of device time per step, more than the draws save
        # by being captured), and the graph no longer bakes in the randint bound, so it is not re-captured while the ring fills.
        self._graph_rng = bool(_cfg_get(algo, "graph_rng", False))
        # own HIP stream: the MI355X form of the reference's separate learner process (Ray actor).  V-learner,
        # P-learner and rollout queues then overlap on the GPU; hand-offs are event-fenced in update().
        self.stream = torch.cuda.Stream(self.device) if bool(_cfg_get(algo, "streams", False)) else None
        # what start()/update() hand out: double-buffered snapshots of the model (the reference returns a pickled copy
        # through Ray, pql_v_learner.py:59-60,122), so a consumer never reads an arena AdamW is writing and the weights a
        # caller holds are those of the hand-off, not of whenever it gets round to using them
        self._pub = H.ArenaPublisher(model)
        self._lock = threading.RLock()   # learn() / update() are FIFO like calls on a Ray actor
        self._capture_stream = torch.cuda.Stream(self.device)   # torch's default capture stream is shared by every graph
        # Own device generator, like the reference's learner PROCESS has its own default generator.  Not a
        # nicety: every hipGraph that draws from a generator is handed its Philox offset through ONE device word per
        # generator, refreshed on the replaying stream -- two learners replaying graphs on two streams off the shared
        # default generator overwrite each other's offset (measured: different sample indices from run to run).
        self.gen = torch.Generator(device=self.device)
        self.gen.manual_seed(int(torch.randint(0, 2 ** 62, (1,)).item()))   # derived from the driver's seed (CPU generator)
        # algo.rng: "auto" (default) = this library produces the draws itself, `_depth` steps ahead in one launch (V:
        # `algo.prefetch_steps`, P: `algo.prefetch_steps_p`), together with ONE batched replay gather for those steps -- if its
        # numbers are torch's on this device (pql_amd/utils/rng.py), else "torch"; "torch" = one randint (V: + one normal_) ATen
        # launch in front of every step (round 2); "philox" = as auto, but refuse to run when the check fails.
        self._rng_mode = str(_cfg_get(algo, "rng", "auto"))
        if self._rng_mode != "torch":   # the on-device check runs HERE, once, under a lock (not lazily inside the first learn(),
            with torch.cuda.device(self.device):   # which free-running learners reach from two threads at the same time)
                R.verified(self.device)
        self._ahead = None
        self._ahead_stamp = None
        self._ws = None
        self._graph = None
        self._graph_post = None
        self._graph_key = None
        self._slot_graphs = {}
        self._run_graph = None   # all K draws-ahead steps of one run in ONE hipGraph (learn_many)
        self._run_graphs = bool(_cfg_get(algo, "run_graph", True))

    # ------------------------------------------------------------------------------------------
    def start(self):
        with self._lock, torch.cuda.device(self.device), self._on_stream():
            return self._published(), self.update_count, self.loss_tracker.mean()

    def _on_stream(self):
        return torch.cuda.stream(self.stream) if self.stream is not None else contextlib.nullcontext()

    def _published(self):
        """The model as handed to other components: a snapshot taken on this learner's queue."""
        return self._pub.publish()

    def _partner(self):
        return getattr(self, self.PARTNER)

    def ready_to_learn(self):
        return self._partner() is not None

    def use_private_rng(self, seed):
        """Re-seed this learner's generator."""
        self.gen.manual_seed(int(seed))
        self._graph = None
        self._drop_ahead()

    def _drop_ahead(self):
        """Forget the draws / gathered tiles prepared for later steps (the ring, its bound, the statistics or the generator
        changed): the next step prepares them again at the generator's current offset."""
        if self._ahead is not None:
            self._ahead.invalidate()

    def _after_step(self, ws, slot):
        """Called once a step (or, from `learn_many`, a run of steps ending with `slot`) is enqueued; slot None = a per-step or
        injected one.  The V-learner's prioritized replay keeps count of the |TD| slabs that wait for their write-back."""

    def _check_ahead(self):
        if self._ahead is not None and self._ahead.valid and self._ahead_stamp != self._data_stamp():
            self._drop_ahead()

    def _norm_key(self):
        """Part of every graph key: a captured gather has the ADDRESSES of the statistics baked in (update() keeps them stable by
        copying into resident buffers; a tuple assigned from outside brings new ones and must re-capture)."""
        nt = self.normalize_tuple
        return None if nt is None else (nt[0].data_ptr(), nt[1].data_ptr(), float(nt[2]))

    def _norm_ptrs(self):
        if not self.cfg.algo.obs_norm or self.normalize_tuple is None:
            return None, None, 0.0
        mean, var, eps = self.normalize_tuple
        return mean, var, float(eps)

    def _want_ahead(self):
        """Draws made ahead + one batched gather: needs draws outside the graphs, and torch's numbers reproduced on this device."""
        if self._rng_mode == "torch" or self._graph_rng:
            return False
        ok = R.verified(self.device) is not None
        if not ok and self._rng_mode == "philox":
            raise L.PqlkError("algo.rng=philox: pqlk_philox_draws does not reproduce torch.randint / normal_ on this device "
                              "(another torch / rocRAND build?); use algo.rng=auto or torch")
        return ok

    @property
    def rng(self):
        """'philox' when the draws come from this library's launch, 'torch' when from ATen's (see __init__)."""
        return "philox" if self._ahead is not None else "torch"

    def fence(self):
        """Event behind everything enqueued on this learner's queue so far."""
        ev = torch.cuda.Event()
        ev.record(self.stream if self.stream is not None else torch.cuda.current_stream(self.device))
        return ev

    def synchronize(self):
        self.fence().synchronize()

    def _allreduce_grads(self, ws):
        if self.dp:  # data-parallel: ONE collective per step, sum over ranks on RCCL; the mean is folded into
            allreduce_sum(ws["grads"], self.pg)                         # the optimiser's grad_scale

    def _draw_and_step(self, ws, slot=None, upto_backward=False, draw=True, part=None):
        if draw and slot is None:   # (a slot holds draws made ahead)
            self._draws(ws)
        self._step(ws, slot, upto_backward, part)

    def _inject(self, dst, src, home):
        """An injected draw arrives on the caller's stream (or from the host)."""
        st = torch.cuda.current_stream(self.device)
        lease = H.acquire(src, st, home) if src.is_cuda else None
        dst.copy_(src.reshape(dst.shape), non_blocking=src.is_cuda)
        H.release(lease, st)

    # ------------------------------------------------------------------------------------------
    def _slot_key(self, B):
        """The key of the graphs over draws made ahead (no randint bound baked in); a new key empties the graph cache."""
        key = (B, 0, id(self._partner()), self._norm_key())
        if self._graph_key != key:
            self._slot_graphs, self._run_graph, self._graph, self._graph_post, self._graph_key = {}, None, None, None, key
        return key

    @torch.no_grad()
    def _learn(self, injected=None):
        """One gradient step: on `injected` draws (parity tests), on a slot of draws made ahead, as the per-step hipGraph, or eagerly."""
        if not self.ready_to_learn():
            return self.sleep_time
        B = int(self.cfg.algo.batch_size)
        home = torch.cuda.current_stream(self.device)
        with self._lock, torch.cuda.device(self.device), self._on_stream():
            ws = self._workspace(B)
            if injected is not None:
                self._learn_injected(ws, injected, home)
                self._after_step(ws, None)
            elif self._ahead is not None and self._bound() < DRAWS_AHEAD_BOUND:
                # draws + input tiles of the next K steps come from one launch pair (`_prefetch`), the step itself has no RNG
                # and no gather launch left; one hipGraph per slot (the tiles' addresses are baked in)
                self._check_ahead()
                if self._ahead.valid == 0:
                    self._prefetch(ws)
                slot = self._ahead.take()
                if self.use_graph:
                    key = self._slot_key(B)
                    if slot not in self._slot_graphs:
                        with H.CAPTURE_LOCK:
                            self._capture(ws, key, slot)
                    self._replay(ws, self._slot_graphs[slot])
                else:
                    self._step(ws, slot)
                self._after_step(ws, slot)
            elif self.use_graph:
                key = (B, self._bound() if self._graph_rng else 0, id(self._partner()), self._norm_key())
                if self._graph is None or self._graph_key != key:
                    with H.CAPTURE_LOCK:
                        self._capture(ws, key)
                if not self._graph_rng:   # draws in front of the graph (see __init__)
                    self._draws(ws)
                self._replay(ws, self._graph)
                self._after_step(ws, None)
            else:
                self._draw_and_step(ws)
                self._after_step(ws, None)
            self.update_count += 1   # under the lock: update() reads it together with the device loss ring (free-running threads)
        return self.sleep_time

    def _run_in_one_graph(self, ws, n):
        """Whether `n` steps from here are one whole run of draws-ahead steps that may replay as ONE hipGraph."""
        return (self.use_graph and self._run_graphs and self._ahead is not None and n == ws["K"] and n > 1 and self._ahead.valid in (0, n)
                and (self._ahead.valid == 0 or self._ahead.pos == 0) and self._bound() < DRAWS_AHEAD_BOUND
                and (not self.dp or graph_collective_enabled(self.pg)))

    @torch.no_grad()
    def learn_many(self, n):
        """`n` consecutive gradient steps: exactly what n `learn()` calls do -- the same draws, tiles and launches in the same
        order on this learner's queue, bit for bit.  When they are one whole run of draws-ahead steps (the critic_sample_ratio
        steps between two `update()` calls of the fixed-ratio loop, scripts/train_pql.py) they replay as ONE hipGraph instead of
        one per step: every graph boundary costs the queue ~5 us of device time (tools/probes/multistep_graph_probe.py: 603.8 ->
        599.0 us per step) and the host a launch.  Anything else (a partial run, per-step draws, eager mode, eager data-parallel
        collectives) is the loop of `learn()` calls itself."""
        n = int(n)
        if not self.ready_to_learn() or n <= 0:
            return self.sleep_time
        with self._lock, torch.cuda.device(self.device), self._on_stream():
            ws = self._workspace(int(self.cfg.algo.batch_size))
            self._check_ahead()
            if self._run_in_one_graph(ws, n):
                if self._ahead.valid == 0:
                    self._prefetch(ws)
                key = self._slot_key(ws["B"])
                if self._run_graph is None:
                    with H.CAPTURE_LOCK:
                        self._capture_run(ws, key)
                for _ in range(n):
                    self._ahead.take()
                self._run_graph.replay()
                self._after_step(ws, n - 1)
                self.update_count += n
                return self.sleep_time
            if self._ahead is not None and self._ahead.valid == 0 and n < ws["K"] and self._bound() < DRAWS_AHEAD_BOUND:
                self._prefetch(ws, steps=n)   # a partial run: fetch what its n steps will use, not K steps' worth
        for _ in range(n):
            self.learn()
        return self.sleep_time

    def _capture_run(self, ws, key):
        """All K steps of a run (slot 0 .. K-1, in order) in one hipGraph; the tiles and draws `_prefetch` left are in place."""
        def run():
            for slot in range(ws["K"]):
                self._step(ws, slot)
        snap = self._warm_up(run)
        g = self._new_graph()
        if self.dp:   # (a run graph under data parallel exists only with captured collectives)
            DP.drain_pending_collectives(self.pg)
        with torch.cuda.graph(g, stream=self._capture_stream, capture_error_mode="thread_local"):
            run()
        self._restore(snap)
        self._run_graph, self._graph_key = g, key

    def _replay(self, ws, g):
        """g: the step's hipGraph, or (data parallel, collectives kept eager) the list of its pieces: one graph up to the
        gradient + ONE all-reduce, or one graph per bucket with that bucket's all-reduce issued behind it; then the optimiser's."""
        if isinstance(g, list):
            for k, piece in enumerate(g):
                piece.replay()
                self._reducer.issue(ws["bucket_views"][k])
            self._reducer.wait()
            self._graph_post.replay()
            return
        g.replay()
        if self._graph_post is not None:   # data parallel: the collective stays outside the graphs
            self._allreduce_grads(ws)
            self._graph_post.replay()

    @torch.no_grad()
    def prepare(self):
        """Build the workspace and capture the step's hipGraph now instead of inside the first `learn()` (capture runs one
        step and restores every tensor and the RNG state it touched, so this changes nothing observable)."""
        if not self.ready_to_learn():
            return
        with self._lock, torch.cuda.device(self.device), self._on_stream():
            ws = self._workspace(int(self.cfg.algo.batch_size))
            if self.use_graph and self._ahead is not None and 0 < self._bound() < DRAWS_AHEAD_BOUND:
                key = self._slot_key(ws["B"])
                off = self.gen.get_offset()
                self._prefetch(ws)              # (the captures' warm-up runs need real tiles; nothing is consumed: the
                for slot in range(ws["K"]):     #  generator is put back and the tiles are dropped)
                    if slot not in self._slot_graphs:
                        with H.CAPTURE_LOCK:
                            self._capture(ws, key, slot)
                if self._run_graph is None and self._run_graphs and ws["K"] > 1 and (not self.dp or graph_collective_enabled(self.pg)):
                    with H.CAPTURE_LOCK:
                        self._capture_run(ws, key)
                self._drop_ahead()
                self.gen.set_offset(off)
            elif self.use_graph:
                key = (ws["B"], self._bound() if self._graph_rng else 0, id(self._partner()), self._norm_key())
                if self._graph is None or self._graph_key != key:
                    with H.CAPTURE_LOCK:
                        self._capture(ws, key)

    def _capture(self, ws, key, slot=None):
        """Capture the whole step into a hipGraph.  With `algo.graph_rng` the RNG draws are captured too; the graph then bakes
        in the randint bound and is re-captured while the ring is still filling.  slot: the step reads the draws / tiles
        `_prefetch` left in that slot (no RNG, no gather inside the graph); one graph per slot."""
        step = functools.partial(self._draw_and_step, ws, slot)
        snap = self._warm_up(step)
        g, g_post = self._new_graph(), None
        # PQL_DP_GRAPH_COLLECTIVE=1 (opt-in, RCCL only, rehearsed with a 1-rank group only): capture the all-reduce inside
        # ONE graph instead of splitting the step around an eager collective
        if not self.dp or graph_collective_enabled(self.pg):
            if self.dp:
                DP.drain_pending_collectives(self.pg)   # (the warm-up's eager all-reduce must have left the watchdog's list)
            with torch.cuda.graph(g, stream=self._capture_stream, capture_error_mode="thread_local"):
                step(draw=self._graph_rng)
        else:   # two graphs around the RCCL all-reduce (kept eager: no collective is ever captured)
            if self._buckets is not None:   # ... or one per gradient bucket, each followed by its own collective
                g = [g] + [self._new_graph() for _ in self._buckets[1:]]
                for k, piece in enumerate(g):
                    with torch.cuda.graph(piece, stream=self._capture_stream, capture_error_mode="thread_local"):
                        step(part=k, draw=self._graph_rng and k == 0)
            else:
                with torch.cuda.graph(g, stream=self._capture_stream, capture_error_mode="thread_local"):
                    step(upto_backward=True, draw=self._graph_rng)
            if slot is None or self._graph_post is None:   # (the optimiser graph is the same for every slot)
                g_post = self._new_graph()
                with torch.cuda.graph(g_post, stream=self._capture_stream, capture_error_mode="thread_local"):
                    self._step_post(ws)
            else:
                g_post = self._graph_post
        self._restore(snap, tensors=self.RESTORE_AFTER_CAPTURE)  # capture does not execute, but keep state exactly as before
        if slot is None:
            self._graph, self._graph_post, self._graph_key = g, g_post, key
        else:
            self._slot_graphs[slot] = g
            self._graph_post, self._graph_key = g_post, key

    def _warm_up(self, step):
        """`step` once outside capture (lazy hipFuncSetAttribute / allocator state), on a side stream as torch requires, and undone."""
        snap = self._snapshot()
        s = torch.cuda.Stream(self.device)
        s.wait_stream(torch.cuda.current_stream(self.device))
        with torch.cuda.stream(s):
            step()
        torch.cuda.current_stream(self.device).wait_stream(s)
        self._restore(snap)
        return snap

    def _new_graph(self):
        g = torch.cuda.CUDAGraph()
        if self._graph_rng:    # a private generator takes part in capture only when registered with the graph
            g.register_generator_state(self.gen)
        return g

    def _snapshot(self):
        return [t.clone() for t in self._captured()], self.gen.get_state()

    def _restore(self, snap, tensors=True):
        saved, rng = snap
        if tensors:
            for dst, src in zip(self._captured(), saved):
                dst.copy_(src)
            self.repack()
        self.gen.set_state(rng)

    # ------------------------------------------------------------------------------------------
    def training_state(self):
        """Everything later steps depend on, as CPU tensors and plain values; the caller has synchronised the
        device.  `_own_state`: the subclass's arenas and its ring's header (the ring's rows are streamed separately)."""
        with self._lock:
            return dict(self._own_state(), opt=adam_state(self.opt), update_count=int(self.update_count), loss_ring=_cpu(self.loss_ring),
                        lagged=lagged_state(self._lagged), loss_tracker=[float(x) for x in self.loss_tracker.moving_average],
                        norm=norm_state(self), sleep_time=float(self.sleep_time), gen=self.gen.get_state().clone(),
                        published=self._pub.training_state())

    @torch.no_grad()
    def load_training_state(self, st, memory=True):
        """In place: arenas, rings, packed copies, publisher buffers and captured hipGraphs keep their addresses.  memory=False
        leaves the (empty) ring and its pointers alone -- a checkpoint written without rings.  The ring ROWS are read by the
        caller right after this call; what was prepared ahead is dropped here, and the ring's version moves on."""
        with self._lock, torch.cuda.device(self.device):
            self._load_own_state(st, memory)
            load_adam_state(self.opt, st["opt"])
            self.update_count = int(st["update_count"])
            self.loss_ring.copy_(st["loss_ring"])
            load_lagged_state(self._lagged, st["lagged"])
            self.loss_tracker = Tracker(LOSS_RING)
            self.loss_tracker.update(list(st["loss_tracker"]))
            load_norm_state(self, st["norm"])
            self.sleep_time = st["sleep_time"]
            self.gen.set_state(st["gen"].cpu())
            self._pub.load_training_state(st["published"])
            self.repack()
            self._drop_ahead()
            self._ahead_stamp = None

    def _load_partner(self, saved, make):
        """The partner's replica out of a checkpoint (None: the learner had not been handed one yet)."""
        if saved is None:
            return
        if self._partner() is None:
            module = make(self.cfg, self.obs_dim, self.action_dim, self.device)
            module.requires_grad_(False)
            setattr(self, self.PARTNER, module)
            setattr(self, "pk_" + self.PARTNER, PackedWeights(module.layout, self.device) if self._fused else None)
        self._partner().arena.data.copy_(saved)

    def loss_mean(self):
        """Exact mean of the last 5 losses (Tracker(5).mean(), zero-filled before 5 steps); synchronises."""
        with torch.cuda.device(self.device), self._on_stream():
            vals = self.loss_ring.tolist()
        m = LaggedLoss.mean_of(vals, self.update_count)
        self.loss_tracker = Tracker(LOSS_RING)
        for t in range(self.update_count - min(self.update_count, LOSS_RING), self.update_count):
            self.loss_tracker.update(vals[t % LOSS_RING])
        return m

    def _adopt_partner(self, module, home=None):
        """Adopt new weights into the resident replica of the partner: a fenced flat-arena copy on this learner's stream; from
        another GPU through the copy streams (peer copy over xGMI) -- the reference pickles the module through Ray.  On first
        sight, or when the layout changed, the replica is a deepcopy (`_new_partner`: what the subclass has to mend in one)."""
        cur, pk = self._partner(), "pk_" + self.PARTNER
        if cur is None or cur.layout.dims != module.layout.dims:
            st = torch.cuda.current_stream(self.device)
            with H.LOCK:
                lease = H.acquire(module, st, home)
                cur = deepcopy(module).to(self.device)
                H.release(lease, st)
            cur.requires_grad_(False)
            self._new_partner(cur)
            setattr(self, self.PARTNER, cur)
            setattr(self, pk, PackedWeights(cur.layout, self.device) if self._fused else None)
        elif module is not cur:
            adopt_arena(cur, module, self.device, home)
        if getattr(self, pk) is not None:
            getattr(self, pk).refresh(cur.arena.data)

    def _new_partner(self, module):
        pass
