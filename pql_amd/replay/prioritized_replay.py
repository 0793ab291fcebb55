"""Prioritized experience replay (Schaul et al. 2016, proportional variant) on the replay ring: `ReplayBuffer` plus a radix-64 sum
tree over its rows that lives on the device (pql_amd/csrc/per.hip; layout and formulas in include/pqlk.h).

The reference has no prioritized replay.  `PrioritizedReplayBuffer` is the plain buffer for everything the plain buffer does
(records, pointers, views, `sample_batch`); on top of it
    add_to_buffer       gives the new rows the largest priority seen so far (`pqlk_per_insert`, the ring insert's segments),
    draw_indices(B)     draws B rows with probability leaf / total, stratified, and keeps their importance weights,
    weights_for(idx)    the importance weights of given rows (parity tests inject their indices),
    draw_steps          the rows and weights of several steps' batches in one launch, all on the tree as it stands (`algo.per.refresh=run`),
    update_priorities   writes |TD| + eps back and repairs the tree.
Nothing here synchronises with the host.  The agent sets `beta` (ActorCriticBase's schedule) before it samples.
"""
from __future__ import annotations

import torch

from pql_amd import _lib as L
from pql_amd.replay.simple_replay import ReplayBuffer, ring_plan


def per_cfg(algo):
    """The `algo.per` block when prioritized replay is switched on, else None (no block, or enabled: False)."""
    per = algo.get("per") if hasattr(algo, "get") else getattr(algo, "per", None)
    if per is None or not bool(per.get("enabled") or False):
        return None
    return per


def per_refresh(per):
    """`algo.per.refresh`: "step" (sample from the live tree and write back every learner step; a block without the key) or "run"
    (one sample launch and one write-back per run of prefetched steps: the PQL V-learner)."""
    value = str(per.get("refresh") or "step")
    if value not in ("step", "run"):
        raise ValueError(f"algo.per.refresh must be step or run, got {value!r}")
    return value


def per_beta(beta0, beta_iters, calls):
    """The importance-sampling exponent of prioritized replay after `calls` calls of `update_net` (PQL V-learner: steps): linear from beta0 to 1 over
    `beta_iters` calls, exactly 1.0 from there on."""
    if calls >= beta_iters:
        return 1.0
    return float(beta0) + (1.0 - float(beta0)) * (calls / float(beta_iters))


class PrioritizedReplayBuffer(ReplayBuffer):
    prioritized = True

    def __init__(self, capacity: int, obs_dim, action_dim: int, device="cuda", alpha: float = 0.6, eps: float = 1.0e-6, **kw):
        super().__init__(capacity, obs_dim, action_dim, device=device, **kw)
        self.alpha, self.eps = float(alpha), float(eps)
        if self.alpha < 0 or self.eps < 0:
            raise ValueError(f"prioritized replay needs alpha >= 0 and eps >= 0, got alpha={alpha}, eps={eps}")
        self.beta = 1.0
        self.levels = int(L.lib.pqlk_per_levels(self.capacity))
        # zeroed once: the pads of every level are never written, and a row never inserted holds priority 0
        self.tree = torch.zeros(int(L.lib.pqlk_per_tree_floats(self.capacity)), dtype=torch.float32, device=self.device)
        self.pmax = torch.ones(1, dtype=torch.float32, device=self.device)
        self.idx = self.w = None   # the last draw: rows (B) int64, weights (B)
        self.wmax = torch.zeros(1, dtype=torch.float32, device=self.device)

    @property
    def leaves(self):
        return self.tree[: self.capacity]

    # ---- state ------------------------------------------------------------------------------------
    def training_state(self):
        st = super().training_state()
        st["per"] = {"alpha": self.alpha, "eps": self.eps, "pmax": self.pmax.detach().cpu(),
                     "leaves": self.tree[: self.cur_capacity].detach().cpu()}
        return st

    def load_training_state(self, st):
        per = st.get("per")
        if per is None:
            raise ValueError("prioritized replay: the checkpoint was written by a plain replay buffer (no priorities)")
        if float(per["alpha"]) != self.alpha:
            raise ValueError(f"prioritized replay: alpha={self.alpha} but the checkpoint holds alpha={float(per['alpha'])}")
        super().load_training_state(st)
        if per["leaves"].numel() != self.cur_capacity:
            raise ValueError(f"prioritized replay: {per['leaves'].numel()} saved priorities for {self.cur_capacity} rows")
        with torch.cuda.device(self.device):
            self.tree.zero_()
            self.tree[: self.cur_capacity].copy_(per["leaves"])
            self.pmax.copy_(per["pmax"])
            L.check(L.lib.pqlk_per_rebuild(L.ptr(self.tree), self.capacity, L.stream(self.device)))

    # ---- insert -----------------------------------------------------------------------------------
    @torch.no_grad()
    def add_to_buffer(self, trajectory):
        m = trajectory[2].numel()   # rewards: one per row
        segs, _, _, _ = ring_plan(self.next_p, self.if_full, self.capacity, m)   # the segments the ring insert is about to write
        super().add_to_buffer(trajectory)
        with torch.cuda.device(self.device):
            st = L.stream(self.device)
            for dst, _, n in segs:
                if n > 0:
                    L.check(L.lib.pqlk_per_insert(L.ptr(self.tree), self.capacity, L.ptr(self.pmax), dst, n, self.alpha, st))

    # ---- sample -----------------------------------------------------------------------------------
    def draw_indices(self, batch_size, device=None):
        """The one RNG draw of a prioritized sample: `u = torch.rand(B)` on the buffer's device, one stratum each
        (t_k = (k + u_k) total / B).  Keeps `idx`, `w` (before the division by `wmax`) and `wmax` for the step."""
        B = int(batch_size)
        u = torch.rand(B, device=self.device)
        idx = torch.empty(B, dtype=torch.int64, device=self.device)
        with torch.cuda.device(self.device):
            L.check(L.lib.pqlk_per_sample(L.ptr(self.tree), self.capacity, L.ptr(u), B, L.ptr(idx), L.stream(self.device)))
        self.weights_for(idx)
        return idx if device is None else idx.to(device)

    def weights_for(self, indices):
        """(w, wmax) of the given rows at the current `beta`; kept, like a draw's, for `update_priorities`."""
        idx = indices.to(device=self.device, dtype=torch.int64).contiguous()
        B = idx.shape[0]
        if self.w is None or self.w.shape[0] != B:
            self.w = torch.empty(B, dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            L.check(L.lib.pqlk_per_weights(L.ptr(self.tree), self.capacity, L.ptr(idx), B, int(self.cur_capacity), float(self.beta),
                                           L.ptr(self.w), L.ptr(self.wmax), L.stream(self.device)))
        self.idx = idx
        return self.w, self.wmax

    def draw_steps(self, r, b, steps, beta, idx_out, w_out, wmax_out):
        """`steps` batches of `b` rows from the tree as it stands, with their weights at `beta`, in one launch (`pqlk_per_sample_steps`).
        r: steps * b int64 draws of torch.randint(1 << 24); idx_out / w_out: steps * b entries, wmax_out: one float per step.  The
        caller keeps the outputs (nothing is remembered here) and hands idx_out with the steps' |TD| to `update_priorities`."""
        with torch.cuda.device(self.device):
            L.check(L.lib.pqlk_per_sample_steps(L.ptr(self.tree), self.capacity, L.ptr(r), int(b), int(steps), int(self.cur_capacity),
                                                float(beta), L.ptr(idx_out), L.ptr(w_out), L.ptr(wmax_out), L.stream(self.device)))

    def update_priorities(self, idx, abs_td):
        """priority[idx] = |TD| + eps (a row drawn twice keeps the larger one); raises `pmax`; repairs the touched ancestors."""
        with torch.cuda.device(self.device):
            L.check(L.lib.pqlk_per_update(L.ptr(self.tree), self.capacity, L.ptr(self.pmax), L.ptr(idx), L.ptr(abs_td), idx.numel(),
                                          self.eps, self.alpha, L.stream(self.device)))
