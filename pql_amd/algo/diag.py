"""Opt-in critic diagnostics (`algo.diag`): THE place where their configuration rules, their log keys and their probe's launches
are stated.  The PQL V-learner (at hand-off time, `update()`) and the DDPG agent (at the end of `update_net`) hold one `CriticProbe`
and hand it the outputs and the post-ELU matrices of one no-gradient forward of the critic and of its target; the probe runs
`pqlk_critic_stats` and `pqlk_unit_stats` (include/pqlk.h) on them, eagerly and outside every graph, into a device block of its own,
and brings the block to the host the way the loss gets there: an async copy to pinned memory, read once its event has passed, no
synchronise.  Nothing here is part of a checkpoint, and nothing a training step reads is written.

What the values describe: the weights as they stand when the probe runs (the ones being handed out), on the LAST batch they were
trained on -- so the TD residual is that batch's AFTER its step -- with the scalar-law target y = r + (1 - d) gamma^n min(V'_1, V'_2)
whatever loss trains the head.  Under data parallel they are the logging rank's own shard: there is no collective.
Every entry is looked up as `L.lib.<name>` when it is called: tests spy on those attributes.
"""
from __future__ import annotations

import torch

from pql_amd import _lib as L

STAT_KEYS = ("q1_mean", "q2_mean", "q_min", "q_max", "target_mean", "td_bias", "td_abs_mean", "td_abs_max", "twin_gap", "nonfinite")
UNIT_KEYS = ("dormant", "act_abs", "elu_slope")   # out[0 .. 3) of pqlk_unit_stats; logged per hidden layer as diag/<key>_l<layer>
assert len(STAT_KEYS) == L.CRITIC_STATS
HEAD_KINDS = {"scalar": L.HEAD_SCALAR, "categorical": L.HEAD_CATEGORICAL, "quantile": L.HEAD_QUANTILE}
# algo.name -> why algo.diag.enabled=True is refused (droq_algo is AgentSAC: name "SAC")
OUT_OF_SCOPE = {
    "SAC": "the diagnostics' target is the scalar law r + (1 - d) gamma^n min Q', which omits SAC's entropy term and would mislead",
    "TQC": "the diagnostics' target is the scalar law r + (1 - d) gamma^n min Q', which omits TQC's entropy term and would mislead",
    "CrossQ": "CrossQ has no target critic to form the diagnostics' TD target from",
    "PPO": "PPO has no twin Q critic",
}


def _whole(v):
    return isinstance(v, (int, float)) and not isinstance(v, bool) and int(v) == v


def diag_cfg(cfg):
    """`algo.diag` checked, before anything is allocated -> None (off, or a config without the node) or (every, tau).  every: an
    integer >= 1 (PQL: hand-offs, DDPG: `update_net` calls between two probes); tau: the dormant threshold, in [0, 1)."""
    algo = cfg.algo
    node = algo.get("diag")
    if node is None:
        return None
    every, tau, enabled = node.get("every", 10), node.get("tau", 0.025), node.get("enabled", False)
    if not isinstance(enabled, bool):
        raise ValueError(f"algo.diag.enabled must be True or False, got {enabled!r}")
    if not _whole(every) or int(every) < 1:
        raise ValueError(f"algo.diag.every must be an integer >= 1 (hand-offs in PQL, update_net calls in DDPG between two probes), got {every!r}")
    if isinstance(tau, bool) or not isinstance(tau, (int, float)) or not 0.0 <= float(tau) < 1.0:
        raise ValueError(f"algo.diag.tau must be a number in [0, 1) (a unit is dormant when its mean |activation| is at most tau times "
                         f"its layer's), got {tau!r}")
    if not enabled:
        return None
    name = str(algo.get("name") or "")
    if name in OUT_OF_SCOPE:
        raise ValueError(f"algo.diag.enabled=True cannot run with algo.name={name}: {OUT_OF_SCOPE[name]}; the diagnostics are built for "
                         f"algo=pql_algo (the V-learner) and algo=ddpg_algo")
    return int(every), float(tau)


def log_keys(n_hidden):
    return ["diag/" + k for k in STAT_KEYS] + [f"diag/{k}_l{l}" for l in range(1, n_hidden + 1) for k in UNIT_KEYS]


class CriticProbe:
    """The device block, its pinned mirror and the launches.  `layers`: hidden layers with a post-ELU matrix, per net the same.
    block = [PQLK_CRITIC_STATS | (net, layer): 3 floats each, the critic's twin nets in order]."""

    def __init__(self, head, every, tau, layers, device):
        self.head, self.every, self.tau, self.layers, self.device = head, int(every), float(tau), int(layers), device
        self.calls = 0      # hand-offs (PQL) / update_net calls (DDPG) seen so far; not saved: a resumed run counts from 0
        n = L.CRITIC_STATS + 2 * 3 * self.layers
        self.block = torch.zeros(n, dtype=torch.float32, device=device)
        self.host = torch.zeros(n, dtype=torch.float32).pin_memory()
        self.scratch = torch.zeros(1, dtype=torch.float32, device=device)
        self.event = None
        self.values = {}

    def due(self):
        """Counts one hand-off / update_net call; True on every `every`-th."""
        self.calls += 1
        return self.calls % self.every == 0

    def _scratch(self, floats):
        if self.scratch.numel() < floats:
            self.scratch = torch.zeros(int(floats), dtype=torch.float32, device=self.device)
        return self.scratch

    def critic_stats(self, q, qt, ld, rew, done, gamma_n, B):
        """q, qt (2, B, ld): the outputs of the critic and of its target -> block[0 : PQLK_CRITIC_STATS)."""
        h, algo = self.head, self.head.algo
        cat = h.kind == "categorical"
        scratch = self._scratch(L.lib.pqlk_critic_stats_scratch_floats(B, h.width))
        L.check(L.lib.pqlk_critic_stats(L.ptr(q), L.ptr(qt), int(ld), HEAD_KINDS[h.kind], h.width, L.ptr(h.critic.z_atoms) if cat else None,
                                        float(algo.v_min) if cat else 0.0, float(algo.v_max) if cat else 0.0, L.ptr(rew), L.ptr(done),
                                        float(gamma_n), int(B), L.ptr(self.block), L.ptr(scratch), L.stream(self.device)))

    def unit_stats(self, which, layer, h, ld, rows, cols):
        """h: a (rows, ld) post-ELU matrix (a tensor whose first element is h[0, 0]) of hidden layer `layer` (0-based) of net
        `which` (0, 1) of the critic -> its three floats of the block."""
        scratch = self._scratch(L.lib.pqlk_unit_stats_scratch_floats(int(cols)))
        o = L.CRITIC_STATS + 3 * (which * self.layers + layer)
        L.check(L.lib.pqlk_unit_stats(L.ptr(h), int(ld), int(rows), int(cols), self.tau, L.ptr(self.block[o: o + 3]), L.ptr(scratch),
                                      L.stream(self.device)))

    def ship(self):
        """The block -> pinned memory, asynchronously on the current stream; `diagnostics` reads it once the copy has landed."""
        self.host.copy_(self.block, non_blocking=True)
        self.event = torch.cuda.Event()
        self.event.record()

    def decode(self, vals):
        """The block's floats -> the log dict; a layer's value is the mean over the critic's two nets."""
        out = {"diag/" + k: float(v) for k, v in zip(STAT_KEYS, vals)}
        n0 = L.CRITIC_STATS
        for l in range(self.layers):
            for j, k in enumerate(UNIT_KEYS):
                a, b = (vals[n0 + 3 * (w * self.layers + l) + j] for w in (0, 1))
                out[f"diag/{k}_l{l + 1}"] = (float(a) + float(b)) / 2.0
        return out

    def diagnostics(self):
        """The values of the last probe whose copy has landed ({} before the first); never waits."""
        if self.event is not None and self.event.query():
            self.values = self.decode(self.host.tolist())
            self.event = None
        return dict(self.values)
