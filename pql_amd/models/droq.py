"""`DoubleQDropoutLayerNorm`: the DroQ critic (Hiraoka et al. 2022) -- `DoubleQLayerNorm` with dropout in front of every LayerNorm:
twin `Linear -> Dropout(p) -> LayerNorm -> ELU -> ... -> Linear` Q heads, in the critic and in its target, the dropout ON in every
learning forward.  It is what lets SAC run a high update-to-data ratio (`algo.update_times`; algo=droq_algo).

Dropout has no parameters: arena, views, state_dict keys and initialisation are `DoubleQLayerNorm`'s, and a checkpoint of either
class loads into the other.  The norm step is `pqlk_drop_ln_elu_forward / _backward` (pql_amd/csrc/ln.hip): the keep mask is
generated inside the LayerNorm + ELU row launches from Philox4x32-10, forward and backward -- no mask tensor exists.  The mask law
(include/pqlk.h) is a pure function of (seed, tag, row, column); this class supplies

    seed = `seed`, or torch.initial_seed() when None (reading it consumes nothing from any generator)
    tag  = (drop_calls << 8) | (drop_stream << 5) | (net << 4) | layer

`drop_calls` counts the `forward_raw(..., drop=True)` calls of this module on the host; `drop_stream` tells a module from its copies:
a `deepcopy` (the target critic) gets `drop_stream + 1`, so a critic and its target never share a mask.  `backward_raw` regenerates
the masks of the forward it belongs to from the counter value that forward stashed.  (seed, drop_calls, drop_stream) is the whole
state of the dropout: `drop_state()` / `load_drop_state()`, saved with an agent's training state.
"""
from __future__ import annotations

import math

import torch

from pql_amd import _lib as L
from pql_amd.models.layernorm import LN_EPS, DoubleQLayerNorm

MAX_DROP_LAYERS, MAX_DROP_STREAM = 16, 7   # the tag's 4 layer bits and 3 stream bits


def check_dropout(p):
    """`algo.critic_dropout` / the constructor's `dropout`: a probability in [0, 1)."""
    ok = isinstance(p, (int, float)) and not isinstance(p, bool) and math.isfinite(p) and 0.0 <= p < 1.0
    if not ok:
        raise ValueError(f"algo.critic_dropout must be a number in [0, 1) (the probability that a hidden unit of the critic is dropped; "
                         f"0 keeps every unit), got {p!r}")
    return float(p)


class DoubleQDropoutLayerNorm(DoubleQLayerNorm):
    def __init__(self, state_dim, act_dim, hidden_layers=None, dropout=0.01, seed=None):
        p = check_dropout(dropout)   # before anything is allocated
        super().__init__(state_dim, act_dim, hidden_layers)
        self.dropout = p
        if self.n_layers - 1 > MAX_DROP_LAYERS:
            raise ValueError(f"DoubleQDropoutLayerNorm: {self.n_layers - 1} hidden layers, the mask tag has room for {MAX_DROP_LAYERS}")
        self.seed = int(torch.initial_seed() if seed is None else seed) & (2 ** 64 - 1)
        self.drop_calls, self.drop_stream = 0, 0

    def __deepcopy__(self, memo):
        new = super().__deepcopy__(memo)
        if new.drop_stream + 1 > MAX_DROP_STREAM:
            raise ValueError(f"DoubleQDropoutLayerNorm: a copy of stream {self.drop_stream} would be stream {new.drop_stream + 1}, the mask "
                             f"tag has room for streams 0 to {MAX_DROP_STREAM}")
        new.drop_stream += 1
        return new

    # ---- the dropout's state ---------------------------------------------------------------------------------
    def drop_state(self):
        return {"seed": int(self.seed), "drop_calls": int(self.drop_calls), "drop_stream": int(self.drop_stream)}

    def load_drop_state(self, st):
        self.seed, self.drop_calls, self.drop_stream = int(st["seed"]), int(st["drop_calls"]), int(st["drop_stream"])

    def tag(self, call, n, l):
        """The mask tag of hidden layer `l` of net `n` in the `call`-th dropout forward of this module."""
        return ((int(call) << 8) | (self.drop_stream << 5) | (n << 4) | l) & (2 ** 64 - 1)

    # ---- the norm step ---------------------------------------------------------------------------------------
    def _norm_forward(self, ws, n, l, z, y, M, st, call=None):
        if call is None:
            return super()._norm_forward(ws, n, l, z, y, M, st)
        L.check(L.lib.pqlk_drop_ln_elu_forward(L.ptr(z), z.stride(0), M, self.dims[l + 1], L.ptr(self.norm_param(n, l, "gamma")),
                                               L.ptr(self.norm_param(n, l, "beta")), LN_EPS, self.dropout, self.seed, self.tag(call, n, l),
                                               L.ptr(y), L.ptr(ws["mean"][(n, l)]), L.ptr(ws["rstd"][(n, l)]), st))

    def _norm_backward(self, ws, n, l, d, M, gg, gb, st):
        call = ws.get("drop_call")   # of the forward this backward belongs to (None: it ran without dropout)
        if call is None:
            return super()._norm_backward(ws, n, l, d, M, gg, gb, st)
        z = ws["z"][(n, l)]
        L.check(L.lib.pqlk_drop_ln_elu_backward(L.ptr(d), L.ptr(ws["y"][(n, l)]), L.ptr(z), z.stride(0), M, self.dims[l + 1],
                                                L.ptr(ws["mean"][(n, l)]), L.ptr(ws["rstd"][(n, l)]), L.ptr(self.norm_param(n, l, "gamma")),
                                                self.dropout, self.seed, self.tag(call, n, l), L.ptr(d), L.ptr(gg), L.ptr(gb),
                                                L.ptr(ws["ln_scratch"]) if gg is not None else None, st))

    @torch.no_grad()
    def forward_raw(self, x_pad, drop=True):
        """x_pad (M, ld(in)) with zero pad columns -> Q (2, M, 32) (column 0).  drop=True (every learning forward): the hidden blocks
        run with this call's masks and `drop_calls` advances; `backward_raw` on the same x_pad regenerates them.  drop=False: the plain
        LayerNorm entries, forward and backward -- `DoubleQLayerNorm`'s bits."""
        call = self.drop_calls if drop else None
        ws = self._forward_layers(x_pad, call=call)
        ws["drop_call"] = call
        if drop:
            self.drop_calls += 1
        return self._q_of(ws)

    # ---- reference surface (evaluation, logging): no dropout ---------------------------------------------------
    def _heads(self, state, action):
        return self.forward_raw(self._x_of(state, action), drop=False)
