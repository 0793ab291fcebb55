"""`DoubleQBroNet`: a residual LayerNorm twin critic (BroNet: BRO, Nauman et al. 2024; SimBa is its pre-norm cousin) for DDPG and SAC.
Twin Q heads on `cat(state, action)`, per net, with width W = `width` (`algo.critic_width`) and K = `blocks` (`algo.critic_blocks`):

    z0 = x W0' + b0          h0 = ELU(LN(z0))                          pqlk_ln_elu_forward
    for k = 1..K:
      za = h_{k-1} Wa' + ba  t   = ELU(LN(za))                         pqlk_ln_elu_forward
      zb = t Wb' + bb        h_k = h_{k-1} + LN(zb)                    pqlk_ln_res_forward
    q  = h_K Wo' + bo

The skip connection around each block is what lets depth grow without the TD loss diverging.  The activation is ELU, like every
critic here; BRO itself uses ReLU.  LayerNorm is `nn.LayerNorm(W, eps=1e-5)`.

A chain of 2 K + 2 Linears with a norm behind all but the last is `DoubleQLayerNorm(hidden_layers=[W] * (2 K + 1))`'s arena, views,
workspace and per-layer GEMM loops (pql_amd/models/normq.py), and they are used as they are; layer 0 is the stem, layers 2 k - 1 /
2 k are block k's first / second Linear, layer 2 K + 1 the output.  Only the norm step differs, by layer:

    forward   stem, first half of a block: LayerNorm + ELU; second half: pqlk_ln_res_forward with res = h_{k-1}, the output of
              two layers before
    backward  second half of block k: pqlk_ln_sum_backward(dy = A_k, dy2 = S_k, y = NULL) -> dsum = G_k = A_k + S_k, dz in place
              (A_k: the gradient that came down through the Linears, S_k: the running skip gradient; S_K does not exist: dy2 NULL);
              first half: pqlk_ln_elu_backward; then S_{k-1} = G_k, updated in place in ONE (M, ld(W)) buffer of the workspace;
              stem: pqlk_ln_sum_backward(dy = A_0, dy2 = S_0, y = h0).

No stand-alone add launch runs, forward or backward.  With K = 0 nothing of this is reached: the class then IS
`DoubleQLayerNorm(hidden_layers=[W])` -- the same launches, the same bits for the same parameters.

Initialisation: Linears get the `nn.Linear` default, gamma = 1, beta = 0; the draws come from the CPU generator in the order
net 1 then net 2, in each the layers in forward order, in each W then b (`NormTwinQ.reset_parameters`).

state_dict keys are those of the torch twin (tests/bronet_cases.py `Twin`): per net `net_q{1,2}.`
    stem.0.{weight,bias}                 Linear(in, W)         stem.1.{weight,bias}        LayerNorm(W)       (stem.2: ELU)
    blocks.{k}.0 / blocks.{k}.1          Linear(W, W), LayerNorm(W)                        k = 0 .. K - 1     (blocks.{k}.2: ELU)
    blocks.{k}.3 / blocks.{k}.4          Linear(W, W), LayerNorm(W)
    out.{weight,bias}                    Linear(W, 1)
There are no buffers.
"""
from __future__ import annotations

import torch

from pql_amd import _lib as L
from pql_amd.models.layernorm import LN_EPS, DoubleQLayerNorm

MAX_BLOCKS = 16


def _whole(v):
    return isinstance(v, (int, float)) and not isinstance(v, bool) and int(v) == v


def check_width(width):
    """`algo.critic_width`: an integer >= 1; -> the int."""
    if not _whole(width) or int(width) < 1:
        raise ValueError(f"algo.critic_width must be an integer >= 1 (the width of every hidden layer of DoubleQBroNet), got {width!r}")
    return int(width)


def check_blocks(blocks):
    """`algo.critic_blocks`: an integer from 0 to 16; -> the int."""
    if not _whole(blocks) or not 0 <= int(blocks) <= MAX_BLOCKS:
        raise ValueError(f"algo.critic_blocks must be an integer from 0 to {MAX_BLOCKS} (the residual blocks of DoubleQBroNet; 0 is "
                         f"DoubleQLayerNorm with one hidden layer), got {blocks!r}")
    return int(blocks)


class DoubleQBroNet(DoubleQLayerNorm):
    key_prefixes = ("net_q1.", "net_q2.")

    def __init__(self, state_dim, act_dim, width=512, blocks=2):
        self.width, self.blocks = check_width(width), check_blocks(blocks)   # before anything is allocated
        super().__init__(state_dim, act_dim, hidden_layers=[self.width] * (2 * self.blocks + 1))
        self.init_kwargs = dict(state_dim=self.state_dim, act_dim=self.act_dim, width=self.width, blocks=self.blocks)

    def layer_key(self, l):
        """(key of Linear `l`, key of the norm behind it) under a net's prefix."""
        if l == 0:
            return "stem.0", "stem.1"
        if l == self.n_layers - 1:
            return "out", None
        k, second = (l - 1) // 2, (l - 1) % 2
        return f"blocks.{k}.{3 * second}", f"blocks.{k}.{3 * second + 1}"

    def named_views(self, arena=None):
        for n, pre in enumerate(self.key_prefixes):
            for l in range(self.n_layers):
                lin, norm = self.layer_key(l)
                yield f"{pre}{lin}.weight", self.weight(n, l, arena)
                yield f"{pre}{lin}.bias", self.bias(n, l, arena)
                if norm is not None:
                    yield f"{pre}{norm}.weight", self.norm_param(n, l, "gamma", arena)
                    yield f"{pre}{norm}.bias", self.norm_param(n, l, "beta", arena)

    def elu_layers(self):
        """The stem and the first half of every block: a block's second half adds the skip to a bare LayerNorm, no ELU."""
        return [l for l in range(self.n_layers - 1) if not self._closes_block(l)]

    # ---- the norm step, by layer -------------------------------------------------------------------------------
    def _closes_block(self, l):
        """Whether hidden layer `l` is the second half of a block: its norm has no ELU and carries the skip."""
        return l > 0 and l % 2 == 0

    def _norm_workspace(self, ws, key, M, w, f):
        super()._norm_workspace(ws, key, M, w, f)
        if self.blocks and "skip" not in ws:
            ws["skip"] = torch.zeros((M, w), **f)    # the running skip gradient S_k; pad columns stay zero

    def _norm_forward(self, ws, n, l, z, y, M, st):
        if not self._closes_block(l):
            return super()._norm_forward(ws, n, l, z, y, M, st)
        L.check(L.lib.pqlk_ln_res_forward(L.ptr(z), z.stride(0), M, self.width, L.ptr(self.norm_param(n, l, "gamma")),
                                          L.ptr(self.norm_param(n, l, "beta")), LN_EPS, L.ptr(ws["y"][(n, l - 2)]), L.ptr(y),
                                          L.ptr(ws["mean"][(n, l)]), L.ptr(ws["rstd"][(n, l)]), st))

    def _norm_backward(self, ws, n, l, d, M, gg, gb, st):
        stem = l == 0 and self.blocks > 0
        if not stem and not self._closes_block(l):
            return super()._norm_backward(ws, n, l, d, M, gg, gb, st)
        z, skip = ws["z"][(n, l)], ws["skip"]
        assert d.stride(0) == skip.stride(0) == z.stride(0)
        last = l == 2 * self.blocks                                     # block K: no skip gradient yet
        L.check(L.lib.pqlk_ln_sum_backward(L.ptr(d), None if last else L.ptr(skip), L.ptr(ws["y"][(n, 0)]) if stem else None, L.ptr(z),
                                           z.stride(0), M, self.width, L.ptr(ws["mean"][(n, l)]), L.ptr(ws["rstd"][(n, l)]),
                                           L.ptr(self.norm_param(n, l, "gamma")), None if stem else L.ptr(skip), L.ptr(d), L.ptr(gg),
                                           L.ptr(gb), L.ptr(ws["ln_scratch"]) if gg is not None else None, st))
