"""`DoubleQLayerNorm`: a LayerNorm twin critic for DDPG and SAC: twin `Linear -> LayerNorm(eps=1e-5, affine) -> ELU -> ... -> Linear`
Q heads on `cat(state, action)` (the reference only hints at it: a commented-out critic at pql/models/mlp.py:288-310).

LayerNorm is row-local, so -- unlike the BatchNorm critic of CrossQ -- it works with target critics and at any batch size and
behaves the same in training and evaluation.  The arena, the views, the state_dict plumbing, the workspace and the per-layer GEMM
loops are `NormTwinQ`'s (pql_amd/models/normq.py); the norm step is `pqlk_ln_elu_forward / _backward` (pql_amd/csrc/ln.hip, the law
in include/pqlk.h).  state_dict keys are those of the equivalent `nn.Sequential`: `net_q{1,2}.net.{0,3,6,9}.{weight,bias}` for the
Linears, `net_q{1,2}.net.{1,4,7}.{weight,bias}` for the norms; there are no buffers.
"""
from __future__ import annotations

import torch

from pql_amd import _lib as L
from pql_amd.models.normq import NormTwinQ

LN_EPS = 1e-5   # nn.LayerNorm default


class DoubleQLayerNorm(NormTwinQ):
    def _norm_workspace(self, ws, key, M, w, f):
        ws.setdefault("mean", {})[key] = torch.zeros(M, **f)
        ws.setdefault("rstd", {})[key] = torch.zeros(M, **f)

    def _norm_scratch(self, ws, wmax, f):
        ws["ln_scratch"] = torch.zeros(int(L.lib.pqlk_ln_scratch_floats(wmax)), **f)

    def _norm_forward(self, ws, n, l, z, y, M, st):
        L.check(L.lib.pqlk_ln_elu_forward(L.ptr(z), z.stride(0), M, self.dims[l + 1], L.ptr(self.norm_param(n, l, "gamma")),
                                          L.ptr(self.norm_param(n, l, "beta")), LN_EPS, L.ptr(y), L.ptr(ws["mean"][(n, l)]),
                                          L.ptr(ws["rstd"][(n, l)]), st))

    def _norm_backward(self, ws, n, l, d, M, gg, gb, st):
        z = ws["z"][(n, l)]
        L.check(L.lib.pqlk_ln_elu_backward(L.ptr(d), L.ptr(ws["y"][(n, l)]), L.ptr(z), z.stride(0), M, self.dims[l + 1],
                                           L.ptr(ws["mean"][(n, l)]), L.ptr(ws["rstd"][(n, l)]), L.ptr(self.norm_param(n, l, "gamma")),
                                           L.ptr(d), L.ptr(gg), L.ptr(gb), L.ptr(ws["ln_scratch"]) if gg is not None else None, st))

    @torch.no_grad()
    def forward_raw(self, x_pad):
        """x_pad (M, ld(in)) with zero pad columns -> Q (2, M, 32) (column 0).  Keeps z / y / mean / rstd of every layer for
        `backward_raw`."""
        return self._q_of(self._forward_layers(x_pad))

    # ---- reference surface: no train / eval difference ----------------------------------------------------------
    def _heads(self, state, action):
        return self.forward_raw(self._x_of(state, action))
