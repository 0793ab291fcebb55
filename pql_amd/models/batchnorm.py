"""`DoubleQBatchNorm`: the CrossQ critic (reference pql/models/mlp.py:224-241 with `create_simple_mlp(use_batchnorm=True)`,
:15-24): twin `Linear -> BatchNorm1d -> ELU -> ... -> Linear` Q heads on `cat(state, action)`.

MI355X form: the arena, the views, the state_dict plumbing, the workspace and the per-layer GEMM loops are `NormTwinQ`'s
(pql_amd/models/normq.py); what is stated here is the norm step: the batch statistics are one `pqlk_batch_moments` launch per
(net, layer), and the normalise + ELU pass, its backward and the column sums it needs are `pqlk_bn_elu_forward / _backward`
(pql_amd/csrc/bn.hip).  state_dict keys are the reference's (`net_q{1,2}.net.{0,3,6,9}.{weight,bias}` for the Linears,
`net_q{1,2}.net.{1,4,7}.{weight,bias,running_mean,running_var,num_batches_tracked}` for the norms).
"""
from __future__ import annotations

import torch

from pql_amd import _lib as L
from pql_amd.models.normq import NormTwinQ

BN_EPS, BN_MOMENTUM = 1e-5, 0.1   # nn.BatchNorm1d defaults


class DoubleQBatchNorm(NormTwinQ):
    def _make_buffers(self):
        # running statistics: per net, per hidden layer [running_mean (ld) | running_var (ld)]
        self.soff = {}
        o = 0
        for n in range(2):
            for l in range(self.n_layers - 1):
                w = L.ld(self.dims[l + 1])
                self.soff[(n, l)] = (o, o + w)
                o += 2 * w
        self.register_buffer("stats", torch.zeros(o, dtype=torch.float32))
        self.register_buffer("num_batches_tracked", torch.zeros(2 * (self.n_layers - 1), dtype=torch.int64))

    bn_param = NormTwinQ.norm_param

    def running(self, n, l, which):
        o = self.soff[(n, l)][0 if which == "mean" else 1]
        return self.stats[o: o + self.dims[l + 1]]

    def _reset_norm(self, n, l):
        self.running(n, l, "var").fill_(1.0)

    def _buffer_state(self, out, prefix):
        for n, pre in enumerate(self.key_prefixes):
            for l in range(self.n_layers - 1):
                out[f"{prefix}{pre}{3 * l + 1}.running_mean"] = self.running(n, l, "mean").clone()
                out[f"{prefix}{pre}{3 * l + 1}.running_var"] = self.running(n, l, "var").clone()
                out[f"{prefix}{pre}{3 * l + 1}.num_batches_tracked"] = self.num_batches_tracked[n * (self.n_layers - 1) + l].clone()

    def _load_buffer_state(self, state_dict, missing):
        for n, pre in enumerate(self.key_prefixes):
            for l in range(self.n_layers - 1):
                for which in ("mean", "var"):
                    k = f"{pre}{3 * l + 1}.running_{which}"
                    if k in state_dict:
                        self.running(n, l, which).copy_(torch.as_tensor(state_dict[k]).to(self.stats.device, torch.float32))
                    else:
                        missing.append(k)
                k = f"{pre}{3 * l + 1}.num_batches_tracked"
                if k in state_dict:
                    self.num_batches_tracked[n * (self.n_layers - 1) + l] = int(state_dict[k])

    # ---- the norm step -----------------------------------------------------------------------------------------
    def _norm_workspace(self, ws, key, M, w, f):
        ws.setdefault("mean", {})[key] = torch.zeros(w, **f)
        ws.setdefault("var", {})[key] = torch.ones(w, **f)

    def _norm_scratch(self, ws, wmax, f):
        ws["mom_scratch"] = torch.zeros(64 * wmax * 3, **f)
        ws["bn_scratch"] = torch.zeros(128 * wmax, **f)

    def _norm_forward(self, ws, n, l, z, y, M, st, training=True):
        cols, w = self.dims[l + 1], z.stride(0)
        mean, var = ws["mean"][(n, l)], ws["var"][(n, l)]
        if training:
            L.check(L.lib.pqlk_batch_moments(L.ptr(z), w, M, cols, L.ptr(mean), L.ptr(var), L.ptr(ws["mom_scratch"]), st))
        rm, rv = self.running(n, l, "mean"), self.running(n, l, "var")
        L.check(L.lib.pqlk_bn_elu_forward(L.ptr(z), w, M, cols, L.ptr(mean), L.ptr(var), L.ptr(self.norm_param(n, l, "gamma")),
                                          L.ptr(self.norm_param(n, l, "beta")), BN_EPS, 1 if training else 0, BN_MOMENTUM,
                                          L.ptr(rm), L.ptr(rv), L.ptr(y), st))

    def _norm_backward(self, ws, n, l, d, M, gg, gb, st):
        cols, w = self.dims[l + 1], ws["z"][(n, l)].stride(0)
        L.check(L.lib.pqlk_bn_elu_backward(L.ptr(d), L.ptr(ws["y"][(n, l)]), L.ptr(ws["z"][(n, l)]), w, M, cols,
                                           L.ptr(ws["mean"][(n, l)]), L.ptr(ws["var"][(n, l)]), L.ptr(self.norm_param(n, l, "gamma")),
                                           BN_EPS, L.ptr(d), L.ptr(gg), L.ptr(gb), L.ptr(ws["bn_scratch"]), st))

    @torch.no_grad()
    def forward_raw(self, x_pad, training=True):
        """x_pad (M, ld(in)) with zero pad columns -> Q (2, M, 32) (column 0).  Keeps z / y / batch statistics of every layer
        for `backward_raw`; training=True normalises with batch statistics and updates the running ones (momentum 0.1)."""
        ws = self._forward_layers(x_pad, training=training)
        if training:
            self.num_batches_tracked += 1
        return self._q_of(ws)

    # ---- reference surface (inference-style calls; train()/eval() select batch vs running statistics) -----------
    def _heads(self, state, action):
        return self.forward_raw(self._x_of(state, action), training=self.training)
