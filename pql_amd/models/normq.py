"""`NormTwinQ`: what the normalised twin critics share -- `DoubleQBatchNorm` (CrossQ) and `DoubleQLayerNorm` (DDPG / SAC).

Twin `Linear -> Norm -> ELU -> ... -> Linear` Q heads on `cat(state, action)`.  Every Linear is a one-layer `PqlMlpDesc` call on
the fp32-MFMA GEMMs (forward with the raw pre-activation as output, backward giving dW / db / dX); between two of them a subclass
runs its norm + ELU pass and, going back, that pass's backward.  All parameters -- Linear weights and biases and the norm's gamma /
beta of both nets -- live in ONE flat arena so that the optimiser's global-norm clip + AdamW is a single launch over it and one
`pqlk_polyak` averages a target copy, like the other critics.  state_dict keys are those of the equivalent `nn.Sequential`:
`net_q{1,2}.net.{0,3,6,..}.{weight,bias}` for the Linears, `net_q{1,2}.net.{1,4,7,..}.{weight,bias}` for the norms.

A subclass states its norm step: `_norm_workspace`, `_norm_forward`, `_norm_backward` (and, if it has any, its buffers' keys).
"""
from __future__ import annotations

import ctypes as C
from collections import OrderedDict
from copy import deepcopy

import torch
from torch import nn

from pql_amd import _lib as L
from pql_amd.models.mlp import HIDDEN_DEFAULT, ArenaLayout, _first, default_splits, mlp_backward_raw, pad_cols


class NormTwinQ(nn.Module):
    key_prefixes = ("net_q1.net.", "net_q2.net.")
    num_atoms = 1

    def __init__(self, state_dim, act_dim, hidden_layers=None):
        super().__init__()
        self.state_dim, self.act_dim = _first(state_dim), int(act_dim)
        hidden = list(HIDDEN_DEFAULT if hidden_layers is None else hidden_layers)
        self.dims = [self.state_dim + self.act_dim, *hidden, 1]
        self.n_layers = len(self.dims) - 1
        self.init_kwargs = dict(state_dim=self.state_dim, act_dim=self.act_dim, hidden_layers=hidden)
        self.lin = [ArenaLayout([self.dims[l], self.dims[l + 1]], 1) for l in range(self.n_layers)]   # one-layer descriptors
        # flat arena: per net, per layer: [W (out, ld(in)) | b (ld(out))] then, for hidden layers, [gamma (ld(out)) | beta (ld(out))]
        self.off = {}
        o = 0
        for n in range(2):
            for l in range(self.n_layers):
                self.off[(n, l, "lin")] = o
                o += self.lin[l].total
                if l < self.n_layers - 1:
                    w = L.ld(self.dims[l + 1])
                    self.off[(n, l, "gamma")], self.off[(n, l, "beta")] = o, o + w
                    o += 2 * w
        self.total = o
        self.arena = nn.Parameter(torch.zeros(self.total, dtype=torch.float32))
        self._make_buffers()
        self.reset_parameters()
        self._ws = {}

    def _make_buffers(self):
        """Buffers of the norm (registered after the arena, before the parameters are drawn)."""

    # ---- parameter views -------------------------------------------------------------------------------------
    def weight(self, n, l, arena=None):
        """W of Linear `l` of net `n` (arena: another flat tensor laid out like the arena, e.g. the gradient)."""
        return self.lin[l].weight((self.arena.data if arena is None else arena)[self.off[(n, l, "lin")]:], 0, 0)

    def bias(self, n, l, arena=None):
        return self.lin[l].bias((self.arena.data if arena is None else arena)[self.off[(n, l, "lin")]:], 0, 0)

    def norm_param(self, n, l, which, arena=None):
        """gamma / beta of the norm behind Linear `l` of net `n` (arena: another flat tensor laid out like it, e.g. the gradient)."""
        a = self.arena.data if arena is None else arena
        o = self.off[(n, l, which)]
        return a[o: o + self.dims[l + 1]]

    @torch.no_grad()
    def reset_parameters(self):
        self.arena.zero_()
        for n in range(2):
            for l in range(self.n_layers):
                bound = 1.0 / (self.dims[l] ** 0.5)    # nn.Linear default
                self.weight(n, l).uniform_(-bound, bound)
                self.bias(n, l).uniform_(-bound, bound)
                if l < self.n_layers - 1:
                    self.norm_param(n, l, "gamma").fill_(1.0)
                    self._reset_norm(n, l)

    def _reset_norm(self, n, l):
        pass

    def named_views(self, arena=None):
        """(reference key, view) pairs of the trainable tensors (arena: as for `weight`)."""
        for n, pre in enumerate(self.key_prefixes):
            for l in range(self.n_layers):
                yield f"{pre}{3 * l}.weight", self.weight(n, l, arena)
                yield f"{pre}{3 * l}.bias", self.bias(n, l, arena)
                if l < self.n_layers - 1:
                    yield f"{pre}{3 * l + 1}.weight", self.norm_param(n, l, "gamma", arena)
                    yield f"{pre}{3 * l + 1}.bias", self.norm_param(n, l, "beta", arena)

    def _buffer_state(self, out, prefix):
        """The norm's buffers -> `out` under the reference's keys."""

    def _load_buffer_state(self, state_dict, missing):
        pass

    def state_dict(self, *args, destination=None, prefix="", keep_vars=False, **kw):
        out = OrderedDict() if destination is None else destination
        for k, v in self.named_views():
            out[prefix + k] = v.detach().clone()
        self._buffer_state(out, prefix)
        return out

    @torch.no_grad()
    def load_state_dict(self, state_dict, strict=True, assign=False):
        missing = []
        for k, v in self.named_views():
            if k in state_dict:
                v.copy_(torch.as_tensor(state_dict[k]).to(v.device, torch.float32))
            else:
                missing.append(k)
        self._load_buffer_state(state_dict, missing)
        if strict and missing:
            raise RuntimeError(f"Missing key(s) in state_dict: {missing}")
        return nn.modules.module._IncompatibleKeys(missing, [])

    def num_params(self):
        return sum(v.numel() for _, v in self.named_views())

    def __deepcopy__(self, memo):
        """A copy (a target critic) gets its own, empty workspace: its forward must not disturb what this one's backward reads."""
        new = self.__class__.__new__(self.__class__)
        memo[id(self)] = new
        for k, v in self.__dict__.items():
            new.__dict__[k] = {} if k == "_ws" else deepcopy(v, memo)
        return new

    # ---- raw launch sequences --------------------------------------------------------------------------------
    def _norm_workspace(self, ws, key, M, w, f):
        """Per (net, hidden layer) tensors of the norm's stash, put into `ws`."""
        raise NotImplementedError

    def _norm_scratch(self, ws, wmax, f):
        """Scratch shared by all layers, put into `ws`."""
        raise NotImplementedError

    def _norm_forward(self, ws, n, l, z, y, M, st, **kw):
        """z (M, ld) -> y = ELU(norm(z)), keeping what `_norm_backward` needs."""
        raise NotImplementedError

    def _norm_backward(self, ws, n, l, d, M, gg, gb, st):
        """d: grad of y, (M, ld) -> grad of z, in place; gg / gb: where dgamma / dbeta go (None: frozen)."""
        raise NotImplementedError

    def _workspace(self, M, dev):
        ws = self._ws.get(M)
        if ws is not None and ws["dev"] == dev:
            return ws
        f = dict(dtype=torch.float32, device=dev)
        ws = dict(dev=dev, z={}, y={}, splits=default_splits(M))
        wmax = max(L.ld(d) for d in self.dims[1:])
        for n in range(2):
            for l in range(self.n_layers):
                w = L.ld(self.dims[l + 1])
                ws["z"][(n, l)] = torch.zeros((M, w), **f)
                if l < self.n_layers - 1:
                    ws["y"][(n, l)] = torch.zeros((M, w), **f)      # pad columns stay zero
                    self._norm_workspace(ws, (n, l), M, w, f)
        self._norm_scratch(ws, wmax, f)
        ws["dcur"] = [torch.zeros((M, wmax), **f) for _ in range(2)]
        ws["dx0"] = [torch.zeros((M, L.ld(self.dims[0])), **f) for _ in range(2)]
        ws["bwd"] = torch.empty(max(lay.bwd_ws_floats(M, ws["splits"]) for lay in self.lin), **f)
        self._ws[M] = ws
        return ws

    @torch.no_grad()
    def _forward_layers(self, x_pad, **kw):
        """x_pad (M, ld(in)) with zero pad columns -> Q (2, M, 32) (column 0); z / y / the norm's stash of every layer are kept."""
        L.require_gpu(self.arena, "parameter arena")
        M, dev = x_pad.shape[0], x_pad.device
        ws = self._workspace(M, dev)
        arena = self.arena.data
        with torch.cuda.device(dev):
            st = L.stream(dev)
            for n in range(2):
                x, ldx = x_pad, x_pad.stride(0)
                for l in range(self.n_layers):
                    lay, z = self.lin[l], ws["z"][(n, l)]
                    L.check(L.lib.pqlk_mlp_forward(C.byref(lay.desc), L.ptr(arena[self.off[(n, l, "lin")]:]), None, 1, L.ptr(x), ldx, M,
                                                   L.ACT_NONE, None, 0.0, 0.0, L.ptr(z), None, 0, st))
                    if l == self.n_layers - 1:
                        break
                    y = ws["y"][(n, l)]
                    self._norm_forward(ws, n, l, z, y, M, st, **kw)
                    x, ldx = y, z.stride(0)
        return ws

    def elu_layers(self):
        """The hidden layers whose norm step ends in an ELU (0-based): what the diagnostics' unit statistics are taken of."""
        return list(range(self.n_layers - 1))

    def elu_output(self, M, dev, n, l):
        """The post-ELU matrix (M, ld) of hidden layer `l` of net `n` as the last forward on M rows left it."""
        return self._workspace(M, dev)["y"][(n, l)]

    def _q_of(self, ws):
        return torch.stack((ws["z"][(0, self.n_layers - 1)], ws["z"][(1, self.n_layers - 1)]))

    @torch.no_grad()
    def backward_raw(self, x_pad, dq, grads=None, need_dx=False):
        """Backward of the LAST `forward_raw` on the same x_pad.  dq (2, M, 32): d loss / d Q (column 0).
        grads: flat tensor like the arena, overwritten with the parameter gradient (None: parameters frozen).
        Returns d loss / d x summed over the nets, (M, ld(in)), when need_dx."""
        M, dev = x_pad.shape[0], x_pad.device
        ws = self._workspace(M, dev)
        arena = self.arena.data
        splits = ws["splits"] if grads is not None else 1
        with torch.cuda.device(dev):
            st = L.stream(dev)
            for n in range(2):
                dcur = dq[n]
                for l in range(self.n_layers - 1, -1, -1):
                    lay = self.lin[l]
                    if l < self.n_layers - 1:   # through ELU and the norm: dcur (grad of y_l) -> dz_l, in place
                        gg = self.norm_param(n, l, "gamma", grads) if grads is not None else None
                        gb = self.norm_param(n, l, "beta", grads) if grads is not None else None
                        self._norm_backward(ws, n, l, dcur, M, gg, gb, st)
                    x_in = x_pad if l == 0 else ws["y"][(n, l - 1)]
                    if l > 0:      # grad of y_{l-1}: ping-pong buffers, viewed with that layer's row stride
                        w_in = x_in.stride(0)
                        dx = ws["dcur"][l & 1].view(-1)[: M * w_in].view(M, w_in)
                    else:
                        dx = ws["dx0"][n] if need_dx else None
                    g_lin = grads[self.off[(n, l, "lin")]:] if grads is not None else None
                    mlp_backward_raw(lay, arena[self.off[(n, l, "lin")]:], x_in, ws["z"][(n, l)], dcur, ws["bwd"], g_lin, splits, dx, rows=M)
                    dcur = dx
            if need_dx:
                return ws["dx0"][0] + ws["dx0"][1]
        return None

    # ---- reference surface -------------------------------------------------------------------------------------
    def _heads(self, state, action):
        raise NotImplementedError

    def _x_of(self, state, action):
        return pad_cols(torch.cat((state, action), dim=1).to(torch.float32), L.ld(self.dims[0]))

    def get_q1_q2(self, state, action):
        q = self._heads(state, action)
        return q[0, :, :1].clone(), q[1, :, :1].clone()

    def get_q_min(self, state, action):
        return torch.min(*self.get_q1_q2(state, action))

    def get_q1(self, state, action):
        return self._heads(state, action)[0, :, :1].clone()
