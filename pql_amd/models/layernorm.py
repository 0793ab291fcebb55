"""`DoubleQLayerNorm`: a LayerNorm twin critic for DDPG and SAC: twin `Linear -> LayerNorm(eps=1e-5, affine) -> ELU -> ... -> Linear`
Q heads on `cat(state, action)` (the reference only hints at it: a commented-out critic at pql/models/mlp.py:288-310).

LayerNorm is row-local, so -- unlike the BatchNorm critic of CrossQ -- it works with target critics and at any batch size and
behaves the same in training and evaluation.  The arena, the views, the state_dict plumbing, the workspace and the per-layer GEMM
loops are `NormTwinQ`'s (pql_amd/models/normq.py); the norm step is `pqlk_ln_elu_forward / _backward` (pql_amd/csrc/ln.hip, the law
in include/pqlk.h).  state_dict keys are those of the equivalent `nn.Sequential`: `net_q{1,2}.net.{0,3,6,9}.{weight,bias}` for the
Linears, `net_q{1,2}.net.{1,4,7}.{weight,bias}` for the norms; there are no buffers.

`fused_forward=True` (`algo.critic_fused_forward`): the forward is ONE launch for both nets and every layer, `pqlk_lnmlp_forward`
(pql_amd/csrc/fwd_ln.hip, the law in include/pqlk.h), reading the arena as it lies.  With `stash` it leaves z / y / mean / rstd of
every hidden layer in one slab of which `ws["z"]`, `ws["y"]`, `ws["mean"]`, `ws["rstd"]` are views, so `backward_raw` and
`elu_output` are what they were; without (a target forward) nothing but Q is written.  The switch is no part of a checkpoint.

`target_dtype="bfloat16"` (`algo.critic_target_dtype`, with `fused_forward` only): the module also owns `packed`, the fragment-ordered
bf16 copy of its weights as int16 (`pqlk_lnmlp_pack_bf16`; never saved), and `forward_raw(x, stash=False)` is the bf16-MFMA launch
`pqlk_lnmlp_forward_bf16` (pql_amd/csrc/fwd_ln_bf16.hip) reading it.  `refresh()` must run behind every change of the arena; a forward
with a stash stays the fp32 launch.

`fused_dx=True` (`algo.critic_fused_dx`, with `fused_forward` only): the way back to the input with the parameters frozen -- the actor
step's `backward_raw(grads=None, need_dx=True)` -- is ONE launch for both nets and every layer, `pqlk_lnmlp_dx`
(pql_amd/csrc/bwd_ln.hip, the law in include/pqlk.h), reading the slab the last stash forward wrote; `fused_dx(...)` is that call, in
its plain form or through the actor's tanh.  A backward that forms parameter gradients stays the per-layer one.  No part of a checkpoint.

`fused_backward=True` (`algo.critic_fused_backward`, with `fused_forward` only): the critic's own update,
`backward_raw(grads=<tensor>, need_dx=False)`, is ONE `pqlk_lnmlp_grad_chain` call -- a chain launch that leaves dz of every net and
hidden layer in the workspace slab `ws["grad_ws"]` and the column sums of dgamma / dbeta per 32-row tile, and a fold launch that
writes dgamma / dbeta into `grads` (pql_amd/csrc/bwd_ln.hip, the law in include/pqlk.h) -- and then the 2 (H + 1) weight-gradient
GEMMs `mlp_backward_raw(..., dx=None)` on those dz: no per-layer norm backward, no dX product.  No part of a checkpoint.
"""
from __future__ import annotations

import ctypes as C

import torch

from pql_amd import _lib as L
from pql_amd.models.mlp import HIDDEN_DEFAULT, _first, mlp_backward_raw
from pql_amd.models.normq import NormTwinQ

LN_EPS = 1e-5   # nn.LayerNorm default


FUSED_KEY = "algo.critic_fused_forward"
TARGET_DTYPE_KEY = "algo.critic_target_dtype"
FUSED_DX_KEY = "algo.critic_fused_dx"
FUSED_BACKWARD_KEY = "algo.critic_fused_backward"
TARGET_DTYPES = ("float32", "bfloat16")


def lnmlp_desc(dims, n_nets=2) -> L.PqlMlpDesc:
    """The descriptor of the whole stack for `pqlk_lnmlp_*` (any `dims`: an ineligible one is what `pqlk_lnmlp_ok` refuses)."""
    d = L.PqlMlpDesc()
    d.n_layers, d.n_nets = len(dims) - 1, n_nets
    for i, x in enumerate(dims[:L.MAX_LAYERS + 1]):
        d.dims[i] = int(x)
    return d


def check_fused_forward(dims, key=FUSED_KEY):
    """`algo.critic_fused_forward=True` on a stack the one-launch forward does not take: refused, never a silent per-layer run.
    key: the switch of the class that asks (the dropout critic has its own, `algo.droq_fused_forward`)."""
    if not L.lib.pqlk_lnmlp_ok(C.byref(lnmlp_desc(dims))):
        raise ValueError(f"{key}=True cannot run a critic of layers {list(dims)}: the one-launch forward takes 1 to "
                         f"{L.MAX_LAYERS - 1} hidden layers whose widths are multiples of 32 and at most 1024, on an input of at most 1248 "
                         f"padded columns; set {key}=False for the per-layer forward")


def check_target_dtype_value(v):
    if v not in TARGET_DTYPES:
        raise ValueError(f"{TARGET_DTYPE_KEY} must be float32 or bfloat16, got {v!r}")


def check_target_bf16(dims, fused_forward, key=FUSED_KEY):
    """`algo.critic_target_dtype=bfloat16` where the bf16 target forward cannot run: refused, never a silent fp32 run."""
    if not fused_forward:
        raise ValueError(f"{TARGET_DTYPE_KEY}=bfloat16 needs {key}=True: the bf16 target forward is a form of the one-launch forward "
                         f"(the per-layer forward has no bf16 kernels)")
    if not L.lib.pqlk_lnmlp_bf16_ok(C.byref(lnmlp_desc(dims))):
        raise ValueError(f"{TARGET_DTYPE_KEY}=bfloat16 cannot run a critic of layers {list(dims)}: the bf16 image of 32 batch rows of its "
                         f"widest layer does not fit the LDS; set {TARGET_DTYPE_KEY}=float32")


def check_fused_dx(fused_forward, key=FUSED_KEY):
    """`algo.critic_fused_dx=True` without the one-launch forward: refused, never a silent per-layer run."""
    if not fused_forward:
        raise ValueError(f"{FUSED_DX_KEY}=True needs {key}=True: the one-launch input gradient reads the stash slab as the one-launch "
                         f"forward lays it out (the per-layer forward keeps a tensor per layer)")


def check_fused_backward(fused_forward, key=FUSED_KEY):
    """`algo.critic_fused_backward=True` without the one-launch forward: refused, never a silent per-layer run."""
    if not fused_forward:
        raise ValueError(f"{FUSED_BACKWARD_KEY}=True needs {key}=True: the one-launch gradient chain reads the stash slab as the one-launch "
                         f"forward lays it out (the per-layer forward keeps a tensor per layer)")


class DoubleQLayerNorm(NormTwinQ):
    fused_key = FUSED_KEY   # the config key of this class's `fused_forward`, for its messages
    grad_r = 0              # rows per block / 32 of the gradient chain's launch (0: the library's choice; a knob for measurements)

    def __init__(self, state_dim, act_dim, hidden_layers=None, fused_forward=False, target_dtype="float32", fused_dx=False,
                 fused_backward=False):
        dims = [_first(state_dim) + int(act_dim), *(HIDDEN_DEFAULT if hidden_layers is None else hidden_layers), 1]
        check_target_dtype_value(target_dtype)
        if fused_forward:   # before anything is allocated
            check_fused_forward(dims, self.fused_key)
        if target_dtype == "bfloat16":
            check_target_bf16(dims, fused_forward, self.fused_key)
        if fused_dx:
            check_fused_dx(fused_forward, self.fused_key)
        if fused_backward:
            check_fused_backward(fused_forward, self.fused_key)
        super().__init__(state_dim, act_dim, hidden_layers)
        self.fused = lnmlp_desc(self.dims) if fused_forward else None   # None: the per-layer forward, no fused state anywhere
        if self.fused is not None:   # the library's statement of the arena law is this module's
            assert int(L.lib.pqlk_lnmlp_param_floats(C.byref(self.fused))) == self.total
            for l in range(self.n_layers):
                offs = [C.c_int64() for _ in range(3)]
                L.check(L.lib.pqlk_lnmlp_offsets(C.byref(self.fused), l, *(C.byref(o) for o in offs)))
                assert [o.value for o in offs] == [self.off.get((0, l, k), -1) for k in ("lin", "gamma", "beta")]
        self.fused_dx_on = bool(fused_dx)   # backward_raw(grads=None, need_dx=True) is the one launch
        self.fused_backward_on = bool(fused_backward)   # backward_raw(grads=<tensor>, need_dx=False) is the chain call + the dW GEMMs
        self._packed_fresh = False
        if target_dtype == "bfloat16":   # a buffer, so that it moves with the module; state_dict is the views' alone: never saved
            self.register_buffer("packed", torch.zeros(int(L.lib.pqlk_lnmlp_packed_bf16_elems(C.byref(self.fused))), dtype=torch.int16),
                                 persistent=False)
        else:
            self.packed = None   # every forward is fp32, no packed state anywhere

    def refresh(self):
        """The packed bf16 copy <- the arena as it is now: one launch on the current stream, behind whatever changed the arena."""
        if self.packed is None:
            raise ValueError(f"refresh() is the packed bf16 copy's: it needs {TARGET_DTYPE_KEY}=bfloat16")
        L.require_gpu(self.arena, "parameter arena")
        dev = self.arena.device
        with torch.cuda.device(dev):
            L.check(L.lib.pqlk_lnmlp_pack_bf16(C.byref(self.fused), L.ptr(self.arena.data), L.ptr(self.packed), L.stream(dev)))
        self._packed_fresh = True
        return self

    @torch.no_grad()
    def load_state_dict(self, state_dict, strict=True, assign=False):
        out = super().load_state_dict(state_dict, strict, assign)
        if self.packed is not None and self.arena.is_cuda:
            self.refresh()
        return out

    def _norm_workspace(self, ws, key, M, w, f):
        ws.setdefault("mean", {})[key] = torch.zeros(M, **f)
        ws.setdefault("rstd", {})[key] = torch.zeros(M, **f)

    def _norm_scratch(self, ws, wmax, f):
        ws["ln_scratch"] = torch.zeros(int(L.lib.pqlk_ln_scratch_floats(wmax)), **f)

    def _stash(self, ws, M, f):
        """Fused: one slab, laid out by `pqlk_lnmlp_stash_offset`, and the (2, M, 32) Q block; z / y / mean / rstd are views of them."""
        if self.fused is None:
            return super()._stash(ws, M, f)
        d, H = self.fused, self.n_layers - 1
        slab = torch.zeros(int(L.lib.pqlk_lnmlp_stash_floats(C.byref(d), M)), **f)
        ws.update(stash=slab, q=torch.zeros((2, M, 32), **f), mean={}, rstd={})

        def view(n, l, which, *shape):
            off, ld = C.c_int64(), C.c_int64()
            L.check(L.lib.pqlk_lnmlp_stash_offset(C.byref(d), M, n, l, which, C.byref(off), C.byref(ld)))
            return slab[off.value: off.value + M * ld.value].view(*shape)

        for n in range(2):
            for l in range(H):
                w = self.dims[l + 1]
                ws["z"][(n, l)], ws["y"][(n, l)] = view(n, l, L.LNMLP_Z, M, w), view(n, l, L.LNMLP_Y, M, w)
                ws["mean"][(n, l)], ws["rstd"][(n, l)] = view(n, l, L.LNMLP_MEAN, M), view(n, l, L.LNMLP_RSTD, M)
            ws["z"][(n, H)] = ws["q"][n]
        if self.fused_backward_on:   # dz of every (net, hidden layer) and the tiles' partial rows, laid out by `pqlk_lnmlp_grad_offset`
            gw = ws["grad_ws"] = torch.zeros(int(L.lib.pqlk_lnmlp_grad_ws_floats(C.byref(d), M)), **f)
            ws["dz"] = {}
            for n in range(2):
                for l in range(H):
                    off, ld = C.c_int64(), C.c_int64()
                    L.check(L.lib.pqlk_lnmlp_grad_offset(C.byref(d), M, n, l, C.byref(off), C.byref(ld)))
                    ws["dz"][(n, l)] = gw[off.value: off.value + M * ld.value].view(M, ld.value)

    def _norm_forward(self, ws, n, l, z, y, M, st):
        L.check(L.lib.pqlk_ln_elu_forward(L.ptr(z), z.stride(0), M, self.dims[l + 1], L.ptr(self.norm_param(n, l, "gamma")),
                                          L.ptr(self.norm_param(n, l, "beta")), LN_EPS, L.ptr(y), L.ptr(ws["mean"][(n, l)]),
                                          L.ptr(ws["rstd"][(n, l)]), st))

    def _norm_backward(self, ws, n, l, d, M, gg, gb, st):
        z = ws["z"][(n, l)]
        L.check(L.lib.pqlk_ln_elu_backward(L.ptr(d), L.ptr(ws["y"][(n, l)]), L.ptr(z), z.stride(0), M, self.dims[l + 1],
                                           L.ptr(ws["mean"][(n, l)]), L.ptr(ws["rstd"][(n, l)]), L.ptr(self.norm_param(n, l, "gamma")),
                                           L.ptr(d), L.ptr(gg), L.ptr(gb), L.ptr(ws["ln_scratch"]) if gg is not None else None, st))

    def _fused_forward(self, x_pad, stash, drop=None):
        """The one launch.  stash: into the workspace `backward_raw` reads; else Q alone, into a block that is no part of it.
        drop (the dropout subclass, pql_amd/models/droq.py): (p, seed, tag_base) -- the `pqlk_lnmlp_drop_*` form of the same launch."""
        fp32, bf16 = (L.lib.pqlk_lnmlp_forward, L.lib.pqlk_lnmlp_forward_bf16) if drop is None else \
            (L.lib.pqlk_lnmlp_drop_forward, L.lib.pqlk_lnmlp_drop_forward_bf16)
        drop = () if drop is None else drop
        L.require_gpu(self.arena, "parameter arena")
        M, dev = x_pad.shape[0], x_pad.device
        if stash:
            ws = self._workspace(M, dev)
            slab, q = ws["stash"], ws["q"]
        else:
            q = self._ws.get(("q", M))
            if q is None or q.device != dev:
                q = self._ws[("q", M)] = torch.zeros((2, M, 32), dtype=torch.float32, device=dev)
            slab = None
            if self.packed is not None:   # algo.critic_target_dtype=bfloat16: the forward nothing goes back through, on bf16 MFMA
                if not self._packed_fresh:
                    raise RuntimeError("forward_raw(stash=False) reads the packed bf16 copy, which was never written: call refresh() "
                                       "behind every change of the arena")
                with torch.cuda.device(dev):
                    L.check(bf16(C.byref(self.fused), L.ptr(self.arena.data), L.ptr(self.packed), L.ptr(x_pad), x_pad.stride(0), M, LN_EPS,
                                 *drop, L.ptr(q), L.stream(dev)))
                return q
        with torch.cuda.device(dev):
            L.check(fp32(C.byref(self.fused), L.ptr(self.arena.data), L.ptr(x_pad), x_pad.stride(0), M, LN_EPS, *drop, L.ptr(slab), L.ptr(q),
                         L.stream(dev)))
        return q

    @torch.no_grad()
    def forward_raw(self, x_pad, stash=True):
        """x_pad (M, ld(in)) with zero pad columns -> Q (2, M, 32) (column 0).  Keeps z / y / mean / rstd of every layer for
        `backward_raw`.  stash=False (fused_forward only; a forward nothing goes back through, the target's): Q alone -- with
        target_dtype="bfloat16" by the bf16 law of include/pqlk.h, from the packed copy `refresh()` last wrote."""
        if self.fused is not None:
            return self._fused_forward(x_pad, stash)
        if not stash:
            raise ValueError(f"forward_raw(stash=False) is the one-launch forward's: it needs {self.fused_key}=True")
        return self._q_of(self._forward_layers(x_pad))

    @torch.no_grad()
    def fused_dx(self, dq, out, col0=None, cols=None, tanh_of=None, r=0):
        """The one launch back to the input, parameters frozen, on the slab of the LAST `forward_raw(x, stash=True)` on dq.shape[1] rows.
        dq (2, M, 32): d loss / d Q (column 0).  Plain: out (M, >= ld(in)) <- d loss / d x summed over the nets, pad columns zero.
        tanh_of (M, ld_a), with col0 and cols: out[:, :cols] <- the columns [col0, col0 + cols) times 1 - tanh_of^2; the rest of `out`
        stays.  r: rows per block / 32 (0: the library's choice)."""
        if self.fused is None:
            check_fused_dx(False, self.fused_key)
        M, dev = dq.shape[1], dq.device
        ws = self._workspace(M, dev)
        if tanh_of is None:
            col0 = cols = ld_a = 0
        else:
            ld_a = tanh_of.stride(0)
        with torch.cuda.device(dev):
            L.check(L.lib.pqlk_lnmlp_dx(C.byref(self.fused), L.ptr(self.arena.data), L.ptr(ws["stash"]), L.ptr(dq), M, L.ptr(out),
                                        out.stride(0), int(col0), int(cols), L.ptr(tanh_of), ld_a, int(r), L.stream(dev)))
        return out

    @torch.no_grad()
    def fused_grad_chain(self, dq, grads, r=0):
        """`pqlk_lnmlp_grad_chain` on the slab of the LAST `forward_raw(x, stash=True)` on dq.shape[1] rows: dz of every net and hidden
        layer into `ws["dz"]`, dgamma / dbeta into their slots of `grads` (laid out like the arena; nothing else of it is written).
        r: rows per block / 32 (0: the library's choice)."""
        if not self.fused_backward_on:
            raise ValueError(f"fused_grad_chain is the one-launch gradient chain's: it needs {FUSED_BACKWARD_KEY}=True")
        M, dev = dq.shape[1], dq.device
        ws = self._workspace(M, dev)
        with torch.cuda.device(dev):
            L.check(L.lib.pqlk_lnmlp_grad_chain(C.byref(self.fused), L.ptr(self.arena.data), L.ptr(ws["stash"]), L.ptr(dq), M,
                                                L.ptr(ws["grad_ws"]), ws["grad_ws"].numel(), L.ptr(grads), int(r), L.stream(dev)))
        return ws["dz"]

    def _fused_backward(self, x_pad, dq, grads):
        """The critic's own update: the chain call, then the weight-gradient GEMMs of every layer on its dz (no dX product anywhere)."""
        M, H = x_pad.shape[0], self.n_layers - 1
        ws = self._workspace(M, x_pad.device)
        dz = self.fused_grad_chain(dq, grads, self.grad_r)
        arena = self.arena.data
        for n in range(2):
            for l in range(H, -1, -1):
                o = self.off[(n, l, "lin")]
                mlp_backward_raw(self.lin[l], arena[o:], x_pad if l == 0 else ws["y"][(n, l - 1)], ws["z"][(n, l)],
                                 dq[n] if l == H else dz[(n, l)], ws["bwd"], grads[o:], ws["splits"], None, rows=M)

    @torch.no_grad()
    def backward_raw(self, x_pad, dq, grads=None, need_dx=False):
        """`NormTwinQ.backward_raw`; with `fused_dx` the frozen-parameter way back to the input is the one launch (the result is a
        workspace tensor, valid until the next such call on as many rows); with `fused_backward` the update's parameter gradient
        (grads given, no dx wanted) is the chain call and the weight-gradient GEMMs."""
        if self.fused_backward_on and grads is not None and not need_dx:
            return self._fused_backward(x_pad, dq, grads)
        if self.fused_dx_on and grads is None and need_dx:
            return self.fused_dx(dq, self._workspace(x_pad.shape[0], x_pad.device)["dx0"][0])
        return super().backward_raw(x_pad, dq, grads, need_dx)

    # ---- reference surface: no train / eval difference ----------------------------------------------------------
    def _heads(self, state, action):
        return self.forward_raw(self._x_of(state, action))
