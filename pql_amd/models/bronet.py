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

`fused_forward=True` (`algo.bronet_fused_forward`): the forward is ONE launch for both nets and all 2 K + 2 layers, `pqlk_bro_forward`
(pql_amd/csrc/fwd_bro.hip, the law in include/pqlk.h), reading the arena as it lies and carrying the residual stream in registers.
With `stash` it leaves z / y / mean / rstd of every hidden layer in one slab of which `ws["z"]`, `ws["y"]`, `ws["mean"]`, `ws["rstd"]`
are views, so `backward_raw`, `elu_layers` and `elu_output` are what they were; without (a target forward) nothing but Q is written.
The switch is no part of a checkpoint and not in `init_kwargs`.

`target_dtype="bfloat16"` (`algo.critic_target_dtype`, with `fused_forward` only): the module also owns `packed`, the fragment-ordered
bf16 copy of its weights as int16 (`pqlk_bro_pack_bf16`; never saved, not in `init_kwargs`), and `forward_raw(x, stash=False)` is the
bf16-MFMA launch `pqlk_bro_forward_bf16` (pql_amd/csrc/fwd_bro_bf16.hip): the Linears' operands are rounded, the residual stream stays
fp32 in registers.  `refresh()` must run behind every change of the arena; a forward with a stash stays the fp32 launch.
"""
from __future__ import annotations

import ctypes as C

import torch

from pql_amd import _lib as L
from pql_amd.models.layernorm import LN_EPS, TARGET_DTYPE_KEY, DoubleQLayerNorm, check_target_dtype_value
from pql_amd.models.mlp import _first

MAX_BLOCKS = 16
BRO_FUSED_KEY = "algo.bronet_fused_forward"


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


def check_bool_bro_fused(v):
    if not isinstance(v, bool):
        raise ValueError(f"{BRO_FUSED_KEY} must be True or False, got {v!r}")


def check_bro_fused(in_dim, width, blocks):
    """`algo.bronet_fused_forward=True` on a stack the one-launch forward does not take: refused, never a silent per-layer run."""
    if not L.lib.pqlk_bro_ok(int(in_dim), int(width), int(blocks), 2):
        raise ValueError(f"{BRO_FUSED_KEY}=True cannot run a residual critic of width {width} and {blocks} blocks on {in_dim} inputs: the "
                         f"one-launch forward takes algo.critic_width a multiple of 32 and at most 1024, 0 to {MAX_BLOCKS} blocks and an "
                         f"input of at most 1248 padded columns; set {BRO_FUSED_KEY}=False for the per-layer forward")


def check_bro_target_bf16(in_dim, width, blocks, fused_forward):
    """`algo.critic_target_dtype=bfloat16` where the residual critic's bf16 target forward cannot run: refused, never a silent fp32 run."""
    if not fused_forward:
        raise ValueError(f"{TARGET_DTYPE_KEY}=bfloat16 needs {BRO_FUSED_KEY}=True with DoubleQBroNet: the bf16 target forward is a form of "
                         f"the one-launch forward (the per-layer forward has no bf16 kernels)")
    if not L.lib.pqlk_bro_bf16_ok(int(in_dim), int(width), int(blocks), 2):
        raise ValueError(f"{TARGET_DTYPE_KEY}=bfloat16 cannot run a residual critic of width {width} and {blocks} blocks on {in_dim} inputs: "
                         f"the bf16 target forward takes what {BRO_FUSED_KEY}=True takes (algo.critic_width a multiple of 32 and at most "
                         f"1024); set {TARGET_DTYPE_KEY}=float32")


class DoubleQBroNet(DoubleQLayerNorm):
    key_prefixes = ("net_q1.", "net_q2.")

    def __init__(self, state_dim, act_dim, width=512, blocks=2, fused_forward=False, target_dtype="float32"):
        self.width, self.blocks = check_width(width), check_blocks(blocks)   # before anything is allocated
        check_bool_bro_fused(fused_forward)
        check_target_dtype_value(target_dtype)
        if fused_forward:
            check_bro_fused(_first(state_dim) + int(act_dim), self.width, self.blocks)
        if target_dtype == "bfloat16":
            check_bro_target_bf16(_first(state_dim) + int(act_dim), self.width, self.blocks, fused_forward)
        super().__init__(state_dim, act_dim, hidden_layers=[self.width] * (2 * self.blocks + 1))
        self.init_kwargs = dict(state_dim=self.state_dim, act_dim=self.act_dim, width=self.width, blocks=self.blocks)
        # None: the per-layer forward, no fused state anywhere; else what every pqlk_bro_* entry is told about the stack
        self.fused = (self.dims[0], self.width, self.blocks, 2) if fused_forward else None
        if self.fused is not None:   # the library's statement of the arena law is this module's
            assert int(L.lib.pqlk_bro_param_floats(*self.fused)) == self.total
            for l in range(self.n_layers):
                offs = [C.c_int64() for _ in range(3)]
                L.check(L.lib.pqlk_bro_offsets(*self.fused[:3], l, *(C.byref(o) for o in offs)))
                assert [o.value for o in offs] == [self.off.get((0, l, k), -1) for k in ("lin", "gamma", "beta")]
        if target_dtype == "bfloat16":   # a buffer, so that it moves with the module; state_dict is the views' alone: never saved
            del self.packed              # (the base class left None: every forward fp32)
            self.register_buffer("packed", torch.zeros(int(L.lib.pqlk_bro_packed_bf16_elems(*self.fused)), dtype=torch.int16),
                                 persistent=False)

    def refresh(self):
        """The packed bf16 copy <- the arena as it is now: one launch on the current stream, behind whatever changed the arena."""
        if self.packed is None:
            raise ValueError(f"refresh() is the packed bf16 copy's: it needs {TARGET_DTYPE_KEY}=bfloat16")
        L.require_gpu(self.arena, "parameter arena")
        dev = self.arena.device
        with torch.cuda.device(dev):
            L.check(L.lib.pqlk_bro_pack_bf16(*self.fused, L.ptr(self.arena.data), L.ptr(self.packed), L.stream(dev)))
        self._packed_fresh = True
        return self

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

    def _stash(self, ws, M, f):
        """Fused: one slab, laid out by `pqlk_bro_stash_offset`, and the (2, M, 32) Q block; z / y / mean / rstd are views of them."""
        if self.fused is None:
            return super()._stash(ws, M, f)
        sizes, W = self.fused[1:], self.width
        slab = torch.zeros(int(L.lib.pqlk_bro_stash_floats(*sizes, M)), **f)
        ws.update(stash=slab, q=torch.zeros((2, M, 32), **f), mean={}, rstd={})
        if self.blocks:
            ws["skip"] = torch.zeros((M, W), **f)    # (the per-layer path makes it in _norm_workspace, which is not reached here)

        def view(n, l, which, *shape):
            off, ld = C.c_int64(), C.c_int64()
            L.check(L.lib.pqlk_bro_stash_offset(*sizes, M, n, l, which, C.byref(off), C.byref(ld)))
            return slab[off.value: off.value + M * ld.value].view(*shape)

        H = self.n_layers - 1
        for n in range(2):
            for l in range(H):
                ws["z"][(n, l)], ws["y"][(n, l)] = view(n, l, L.LNMLP_Z, M, W), view(n, l, L.LNMLP_Y, M, W)
                ws["mean"][(n, l)], ws["rstd"][(n, l)] = view(n, l, L.LNMLP_MEAN, M), view(n, l, L.LNMLP_RSTD, M)
            ws["z"][(n, H)] = ws["q"][n]

    def _fused_forward(self, x_pad, stash):
        """The one launch.  stash: into the workspace `backward_raw` reads; else Q alone, into a block that is no part of it."""
        L.require_gpu(self.arena, "parameter arena")
        M, dev = x_pad.shape[0], x_pad.device
        if stash:
            ws = self._workspace(M, dev)
            slab, q = ws["stash"], ws["q"]
        else:
            slab, q = None, self._ws.get(("q", M))
            if q is None or q.device != dev:
                q = self._ws[("q", M)] = torch.zeros((2, M, 32), dtype=torch.float32, device=dev)
            if self.packed is not None:   # algo.critic_target_dtype=bfloat16: the forward nothing goes back through, on bf16 MFMA
                if not self._packed_fresh:
                    raise RuntimeError("forward_raw(stash=False) reads the packed bf16 copy, which was never written: call refresh() "
                                       "behind every change of the arena")
                with torch.cuda.device(dev):
                    L.check(L.lib.pqlk_bro_forward_bf16(*self.fused, L.ptr(self.arena.data), L.ptr(self.packed), L.ptr(x_pad),
                                                        x_pad.stride(0), M, LN_EPS, L.ptr(q), L.stream(dev)))
                return q
        with torch.cuda.device(dev):
            L.check(L.lib.pqlk_bro_forward(*self.fused, L.ptr(self.arena.data), L.ptr(x_pad), x_pad.stride(0), M, LN_EPS, L.ptr(slab),
                                           L.ptr(q), L.stream(dev)))
        return q

    @torch.no_grad()
    def forward_raw(self, x_pad, stash=True):
        """As `DoubleQLayerNorm.forward_raw`; stash=False is the one-launch forward's (fused_forward only)."""
        if self.fused is None and not stash:
            raise ValueError(f"forward_raw(stash=False) is the one-launch forward's: it needs {BRO_FUSED_KEY}=True")
        return super().forward_raw(x_pad, stash)

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
