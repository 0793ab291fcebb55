"""CPU model of the bf16 law of the forward-only bf16-MFMA stack (include/pqlk.h, pql_amd/csrc/fwd_bf16.hip), in torch:

    x~ = bf16(x[:, :dims[0]]);  W~_l = bf16(W_l) for every layer;  z_l = sum_k a~_{l-1,k} W~_l[j,k] + b_l[j];
    hidden a_l = bf16(elu(z_l));  the output layer's z_L stays unrounded and gets out_act.

`forward(..., mode=)`: "f64" accumulates in float64 (the reference of the tests); "f32" is a plain fp32 matmul; "f32rev" sums
16-column chunks in reverse order in fp32 -- two different fixed orders an implementation of the law may use.  bf16 rounding is the
dtype cast (round to nearest even).  Besides the output the f64 model returns, per row, the bound term of the output layer
(sum_k |a~_k| |w~_k| + |b|) and an AMBIGUITY flag: for some hidden pre-activation z < 0, float64 expm1(z) lies within 2^-21
(absolute; four times the stated error of __expf, pql_amd/csrc/gemm.hip:156) of the midpoint between two neighbouring bf16
values, so a correct kernel may round that activation either way.  Positive pre-activations are never ambiguous.
Shared by tests/test_bf16_forward_cpu.py, tests/test_bf16_forward_gpu.py and tests/test_bf16_learner_gpu.py."""
import functools
import math

import torch

ACT_NONE, ACT_TANH, ACT_TANH_NOISE = 0, 1, 2
AMBIG = 2.0 ** -21
BATCHES = (1, 63, 64, 65, 96, 257)
# (dims, n_nets, out_act, ldx or None)
EXACT_CASES = {
    "c24_128_128_1": ([24, 128, 128, 1], 2, ACT_NONE, None),
    "c104_512_256_1": ([104, 512, 256, 1], 2, ACT_NONE, None),
    "c40_128x3_1": ([40, 128, 128, 128, 1], 2, ACT_NONE, None),
    "c24_128_64_51": ([24, 128, 64, 51], 2, ACT_NONE, None),
    "p88_256_128_16_tanh": ([88, 256, 128, 16], 1, ACT_TANH, None),
    "p88_256_128_16_noise": ([88, 256, 128, 16], 1, ACT_TANH_NOISE, None),
    "c136_128_128_1_wide": ([136, 128, 128, 1], 2, ACT_NONE, 256),   # ldx wider than pqlk_ld(136) = 160, garbage past column 136
}
FIRST_FIVE = ("c24_128_128_1", "c104_512_256_1", "c40_128x3_1", "c24_128_64_51", "p88_256_128_16_tanh")
REAL_CASES = {
    "r104_512_512_256_1": ([104, 512, 512, 256, 1], 2, ACT_NONE),
    "r88_512_256_128_16": ([88, 512, 256, 128, 16], 1, ACT_TANH),
    "r136_512_512_256_1": ([136, 512, 512, 256, 1], 2, ACT_NONE),
}
NOISE_STD, NOISE_CLIP = 0.8, 0.2


def bf(t):
    """Round to bf16 (nearest even) and return in the dtype it came in."""
    return t.to(torch.float32).to(torch.bfloat16).to(t.dtype)


def _ambiguous(z64):
    """(B,) flag: some z < 0 of the row has expm1(z) within AMBIG of a bf16 rounding midpoint."""
    e = torch.expm1(z64.clamp(max=0.0))
    e32 = e.to(torch.float32)
    lo_bits = e32.view(torch.int32) & -65536                      # truncated towards zero: the bf16 neighbour of smaller magnitude
    lo = lo_bits.view(torch.float32).double()
    hi = (lo_bits + 65536).view(torch.float32).double()           # ... and the one of larger magnitude
    near = ((e - 0.5 * (lo + hi)).abs() <= AMBIG) & (z64 < 0)
    return near.any(dim=1)


def _matmul(a, w, mode):
    if mode == "f64":
        return a.double() @ w.double().T
    if mode == "f32":
        return a.float() @ w.float().T
    if mode == "f32rev":
        a, w = a.float(), w.float()
        acc = None
        for c in reversed(range(0, a.shape[1], 16)):
            part = a[:, c:c + 16] @ w[:, c:c + 16].T
            acc = part if acc is None else acc + part
        return acc
    raise ValueError(mode)


def forward(dims, W, b, x, out_act=ACT_NONE, draw=None, mode="f64", std=NOISE_STD, clip=NOISE_CLIP):
    """W[net][l] (out, in) and b[net][l] fp32, x (B, >= dims[0]) fp32 -> dict(out (nets, B, N), z (pre-activation of the output
    layer), hidden [net][l] bf16-valued activations as fp32, bound (nets, B, N) = sum |a~||w~| + |b|, ambiguous (B,) bool)."""
    n_nets, nl = len(W), len(dims) - 1
    x0 = bf(x[:, : dims[0]].float())
    outs, zs, hid, bounds = [], [], [], []
    amb = torch.zeros(x.shape[0], dtype=torch.bool)
    for n in range(n_nets):
        a, hs = x0, []
        for l in range(nl):
            wt = bf(W[n][l].float())
            z = _matmul(a, wt, mode) + (b[n][l].double() if mode == "f64" else b[n][l].float())
            if l == nl - 1:
                bounds.append(a.double().abs() @ wt.double().abs().T + b[n][l].double().abs())
                break
            if mode == "f64":
                amb |= _ambiguous(z)
                e = torch.where(z > 0, z, torch.expm1(z))
            else:
                e = torch.where(z > 0, z, torch.exp(z) - 1.0)
            a = bf(e.float())
            hs.append(a)
        y = z
        if out_act in (ACT_TANH, ACT_TANH_NOISE):
            y = torch.tanh(y)
        if out_act == ACT_TANH_NOISE:
            y = _smooth(y, draw, std, clip)
        outs.append(y); zs.append(z); hid.append(hs)
    return dict(out=torch.stack(outs), z=torch.stack(zs), hidden=hid, bound=torch.stack(bounds), ambiguous=amb)


def _smooth(y, draw, std, clip):
    """Target-policy smoothing: clamp(a + clamp(std draw, +-clip), +-1), the product rounded in fp32 as the kernels do."""
    nz = (torch.tensor(std, dtype=torch.float32) * draw.float()).clamp(-clip, clip)
    return (y + nz.to(y.dtype)).clamp(-1.0, 1.0)


def forward_fp32(dims, W, b, x, out_act=ACT_NONE, draw=None, std=NOISE_STD, clip=NOISE_CLIP):
    """The unrounded network (what the fp32 kernels compute), evaluated in float64."""
    outs = []
    for n in range(len(W)):
        a = x[:, : dims[0]].double()
        for l in range(len(dims) - 1):
            a = a @ W[n][l].double().T + b[n][l].double()
            if l < len(dims) - 2:
                a = torch.where(a > 0, a, torch.expm1(a))
        a = torch.tanh(a) if out_act != ACT_NONE else a
        outs.append(_smooth(a, draw, std, clip) if out_act == ACT_TANH_NOISE else a)
    return torch.stack(outs)


def out_tolerance(dims, bound):
    """Forward error bound of an fp32 dot product of K_L terms plus the bias add, in any order: (K_L + 2) 2^-24 (sum |a||w| + |b|)."""
    return (dims[-2] + 2) * 2.0 ** -24 * bound


def _ints(g, shape, lo, hi):
    return torch.randint(lo, hi + 1, shape, generator=g).float()


@functools.lru_cache(maxsize=None)
def exact_case(name, B=257, seed=1):
    """Exact data: every partial sum of the hidden layers is exact in fp32, so every implementation of the law has the same
    hidden activations unless a row is ambiguous.  -> dict(dims, n_nets, out_act, ldx, W, b, x (B, ldx) with garbage past
    dims[0], draw, model (the f64 forward)).  Rows do not depend on B: callers slice the first rows of the B = 257 case."""
    dims, n_nets, out_act, ldx = EXACT_CASES[name]
    g = torch.Generator().manual_seed(1000 * seed + sorted(EXACT_CASES).index(name))
    nl = len(dims) - 1
    ld0 = (dims[0] + 31) // 32 * 32
    ldx = ld0 if ldx is None else ldx
    x = torch.full((B, ldx), 1e30)                                   # garbage in the ignored columns
    x[:, : dims[0]] = _ints(g, (B, dims[0]), -2, 2)
    W, b = [], []
    for n in range(n_nets):
        Wn, bn = [], []
        for l in range(nl):
            if l < nl - 1:
                w = _ints(g, (dims[l + 1], dims[l]), -2, 2) * (torch.rand((dims[l + 1], dims[l]), generator=g) < 0.25)
                bb = _ints(g, (dims[l + 1],), -3, 3)
                if l == 0 and nl - 1 == 3:
                    bb = bb + 4 * dims[0]
            else:
                bound = 1.0 / math.sqrt(dims[l])
                w = (torch.rand((dims[l + 1], dims[l]), generator=g) * 2 - 1) * bound
                bb = (torch.rand((dims[l + 1],), generator=g) * 2 - 1) * bound
            Wn.append(w); bn.append(bb)
        W.append(Wn); b.append(bn)
    draw = torch.randn((B, dims[-1]), generator=g) if out_act == ACT_TANH_NOISE else None
    if out_act != ACT_NONE:   # the policy: |z_L| <= 3 on the model, so that tanh is not saturated
        zmax = float(forward(dims, W, b, x, ACT_NONE)["z"].abs().max())
        if zmax > 3.0:
            W[0][-1] = W[0][-1] * (3.0 / zmax * 0.999)
            b[0][-1] = b[0][-1] * (3.0 / zmax * 0.999)
    return dict(dims=dims, n_nets=n_nets, out_act=out_act, ldx=ldx, W=W, b=b, x=x, draw=draw,
                model=forward(dims, W, b, x, out_act, draw))


@functools.lru_cache(maxsize=None)
def real_case(name, scale, B=256, seed=7):
    """Realistic data: nn.Linear default init times `scale`, inputs clamp(N(0,1), +-5)."""
    dims, n_nets, out_act = REAL_CASES[name]
    g = torch.Generator().manual_seed(100 * seed + 10 * sorted(REAL_CASES).index(name) + int(scale))
    W, b = [], []
    for n in range(n_nets):
        Wn, bn = [], []
        for l in range(len(dims) - 1):
            bound = 1.0 / math.sqrt(dims[l])
            Wn.append((torch.rand((dims[l + 1], dims[l]), generator=g) * 2 - 1) * bound * scale)
            bn.append((torch.rand((dims[l + 1],), generator=g) * 2 - 1) * bound * scale)
        W.append(Wn); b.append(bn)
    ld0 = (dims[0] + 31) // 32 * 32
    x = torch.zeros((B, ld0))
    x[:, : dims[0]] = torch.randn((B, dims[0]), generator=g).clamp(-5, 5)
    o64 = forward(dims, W, b, x, out_act)["out"]
    return dict(dims=dims, n_nets=n_nets, out_act=out_act, W=W, b=b, x=x, o64=o64, fp32=forward_fp32(dims, W, b, x, out_act))


def rms(t):
    return float(t.double().pow(2).mean().sqrt())


def unpack(packed, dims, n_nets):
    """Inverse of pqlk_mlp_pack_bf16's fragment order: int16 tensor -> [net][l] (N, K) int16 bit patterns (pads checked zero)."""
    out, o = [], 0
    for n in range(n_nets):
        layers = []
        for l in range(len(dims) - 1):
            K, N = dims[l], dims[l + 1]
            Kp, Np = (K + 15) // 16 * 16, (N + 31) // 32 * 32
            blk = packed[o: o + Np * Kp].view(Np // 32, Kp // 16, 2, 32, 8)   # [tile][k/16][h][r][j]
            full = blk.permute(0, 3, 1, 2, 4).reshape(Np, Kp)                   # row 32 tile + r, column 16 ks + 8 h + j
            assert not full[N:].any() and not full[:, K:].any(), "pad rows / columns of the packed copy must be zero"
            layers.append(full[:N, :K])
            o += Np * Kp
        out.append(layers)
    assert o == packed.numel()
    return out
