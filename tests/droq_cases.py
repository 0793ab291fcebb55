"""The mask law of the dropout LayerNorm entries (include/pqlk.h, `pqlk_drop_*`) as a numpy model, the dropped inputs, the float64
references and the shape table of tests/test_droq_kernels_gpu.py (plain numpy / torch, no GPU); tests/test_droq_cpu.py proves what
they guarantee.  Inputs, bars and the reference function are those of tests/layernorm_cases.py, applied to u = keep ? z * s : 0."""
import functools

import numpy as np

import layernorm_cases as lc

F32, U32, U64 = np.float32, np.uint32, np.uint64
M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK32 = 0xFFFFFFFF


def philox4x32_10(key, ctr):
    """Philox4x32-10 (Salmon et al. 2011).  key: 2 words, ctr: 4 words, each a python int or an integer array (broadcast together).
    Returns the block's four uint32 words as arrays of the broadcast shape."""
    k0, k1 = (np.asarray(k, U64) & U64(MASK32) for k in key)
    c0, c1, c2, c3 = np.broadcast_arrays(*(np.asarray(c, U64) & U64(MASK32) for c in ctr))
    for _ in range(10):
        p0, p1 = U64(M0) * c0, U64(M1) * c2          # 32 x 32 -> 64 bits: no overflow in uint64
        hi0, lo0, hi1, lo1 = p0 >> U64(32), p0 & U64(MASK32), p1 >> U64(32), p1 & U64(MASK32)
        c0, c1, c2, c3 = hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0
        k0, k1 = (k0 + U64(W0)) & U64(MASK32), (k1 + U64(W1)) & U64(MASK32)
    return tuple(c.astype(U32) for c in (c0, c1, c2, c3))


def threshold(p):
    """thr = (uint32_t) floor((double)p * 2^32) of the fp32 value of p."""
    return int(np.floor(float(F32(p)) * 4294967296.0))


def scale(p):
    """s = 1.0f / (1.0f - p), one fp32 rounding each."""
    return F32(1.0) / (F32(1.0) - F32(p))


def mask_words(seed, tag, m, cols):
    """x(r, c): component c & 3 of the block with key (seed lo, seed hi) and counter (c >> 2, r, tag lo, tag hi), (m, cols) uint32."""
    nb = (cols + 3) // 4
    r, b = np.arange(m, dtype=U64)[:, None], np.arange(nb, dtype=U64)[None, :]
    words = philox4x32_10((seed & MASK32, seed >> 32), (b, r, tag & MASK32, tag >> 32))
    return np.stack(words, axis=-1).reshape(m, nb * 4)[:, :cols]


def keep_mask(seed, tag, p, m, cols):
    """keep(r, c) = x(r, c) >= thr, (m, cols) bool."""
    return mask_words(seed, tag, m, cols) >= U32(threshold(p))


def dropped(z, seed, tag, p):
    """u = keep ? z * s : 0.0f in fp32 (one rounding), and the mask."""
    keep = keep_mask(seed, tag, p, *z.shape)
    return np.where(keep, (np.asarray(z, F32) * scale(p)).astype(F32), F32(0.0)).astype(F32), keep


def make_tag(call, stream, net, layer):
    """The model's tag layout (pql_amd/models/droq.py)."""
    return (call << 8) | (stream << 5) | (net << 4) | layer


SEED = 0x9E3779B97F4A7C15                      # both key words in play
TAGS = [make_tag(0, 0, 0, 0), (0xA5 << 32) | make_tag(70001, 1, 1, 2)]   # the second: the tag's high word in play too
P = [0.0, 0.01, 0.5]

COLS = [1, 3, 33, 64, 65, 128, 129, 130, 257, 513, 1025]
M_SMALL = [1, 5, 257]
# past each grid cap a wave takes a second row: the mask must follow the ROW index, not the trip or the block
SHAPES = [(m, c) for c in COLS for m in M_SMALL] + [(lc.M_PAST_ROW_BLOCKS, 33), (lc.M_PAST_CHUNKS, 130)]
MASK_SHAPES = SHAPES + [(m, 2) for m in M_SMALL]      # cols = 2: mask and p = 0 tests only (see layernorm_cases.generic_inputs)

# The float64 comparison.  Forward: every shape.  Backward: cols >= 2 as in tests/test_layernorm_kernels_gpu.py (at cols = 1 dz and
# dgamma are exactly 0 and the float64 reference is ~1e-17: an equality, which the GPU test asserts, not a bar).  Taken out of the
# backward comparison, because torch's own fp32 CPU autograd misses the bar there, 431-fold (tests/test_droq_cpu.py holds that this
# shape, and only this one, does): (1, 3) at p = 0.5.  Its one row keeps ONE of three columns, u = (a, 0, 0): xhat is
# (+-sqrt 2, -+1 / sqrt 2, -+1 / sqrt 2) whatever a is, and dz is eps / (var + eps) of the terms it is the difference of -- the
# cols = 2 degeneracy that layernorm_cases.generic_inputs describes -- with no well-conditioned row to set the bar's scale.
BWD_EXCLUDED = {(1, 3, 0.5)}


def fwd_cases():
    return [(s, p) for s in SHAPES for p in P[1:]]


def bwd_cases():
    return [(s, p) for s in SHAPES for p in P[1:] if s[1] >= 2 and (s[0], s[1], p) not in BWD_EXCLUDED]


def case_id(c):
    (m, cols), p = c
    return f"m{m}-c{cols}-p{p}"


@functools.lru_cache(maxsize=None)
def drop_case(m, cols, p, tag=TAGS[1], seed=SEED):
    """(z, gamma, beta, dy), keep, u, float64 reference on u with dz masked and scaled: computed once, shared, never written to."""
    inp = lc.generic_inputs(m, cols)
    z, gamma, beta, dy = inp
    u, keep = dropped(z, seed, tag, p)
    ref = dict(lc.torch_reference(u, gamma, beta, dy))
    ref["dz"] = np.where(keep, ref["dz"] * np.float64(scale(p)), 0.0)
    for a in (*inp, keep, u, *ref.values()):
        a.setflags(write=False)
    return inp, keep, u, ref
