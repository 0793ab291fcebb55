"""Cases, inputs, mirror, references and checks for tests/test_dpg_fused_paths_gpu.py (plain numpy, no GPU, no library): the
P-learner's default step, pqlk_mlp_forward_qc -> pqlk_dpg_backward_fused -> pqlk_mlp_backward_tail.  Built on
tests/backward_cases.py (imported as bc); tests/test_dpg_fused_cases_cpu.py holds the mirror against the library's host-only calls
and the table against the conditions the checks rest on.

What runs.  k_dpg_minnet_head (minnet.h) reads the compact Q block qc (2, B), leaves 32 loss partials, the stable partition of the
batch by the net that attains min(Q1, Q2) -- perm, tie0, mn in the critic's workspace -- and the compact dZ of the critic's last
hidden layer, g w ELU'(H) with g = -1.0f / (float)B, 0.5 g on an exact tie.  The compact dX GEMMs walk down to the first hidden
layer; k_dx_slice<D, QPW> (narrow.h) forms columns [col0, col0 + A) of the input gradient through tanh', writes dz_a, and runs the
actor's head backward: dL/dZ of the actor's last hidden layer and one head partial (dW, db) per 32-row compact tile.
pqlk_mlp_backward_tail runs the actor's lower layers and k_reduce_slabs folds the partials of the tiles in use.

The data.  As in backward_cases: stash values from HVALS, weights in {-1, 0, 1}, tanh outputs from TVALS, integer qc built from
owner_input, integer observations.  Every weight matrix is thinned (one entry in `thin` is kept): the sums stay short enough for
the conditions below at batches up to 131072.  Rows repeat with period PERIOD = 4096 (the owners do not), so that the reference of
the largest case costs what a 4096-row case costs.

Power-of-two B.  g = -2^-k is exact, every value of the chain is a dyadic rational, and `exactness_bits` -- the worst
log2(sum_i |t_i| 2^g) over every output element of every product, measured on the chain with |g| = 1, i.e. with the 2^-k scale
folded in: the condition does not see a power-of-two scale -- is at most 24: every partial sum in any order is exact in fp32 and
every check is `==`.

Any other B.  perm, tie0, mn and the loss partials are integers or sums of integers: `==`.  g is the fp32 quotient the library
forms (the reference takes that rounded value as its input), and the float outputs are held to the float64 reference within a
bound derived here, not measured.  With u = 2^-24, a computed sum s = sum_i a_i w_i of n terms, taken in any order or grouping
(MFMA chain, sequential dot product, shuffle tree, fold of partials), whose inputs a_i carry absolute errors <= E(a_i) and whose
w_i are exact, satisfies
    |s - s*| <= sum_i |w_i| E(a_i) + (n + SPARE) u sum_i |a_i w_i|:
each product and each of at most n - 1 additions of non-zero operands rounds once (standard forward bound, gamma_n ~ n u; adding
an exact zero -- a pad row, a thinned weight -- rounds nothing); SPARE = 8 further roundings cover the second-order terms (n u / 2
of the first-order bound, at most 2^-12 for n <= 8193, the longest ragged sum of the table; 8 / n is at least 2^-11 there) and
the extra addition of a tie's second share.  The factors
ELU'(h) = 1, 0.5, 0.25, 0 scale value and error alike and round nothing; tanh' = 1 - a^2 in {1, 0.75, 0} is exact and its product
rounds once: E <- tanh' E + u |s tanh'|.  The stages compound in the order the kernels run them: the head's dZ (exact: g or 0.5 g
times +-1 times a power of two), each compact dX product (n = the layer's output width), the slice (n = dims[1]) and the tie's
second share, tanh', the actor head's dX (n = A), dW and db (n = B), and the same down the actor's lower layers.  `reference`
returns these E next to the values.
A dropped or doubled term must not hide under the bound: all terms of an output element are multiples of |g| 2^-G, G the
granularity of the product's terms on the |g| = 1 chain, so the smallest non-zero |t_i| is at least |g| 2^-G and the condition
asserted on the CPU is E < 0.5 |g| 2^-G (times the exact elementwise factor) for every checked element of dz_a and of the last
hidden dL/dZ: the row-local outputs.  The actor's dW / db sum B terms and meet that only at tiny B; where they do not
(`sharp["grads"]` false) the arena is still held to its bound, and the table holds the same pair, action width, column and owner
pattern at the neighbouring power of two, where the row sums are exact.

Source lines cited are those of pql_amd/csrc at the commit that added this file."""
import functools
from collections import namedtuple
from types import SimpleNamespace

import numpy as np

import backward_cases as bc
import detdata as dd

F32, F64 = np.float32, np.float64
POISON = bc.POISON
U, SPARE = 2.0 ** -24, 8
PERIOD = 4096
LOSS_PARTS = 32                           # minnet.h:159 (DPG_LOSS_PARTS)
MAX_B = 131072                            # gemm.hip, dpg_fused_ok: 1024 threads x 128 samples
E_UNSUPPORTED, E_WORKSPACE = 5, 6         # include/pqlk.h


# ---------------------------------------------------------------- mirror: eligibility (gemm.hip, narrow.h)
def fused_with_head(dims):
    """gemm.hip, fused_with_head (PQLK_NO_FUSED_HEAD unset): fusable (bc.buf_ld != 0) and head_fusable."""
    return bc.buf_ld(dims) != 0 and bc.head_fusable(dims)


def compact_chain_ok(dims, nets):
    """gemm.hip, compact_chain_ok."""
    return bc.minnet_ok(dims, nets, 0)


def dx_slice_head_ok(n_out, k_h):
    """narrow.h:467."""
    return 1 <= n_out <= 16 and k_h in (128, 256)


def dpg_fused_ok(cdims, cnets, adims, anets, B):
    """gemm.hip, dpg_fused_ok."""
    if B <= 0 or B > MAX_B:
        return False
    La, A = len(adims) - 1, adims[-1]
    if not compact_chain_ok(cdims, cnets) or anets != 1 or La < 2 or not fused_with_head(cdims):
        return False
    return (A <= 16 and cdims[0] >= A and bc.head_is_fused(adims) and dx_slice_head_ok(A, bc.ld(adims[La - 1]))
            and adims[La - 1] % 32 == 0)


# ---------------------------------------------------------------- mirror: workspace and launch geometry
def compact_ws(max_hidden_ld, B):
    """gemm.hip, compact_ws: float offsets of dz[0], dz[1], perm, mn, tie0 and the total."""
    cap = 2 * bc.round_up(B, bc.MN_TILE)
    dz1 = cap * max_hidden_ld
    perm = 2 * dz1
    mn = perm + cap
    return dict(rows_cap=cap, dz0=0, dz1=dz1, perm=perm, mn=mn, tie0=mn + 64, total=mn + 64 + cap)


def mn_offset(cdims, B):
    """gemm.hip, pqlk_dpg_fused_mn_offset."""
    return compact_ws(bc.max_hidden_ld(cdims), B)["mn"]


def head_parts(B):
    """gemm.hip, pqlk_dpg_fused_head_parts: one head partial per 32-row tile of the compact layout."""
    return compact_ws(0, B)["rows_cap"] // 32 if B > 0 else 0


def slice_instance(cdims, adims):
    """narrow.h:484-495 (launch_dx_slice with the actor head): (D, QPW) of k_dx_slice<D, QPW>."""
    K8 = cdims[1] // 32
    return (16 if K8 % 16 == 0 else 4), (16 if bc.ld(adims[-2]) == 256 else 8)


def head_launch(B):
    """gemm.hip, pqlk_dpg_backward_fused step 1: (blocks, rows_cap_blk) of k_dpg_minnet_head."""
    cap = compact_ws(0, B)["rows_cap"]
    blocks = max(1, min(cap // 16, 256))
    return blocks, bc.cdiv(cap, blocks)


def samples_per_thread(B):
    """minnet.h:186: S, a multiple of 8."""
    return ((B + 1023) // 1024 + 7) // 8 * 8


def qc_words(B):
    """minnet.h:191-209: the kinds of 8-sample words the head kernel reads: "vec" (two 16-byte loads per net), "scalar"."""
    # every word that starts below B belongs to some thread: a thread's first sample t S is a multiple of 8
    return {"vec" if B % 4 == 0 and m0 + 8 <= B else "scalar" for m0 in range(0, B, 8)}


def staging(col0):
    """narrow.h:270: 16-byte weight staging when the slice starts on a 16-byte boundary, else one float at a time."""
    return "vec" if col0 % 4 == 0 else "scalar"


# ---------------------------------------------------------------- the partition law (minnet.h:7-11, :157-158)
def partition(own):
    """own (B,) bytes (bit 0: net 0, bit 1: net 1) -> (perm, tie0, mn) over the `used` compact rows.  Stable; run 1 starts at c0
    rounded up to 128; mn = {c0, c1, base1, used}; perm is -1 on pad rows; tie0 is -1 on ordinary rows, -2 on a tie's run-0 row and
    the run-0 index on a tie's run-1 row."""
    own = np.asarray(own)
    i0, i1 = np.flatnonzero(own & 1), np.flatnonzero(own & 2)
    c0, c1 = len(i0), len(i1)
    base1 = bc.round_up(c0, bc.MN_TILE)
    used = base1 + bc.round_up(c1, bc.MN_TILE)
    perm, tie0 = np.full(used, -1, dtype=np.int32), np.full(used, -1, dtype=np.int32)
    perm[:c0], perm[base1: base1 + c1] = i0, i1
    pos0 = np.full(len(own), -1, dtype=np.int32)
    pos0[i0] = np.arange(c0)
    tie0[:c0][own[i0] == 3] = -2
    t1 = own[i1] == 3
    tie0[base1: base1 + c1][t1] = pos0[i1[t1]]
    return perm, tie0, np.array([c0, c1, base1, used], dtype=np.int32)


def loss_parts(q, B):
    """float64: 32 sums of min(Q1, Q2) over runs of 32 S consecutive samples (minnet.h:218-222)."""
    run = 32 * samples_per_thread(B)
    mq = np.minimum(q[0], q[1]).astype(F64)
    return np.array([mq[i * run: (i + 1) * run].sum() for i in range(LOSS_PARTS)])


# ---------------------------------------------------------------- the table
# thin: one weight in `thin` is kept; data: "std" (HVALS, TVALS) | "int" (integer stash, tanh outputs in {0, +-1})
FCase = namedtuple("FCase", "name cdims adims B col0 owner splits thin data")
OWNERS = bc.OWNERS + ("halves", "alternate")      # first half net 0, second half net 1 | even rows net 0, odd rows net 1


def pair(p, A):
    """The four (critic, actor) pairs, O = 8: the (D, QPW) instances <4, 8>, <4, 16>, <16, 8> (the head's row loop with 8 live
    lanes), <16, 16> (two compact dX products; kq = 72: two trips of the head's lane loop)."""
    return {1: ([8 + A, 128, 128, 1], [8, 128, A]), 2: ([8 + A, 128, 128, 1], [8, 64, 256, A]),
            3: ([8 + A, 512, 32, 1], [8, 128, A]), 4: ([8 + A, 512, 128, 288, 1], [8, 256, A])}[p]


_TABLE = [
    # pair, A, col0, B, owner, thin, data
    (1, 16, 8, 1, "mixed", 4, "std"),               # a lone row
    (1, 5, 7, 3, "ties", 4, "std"),                 # B < 128, B % 4 != 0, every row a tie: used == rows_cap
    (1, 5, 7, 4, "ties", 4, "std"),
    (3, 1, 7, 12, "mixed", 8, "std"),               # B % 8 != 0, B % 4 == 0: one vector word and one scalar word
    (3, 1, 7, 16, "mixed", 8, "std"),
    (2, 16, 8, 32, "net1", 4, "std"),               # run 0 empty
    (1, 5, 7, 127, "mixed", 4, "std"),
    (1, 5, 7, 128, "mixed", 4, "std"),
    (1, 16, 8, 128, "ties", 4, "std"),              # both runs full at B = 128
    (2, 1, 8, 129, "ties", 4, "std"),               # c0 = 129; both runs full
    (2, 1, 8, 128, "ties", 4, "std"),
    (1, 16, 7, 256, "halves", 4, "std"),            # c0 exactly 128, no tie
    (1, 16, 7, 256, "alternate", 4, "std"),         # ... and interleaved alongside
    (3, 5, 8, 256, "net0", 8, "std"),               # run 1 empty: c1 = 0, used = base1
    (4, 16, 8, 257, "mixed", 32, "std"),
    (4, 16, 8, 256, "mixed", 32, "std"),
    (4, 5, 7, 256, "mixed", 32, "std"),
    (3, 16, 8, 2048, "mixed", 16, "std"),           # the head launch's grid cap: 256 blocks of 16 rows | of 17
    (3, 16, 8, 2049, "mixed", 16, "std"),
    (1, 5, 8, 8192, "mixed", 8, "std"),             # S = 8 | 16
    (1, 5, 8, 8193, "mixed", 8, "std"),
    (2, 16, 7, 16384, "mixed", 32, "std"),
    (1, 1, 8, 131072, "mixed", 16, "std"),          # the limit: 128 samples per thread
    (1, 5, 8, 8, "alternate", 4, "int"),            # integer stash, tanh' in {0, 1}, no tie: gradients with exact squares
]


def _fname(p, A, col0, B, owner, data):
    return f"p{p}-A{A}-c{col0}-B{B}-{owner}" + ("" if data == "std" else f"-{data}")


CASES = [FCase(_fname(p, A, col0, B, owner, data), pair(p, A)[0], pair(p, A)[1], B, col0, owner, bc.default_splits(B), thin, data)
         for p, A, col0, B, owner, thin, data in _TABLE]
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
NAMES = [c.name for c in CASES]
NORM_NAME = "p1-A5-c8-B8-alternate-int"
INSTANCES = [(4, 8), (4, 16), (16, 8), (16, 16)]
# each threshold of the path: (what, predicate of B, the smallest batch that satisfies it); the CPU test proves them minimal
THRESHOLDS = [("S = 16", lambda B: samples_per_thread(B) > 8, 8193),
              ("head grid cap", lambda B: head_launch(B) != (compact_ws(0, B)["rows_cap"] // 16, 16), 2049),
              ("refused", lambda B: not dpg_fused_ok(pair(1, 1)[0], 2, pair(1, 1)[1], 1, B), MAX_B + 1),
              ("a second tile per run", lambda B: compact_ws(0, B)["rows_cap"] > 256, 129)]


def instance(c):
    return slice_instance(c.cdims, c.adims)


# ---------------------------------------------------------------- inputs
def _rows(c):
    return PERIOD if c.B % PERIOD == 0 else c.B


def _ccase(c, B=None):
    return bc.Case(c.name + "/critic", list(c.cdims), 2, _rows(c) if B is None else B, 1, "slice", c.col0, c.adims[-1],
                   bc.ld(c.cdims[0]), ())


def _acase(c):
    return bc.Case(c.name + "/actor", list(c.adims), 1, _rows(c), c.splits, "g", 0, 0, 64, ())   # ldx = 64: the learner's obs tile


def _thinned(case, thin):
    """bc.weights with one entry in `thin` kept."""
    W = bc.weights(case)
    return [[(w * (dd.integers(w.shape, bc._seed(case, 31, n, l), thin) == 0)).astype(F32) for l, w in enumerate(net)]
            for n, net in enumerate(W)]


def _hidden(case, data):
    if data == "std":
        return bc.hidden(case)
    return [[bc.HINT[dd.integers((case.B, case.dims[l + 1]), bc._seed(case, 2, n, l), len(bc.HINT))] for l in range(len(case.dims) - 2)]
            for n in range(case.nets)]


def owners(c):
    """(own (B,) bytes, q (2, B) integer Q that says the same)."""
    if c.owner in bc.OWNERS:
        return bc.owner_input(_ccase(c, c.B), c.owner)
    m = np.arange(c.B)
    own = np.where(m < (c.B + 1) // 2, 1, 2).astype(np.uint8) if c.owner == "halves" else (1 + m % 2).astype(np.uint8)
    q = np.zeros((2, c.B), dtype=F32)
    q[0] = bc.rc.ints((c.B,), bc._seed(_ccase(c, c.B), 7), -3, 3)
    q[1] = q[0] + np.where(own == 1, 1, -1).astype(F32)
    return own, q


@functools.lru_cache(maxsize=4)
def problem(name):
    """One case: Wc / Hc (critic, [net][layer]), Wa / Ha (actor, [layer]), xa (rows, 64) observations, tanh (rows, A), own, q.
    The row-wise arrays hold `rows` rows (PERIOD where that divides B, else B); sample m reads row m % rows."""
    c = BY_NAME[name]
    cc, ac = _ccase(c), _acase(c)
    tanh = bc.tanh_input(cc)
    if c.data == "int":
        tanh = np.sign(tanh).astype(F32)                           # {0, +-1}: tanh' in {1, 0}
    own, q = owners(c)
    return make_problem(c, _thinned(cc, c.thin), _hidden(cc, c.data), _thinned(ac, c.thin)[0], _hidden(ac, c.data)[0],
                        bc.x_input(ac), tanh, own, q)


def make_problem(c, Wc, Hc, Wa, Ha, xa, tanh, own, q):
    p = SimpleNamespace(c=c, rows=len(xa), Wc=Wc, Hc=Hc, Wa=Wa, Ha=Ha, xa=xa, tanh=tanh, own=own, q=q,
                        g=F64(F32(-1.0) / F32(c.B)))
    assert c.B % p.rows == 0 or p.rows == c.B
    return p


def arena_of(dims, W):
    """The parameter arena of [net][layer] weights: zero pad columns, 1.0 in the biases (the backward reads none)."""
    ns = bc.net_stride(dims)
    out = np.zeros(ns * len(W), dtype=F32)
    for n, net in enumerate(W):
        for l, w in enumerate(net):
            wo, bo = bc.layer_offsets(dims, l)
            out[n * ns + wo: n * ns + bo].reshape(dims[l + 1], bc.ld(dims[l]))[:, : dims[l]] = w
            out[n * ns + bo: n * ns + bo + dims[l + 1]] = 1.0
    return out


def stash_of(dims, H, B):
    """The flat activation stash of [net][layer] hidden blocks tiled to B rows: zero pad columns, NaN in the output block."""
    nets = len(H)
    out = np.zeros(bc.acts_floats(dims, nets, B), dtype=F32)
    for n, net in enumerate(H):
        for l, h in enumerate(net):
            off, ldh = bc.act_offset(dims, nets, B, n, l)
            out[off: off + B * ldh].reshape(B, ldh)[:, : dims[l + 1]] = np.tile(h, (B // len(h), 1))
    off, _ = bc.act_offset(dims, nets, B, 0, len(dims) - 2)
    out[off:] = np.nan
    return out


def tiled(a, B):
    return np.tile(a, (B // len(a), 1))


def ld_tanh(c):
    return c.adims[-1] + 1                 # an odd row stride, one IN_ONE column behind the tanh outputs


# ---------------------------------------------------------------- the float64 reference
def _critic_unit(p):
    """Per net n, on the distinct rows and for g = 1 with the net as sole owner: (C (rows, A) the slice sum before tanh', its
    error bound E, [(name, mass, granularity)] per product, G the granularity of the slice's terms)."""
    c, out = p.c, []
    dims, L, A = c.cdims, len(c.cdims) - 1, c.adims[-1]
    for n in range(2):
        prods = []
        f = bc.elu_prime(p.Hc[n][L - 2])
        dz = p.Wc[n][L - 1][0].astype(F64)[None, :] * f             # exact: +-1 times a power of two
        E, g = np.zeros_like(dz), bc._gran(dz)
        prods.append((f"head net {n}", np.abs(dz), g))
        for l in range(L - 2, -1, -1):
            w = p.Wc[n][l].astype(F64)
            if l == 0:
                w = w[:, c.col0: c.col0 + A]
            mass = np.abs(dz) @ np.abs(w)
            prods.append((f"critic dX{l} net {n}", mass, g))
            E = E @ np.abs(w) + (dims[l + 1] + SPARE) * U * mass
            dz = dz @ w
            if l > 0:
                f = bc.elu_prime(p.Hc[n][l - 1])
                dz, E = dz * f, E * f
                g += bc._gran(f)
                prods.append((f"critic dX{l} * ELU' net {n}", np.abs(dz), g))
        out.append((dz, E, prods, g))
    return out


@functools.lru_cache(maxsize=4)
def _reference(name):
    return reference_of(problem(name))


def reference(name):
    """float64, read-only.  Values: "perm", "tie0", "mn" (the partition), "loss" (32,), "dz_a" (B, A), "dxh" (B, Kh: dL/dZ of the
    actor's last hidden layer), "grads" (the actor's arena).  "E": the absolute error bounds of dz_a, dxh and grads for a ragged
    B; "bits": exactness_bits of the |g| = 1 chain; "sharp": per output, whether E < half the smallest possible non-zero term
    everywhere."""
    return _reference(name)


def reference_of(p):
    c = p.c
    B, rows, A, adims = c.B, p.rows, c.adims[-1], c.adims
    La = len(adims) - 1
    idx = np.arange(B) % rows
    perm, tie0, mn = partition(p.own)
    (C0, E0, prods0, g0), (C1, E1, prods1, g1) = _critic_unit(p)
    a0 = np.where(p.own == 3, 0.5, (p.own & 1).astype(F64))[:, None]
    a1 = np.where(p.own == 3, 0.5, ((p.own >> 1) & 1).astype(F64))[:, None]
    tie = (p.own == 3)[:, None]
    S = a0 * C0[idx] + a1 * C1[idx]
    ES = a0 * E0[idx] + a1 * E1[idx] + np.where(tie, U * np.abs(S), 0.0)
    gS = max(g0, g1) + (1 if tie.any() else 0)
    t = p.tanh[idx].astype(F64)
    tp = 1.0 - t * t
    dz_a = S * tp
    E_a = ES * tp + U * np.abs(dz_a)
    prods = prods0 + prods1 + [("slice, both shares", a0 * np.abs(C0[idx]) + a1 * np.abs(C1[idx]), gS), ("tanh'", np.abs(dz_a), gS + 2)]
    g_a = bc._gran(dz_a)
    sharp = {"dz_a": bool(np.all(E_a[tp > 0] < (0.5 * 2.0 ** -gS * tp)[tp > 0]))}
    # ---- the actor: the head on every row, then folded over the period for the row sums
    Wh = p.Wa[La - 1].astype(F64)
    fh = bc.elu_prime(p.Ha[La - 2])[idx]
    mass_h = np.abs(dz_a) @ np.abs(Wh)
    dxh = (dz_a @ Wh) * fh
    E_h = (E_a @ np.abs(Wh) + (A + SPARE) * U * mass_h) * fh
    prods += [("actor head dX", mass_h, g_a), ("actor head dX * ELU'", np.abs(dxh), g_a + bc._gran(fh))]
    sharp["dxh"] = bool(np.all(E_h[fh > 0] < (0.5 * 2.0 ** -g_a * fh)[fh > 0]))
    folded = B > rows

    def fold(v):
        return v.reshape(B // rows, rows, -1).sum(0) if folded else v

    dz, adz, E, g = fold(dz_a), fold(np.abs(dz_a)), fold(E_a), g_a
    ns = bc.net_stride(adims)
    grads, E_g, sharp_g = np.zeros(ns), np.zeros(ns), True
    for l in range(La - 1, -1, -1):
        inp = (p.xa[:, : adims[0]] if l == 0 else p.Ha[l - 1]).astype(F64)
        gi = g + bc._gran(inp)
        mW, mb = adz.T @ np.abs(inp), adz.sum(0)
        EW, Eb = E.T @ np.abs(inp) + (B + SPARE) * U * mW, E.sum(0) + (B + SPARE) * U * mb
        prods += [(f"actor dW{l}", mW, gi), (f"actor db{l}", mb, g)]
        sharp_g = sharp_g and bool(np.all(EW[mW > 0] < 0.5 * 2.0 ** -gi)) and bool(np.all(Eb[mb > 0] < 0.5 * 2.0 ** -g))
        wo, bo = bc.layer_offsets(adims, l)
        for arr, vW, vb in ((grads, dz.T @ inp, dz.sum(0)), (E_g, EW, Eb)):
            arr[wo: bo].reshape(adims[l + 1], bc.ld(adims[l]))[:, : adims[l]] = vW
            arr[bo: bo + adims[l + 1]] = vb
        if l > 0:
            w, f = p.Wa[l].astype(F64), bc.elu_prime(p.Ha[l - 1])
            m = adz @ np.abs(w)
            if l < La - 1:
                prods.append((f"actor dX{l}", m, g))
            E = (E @ np.abs(w) + (adims[l + 1] + SPARE) * U * m) * f
            dz = (dz @ w) * f
            adz = m * f if folded else np.abs(dz)                    # folded: an upper bound of sum |.| over the period
            g += bc._gran(f)
    sharp["grads"] = sharp_g
    bits = 0.0
    for _, mass, gg in prods:
        if mass.size and mass.max() > 0:
            bits = max(bits, float(np.log2(mass.max() * 2.0 ** gg)))
    ag = abs(p.g)
    out = dict(perm=perm, tie0=tie0, mn=mn, loss=loss_parts(p.q, B), dz_a=dz_a * p.g, dxh=dxh * p.g, grads=grads * p.g,
               E=dict(dz_a=E_a * ag, dxh=E_h * ag, grads=E_g * ag), bits=bits, sharp=sharp, exact=bc.is_pow2(B))
    for v in list(out.values()) + list(out["E"].values()):
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def exactness_bits(name):
    return reference(name)["bits"]


# ---------------------------------------------------------------- checks (numpy in, AssertionError out)
def _held(got, want, E, exact, what):
    """`==` for an exact case, else |got - want| <= E elementwise.  Returns the worst err / bound (0 where all is equal)."""
    got = got.astype(F64)
    assert got.shape == want.shape, f"{what}: shape {got.shape} != {want.shape}"
    err = np.abs(got - want)
    assert not np.isnan(err).any(), f"{what}: NaN left"
    if exact:
        bad = np.argwhere(err != 0)
        assert bad.size == 0, f"{what}: {len(bad)} elements differ, first at {tuple(bad[0])}: {got[tuple(bad[0])]} != {want[tuple(bad[0])]}"
        return 0.0
    bad = np.argwhere(err > E)
    assert bad.size == 0, (f"{what}: {len(bad)} elements leave the bound, first at {tuple(bad[0])}: {got[tuple(bad[0])]} vs "
                           f"{want[tuple(bad[0])]} +- {E[tuple(bad[0])]}")
    return float((err[E > 0] / E[E > 0]).max()) if (E > 0).any() else 0.0


def check_partition(perm, tie0, mn, ref, what=""):
    """perm, tie0: the first rows_cap ints of the workspace blocks; mn: 4 ints."""
    used = int(ref["mn"][3])
    assert np.array_equal(mn, ref["mn"]), f"{what}: mn {mn.tolist()} != {ref['mn'].tolist()}"
    for got, want, nm in ((perm, ref["perm"], "perm"), (tie0, ref["tie0"], "tie0")):
        bad = np.flatnonzero(got[:used] != want)
        assert bad.size == 0, f"{what}: {nm} differs at compact row {int(bad[0])}: {got[bad[0]]} != {want[bad[0]]}"


def check_loss(loss, ref, what=""):
    """loss: the 64 floats of loss_part, NaN before the call."""
    bad = np.flatnonzero(~(loss[:LOSS_PARTS].astype(F64) == ref["loss"]))
    assert bad.size == 0, f"{what}: loss partial {int(bad[0])} is {loss[bad[0]]}, not {ref['loss'][bad[0]]}"
    assert np.isnan(loss[LOSS_PARTS:]).all(), f"{what}: loss_part written behind its {LOSS_PARTS} partials"


def check_floats(dz_a, dxh, grads, ref, what=""):
    """dz_a (B, ld_dz) as left (POISON before the call), dxh (B, Kh), grads (arena).  Returns the worst err / bound."""
    A = ref["dz_a"].shape[1]
    ex = ref["exact"]
    r = _held(dz_a[:, :A], ref["dz_a"], ref["E"]["dz_a"], ex, f"{what} dz_a")
    assert np.all(dz_a[:, A:].view(np.uint32) == np.array(POISON, dtype=F32).view(np.uint32)), f"{what}: pad columns of dz_a written"
    r = max(r, _held(dxh, ref["dxh"], ref["E"]["dxh"], ex, f"{what} dL/dZ of the actor's last hidden layer"))
    if grads is not None:
        r = max(r, _held(grads, ref["grads"], ref["E"]["grads"], ex, f"{what} actor arena"))
    return r


# ---------------------------------------------------------------- a plain numpy backward, for the checks' own tests
FAULTS = ("tie_twice", "tie_no_net0", "run1_net0_weights", "fold_one_more", "fold_one_less", "db_row", "tanh_row")


def model_backward(name, fault=None):
    """What the three launches leave -- dict(perm, tie0, mn, loss, dz_a, dxh, grads) -- computed by plain numpy the way the
    kernels split the work (compact rows, 32-row tiles, one head partial per tile, the partials of the tiles in use folded), with
    one fault planted:
      tie_twice          a tie's run-0 row is not skipped: its tile writes the row and counts it in its partial as well
      tie_no_net0        a tie's run-1 row lacks net 0's share
      run1_net0_weights  the tiles of run 1 take net 0's weights
      fold_one_more      one head partial too many is folded (the one behind the tiles in use: POISON)
      fold_one_less      the last tile's partial is not folded
      db_row             db sums 31 rows of each tile
      tanh_row           tanh' is read at the compact row's index, not at the batch row's"""
    p = problem(name)
    c = p.c
    B, A, adims = c.B, c.adims[-1], c.adims
    assert B == p.rows
    La, Kh = len(adims) - 1, adims[-2]
    perm, tie0, mn = partition(p.own)
    (C0, _, _, _), (C1, _, _, _) = _critic_unit(p)
    t = p.tanh.astype(F64)
    tp = 1.0 - t * t
    Hh, fh, Wh = p.Ha[La - 2].astype(F64), bc.elu_prime(p.Ha[La - 2]), p.Wa[La - 1].astype(F64)
    hf = A * bc.ld(Kh) + 32
    parts = np.full((head_parts(B), hf), F64(POISON))
    dz_a, dxh = np.full((B, bc.ld(A)), F64(POISON)), np.zeros((B, Kh))
    used, base1 = int(mn[3]), int(mn[2])
    for tile in range(used // 32):
        dzt = np.zeros((32, A))
        rows_m = np.full(32, -1)
        for r in range(32):
            i = 32 * tile + r
            m = int(perm[i])
            if m < 0 or (tie0[i] == -2 and fault != "tie_twice"):
                continue
            share = 0.5 if p.own[m] == 3 else 1.0
            run1 = i >= base1
            s = share * ((C1 if run1 and fault != "run1_net0_weights" else C0)[m])
            if tie0[i] >= 0 and fault != "tie_no_net0":
                s = s + 0.5 * C0[m]
            dzt[r] = s * tp[min(i, B - 1) if fault == "tanh_row" else m] * p.g
            rows_m[r] = m
        live = rows_m >= 0
        dz_a[rows_m[live], :A] = dzt[live]
        dxh[rows_m[live]] = (dzt[live] @ Wh) * fh[rows_m[live]]
        part = np.zeros(hf)
        part[: A * bc.ld(Kh)].reshape(A, bc.ld(Kh))[:, :Kh] = dzt[live].T @ Hh[rows_m[live]]
        part[A * bc.ld(Kh): A * bc.ld(Kh) + A] = dzt[:31].sum(0) if fault == "db_row" else dzt.sum(0)
        parts[tile] = part
    n_fold = used // 32 + {"fold_one_more": 1, "fold_one_less": -1}.get(fault, 0)
    head = parts[: min(n_fold, len(parts))].sum(0)
    grads = np.zeros(bc.net_stride(adims))
    wo, _ = bc.layer_offsets(adims, La - 1)
    grads[wo: wo + hf] = head
    dz = dxh
    for l in range(La - 2, -1, -1):
        inp = (p.xa[:, : adims[0]] if l == 0 else p.Ha[l - 1]).astype(F64)
        wo, bo = bc.layer_offsets(adims, l)
        grads[wo: bo].reshape(adims[l + 1], bc.ld(adims[l]))[:, : adims[l]] = dz.T @ inp
        grads[bo: bo + adims[l + 1]] = dz.sum(0)
        if l > 0:
            dz = (dz @ p.Wa[l].astype(F64)) * bc.elu_prime(p.Ha[l - 1])
    return dict(perm=perm, tie0=tie0, mn=mn, loss=np.concatenate([loss_parts(p.q, B), np.full(32, np.nan)]).astype(F32),
                dz_a=dz_a.astype(F32), dxh=dxh.astype(F32), grads=grads.astype(F32))


def check_all(out, ref, what=""):
    check_partition(out["perm"], out["tie0"], out["mn"], ref, what)
    check_loss(out["loss"], ref, what)
    return check_floats(out["dz_a"], out["dxh"], out["grads"], ref, what)


# ---------------------------------------------------------------- pqlk_mlp_forward_qc on the exactly evaluable network
QC_DIMS, QC_O, QC_A = [24, 128, 128, 1], 8, 16
QC_BATCHES = (1, 33, 257)
CHAIN_B = 256


def qc_problem(B, twin):
    """bc.exact_network on [24, 128, 128, 1] whose input is [obs (8 integer columns, the gate in column 0) | 16 tanh outputs from
    TVALS]: every hidden pre-activation is a half-integer >= 0 or <= -32 (the bounds of exact_network hold for inputs in [-2, 2]).
    Returns (case, W, bias, x (B, 32), H, q)."""
    case = bc.Case(f"qc-B{B}-{'twin' if twin else 'two'}", list(QC_DIMS), 2, B, 1, "slice", QC_O, QC_A, 32, ())
    W, bias, x = bc.exact_network(case, twin=twin)
    x = np.array(x)
    x[:, QC_O: QC_O + QC_A] = bc.tanh_input(case)
    _, H, q = bc.exact_forward(case, W, bias, x)
    return case, W, bias, x, H, q


def qc_arena(case, W, bias):
    out = arena_of(case.dims, W)
    ns = bc.net_stride(case.dims)
    for n in range(2):
        for l in range(len(case.dims) - 1):
            _, bo = bc.layer_offsets(case.dims, l)
            out[n * ns + bo: n * ns + bo + bc.ld(case.dims[l + 1])] = 0
            out[n * ns + bo: n * ns + bo + case.dims[l + 1]] = bias[n][l]
    return out


def qc_stash(case, H, q):
    """What the forward must leave: hidden blocks with zero pads, Q in column 0 of the output block and zeros beside it."""
    out = stash_of(case.dims, H, case.B)
    off, ldo = bc.act_offset(case.dims, 2, case.B, 0, len(case.dims) - 2)
    blk = out[off:].reshape(2, case.B, ldo)
    blk[:] = 0
    blk[:, :, 0] = q
    return out


CHAIN = FCase("chain-B256", list(QC_DIMS), [8, 128, QC_A], CHAIN_B, QC_O, "from the forward", 1, 4, "std")


@functools.lru_cache(maxsize=1)
def chain_problem():
    """The chained case: the critic is the exact network (its stash and qc come out of the real forward), the owners follow its
    integer Q (ties included), the actor is pair 1's with the network's tanh block as its output.  Returns (problem, qc parts)."""
    case, W, bias, x, H, q = qc_problem(CHAIN_B, False)
    ac = _acase(CHAIN)
    own = ((q[0] <= q[1]).astype(np.uint8) | ((q[1] <= q[0]).astype(np.uint8) << 1))
    p = make_problem(CHAIN, W, H, _thinned(ac, CHAIN.thin)[0], bc.hidden(ac)[0], bc.x_input(ac), x[:, QC_O: QC_O + QC_A].copy(), own,
                     q.astype(F32))
    return p, (case, W, bias, x, H, q)
