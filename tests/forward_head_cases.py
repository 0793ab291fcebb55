"""Cases, inputs, references and checks for tests/test_forward_heads_gpu.py (plain numpy, no GPU, no library).

pqlk_mlp_forward ends in one of five output-layer implementations, each with its own copy of the epilogue (bias, NONE / TANH /
TANH_NOISE with its two clamps, zero pad columns, second destination out2).  `head_path` restates the library's dispatch so that
every case can name the kernel it reaches; tests/test_forward_head_cases_cpu.py holds the table against it, and holds `fusable`
against the one predicate the library exposes (pqlk_mlp_packed_floats).  The checks themselves are numpy functions of the
kernel's output, so that the CPU tests can show them failing on a wrong epilogue.

Source lines cited below are those of pql_amd/csrc at the commit that added this file."""
from collections import namedtuple

import numpy as np

import detdata as dd
import reduction_cases as rc

F32 = np.float32
POISON, SLACK = rc.POISON, rc.SLACK
ACT_NONE, ACT_TANH, ACT_TANH_NOISE = 0, 1, 2
ACTS = (ACT_NONE, ACT_TANH, ACT_TANH_NOISE)
NOISE_STD, NOISE_CLIP = 0.8, 0.2

# ---------------------------------------------------------------- the library's constants
LDS_BYTES = 160 * 1024          # gemm.hip, fusable and fused_rows
FUSED_NW = 8                    # fused.h:70, waves per block of the fused forward
SKINNY_MAX_K = 1024             # skinny.h:10


def ld(cols):
    """pqlk_ld (replay.hip:7): round up to 32 floats."""
    return (max(int(cols), 1) + 31) // 32 * 32


# ---------------------------------------------------------------- mirror of the forward's dispatch
def fused_lds_bytes(dims, buf_ld, R):
    """gemm.hip, fused_lds_bytes."""
    acts = (32 * R * buf_ld + (len(dims) - 2) * (buf_ld - 4)) * 4
    head = 8 * R * 16 * 64 * 4
    return max(acts, head)


def fusable(dims):
    """gemm.hip, fusable: the LDS row stride buf_ld of the fused hidden stack, or 0 when it cannot run."""
    L = len(dims) - 1
    if L < 2:
        return 0
    w = ld(dims[0])
    for l in range(1, L):
        if dims[l] % 32 != 0 or dims[l] > 1024:
            return 0
        w = max(w, dims[l])
    buf_ld = w + 4
    return buf_ld if fused_lds_bytes(dims, buf_ld, 1) <= LDS_BYTES else 0


def head_fusable(dims):
    """gemm.hip, head_fusable."""
    return len(dims) - 1 >= 2 and dims[-1] <= 32 and dims[-2] % 32 == 0


def fused_wide(dims):
    """gemm.hip, launch_fused_hidden (`wide`): a hidden layer wider than 512 selects k_mlp_fwd_fused<1, 4>."""
    return any(d > 512 for d in dims[1:-1])


def fused_rows(dims, nets, buf_ld, B):
    """gemm.hip, fused_rows without the PQLK_FUSED_ROWS override: 32-row tiles per block."""
    R = 1
    if not fused_wide(dims) and fused_lds_bytes(dims, buf_ld, 2) <= LDS_BYTES:
        b1, b2 = (B + 31) // 32 * nets, (B + 63) // 64 * nets
        c1, c2 = 1.15 * ((b1 + 255) // 256), 2.0 * ((b2 + 255) // 256)
        if c2 <= c1:
            R = 2
    return R


def skinny_fwd_ok(n_out, k_padded):
    """skinny.h:475."""
    return n_out <= 4 and k_padded <= SKINNY_MAX_K


def narrow_fwd_ok(N, K, lda, ldb):
    """narrow.h:151."""
    return N <= 64 and K >= 32 and K % 32 == 0 and lda % 4 == 0 and ldb % 4 == 0


def narrow_kernel(N, K):
    """narrow.h:154-164 (launch_fwd_narrow_e): (NT, D) of k_fwd_narrow<NT, EPI, D>."""
    K8 = K >> 3
    if N <= 32:                                                    # :157
        return (1, 16 if K8 % 16 == 0 else 8 if K8 % 8 == 0 else 4)
    return (2, 8 if K8 % 8 == 0 else 4)                            # :162-163


def gemm_tile(M, ncols_store, gz):
    """gemm.hip:826-836 (launch_tile<MODE_FWD>): 128 for k_gemm<FWD, 128, 128>, else 64."""
    big = ((M + 127) // 128) * ((ncols_store + 127) // 128) * gz   # :828
    return 128 if big >= 256 and ncols_store >= 128 else 64        # :832


def hidden_path(dims, packed):
    """pqlk_mlp_forward: "fused" (one launch, fused.h), "gemm" (one k_gemm<FWD, EPI_ELU> launch per hidden layer), or None."""
    if len(dims) == 2:
        return None
    return "fused" if packed and fusable(dims) else "gemm"


def head_path(dims, nets, packed, B):
    """The output layer's kernel in pqlk_mlp_forward (gemm.hip; PQLK_NO_FUSED_HEAD unset):
    ("fused", R, wide) | ("skinny",) | ("narrow", NT, D) | ("gemm", 64 | 128)."""
    N = dims[-1]
    buf_ld = fusable(dims)
    if packed and buf_ld and head_fusable(dims):                   # fused_with_head
        return ("fused", fused_rows(dims, nets, buf_ld, B), fused_wide(dims))   # launch_fused_hidden
    K = ld(dims[-2])                                               # MlpGeom::ld
    lda = ldb = K                                                  # x with ldx = pqlk_ld(in), else the stash; the arena
    if skinny_fwd_ok(N, K):
        return ("skinny",)
    if narrow_fwd_ok(N, K, lda, ldb):
        return ("narrow",) + narrow_kernel(N, K)
    return ("gemm", gemm_tile(B, ld(N), nets))                     # launch_auto<MODE_FWD>, ncols_store = pqlk_ld(out)


def narrow_vec(N, place):
    """narrow.h:84-85: the 16-byte epilogue of k_fwd_narrow.  ncols_store is a multiple of 32 and the bias, the output block and
    the draw start 16-byte aligned in these tests, so N % 4 and the second destination decide."""
    return N % 4 == 0 and place in (None, "aligned")


def gemm_full_tiles(B, N, tile, act, place):
    """gemm.hip:662: number of tiles of the head GEMM that take the 16-byte `full` epilogue."""
    if act == ACT_TANH_NOISE or place is not None:
        return 0
    return (B // tile) * (N // tile)


def smallest_b(pred, hi=1 << 20):
    for B in range(1, hi):
        if pred(B):
            return B
    raise AssertionError("no batch size below the cap satisfies the predicate")


# ---------------------------------------------------------------- the table
Case = namedtuple("Case", "name dims nets packed B path")

# smallest batches at which the mirror picks 64-row fused blocks / 128 x 128 GEMM tiles (the CPU tests prove they are minimal)
B_FUSED_R2_2NETS = smallest_b(lambda B: head_path([12, 64, 6], 2, True, B) == ("fused", 2, False))
B_FUSED_R2_1NET = smallest_b(lambda B: head_path([12, 64, 6], 1, True, B) == ("fused", 2, False))
B_GEMM128_1NET = smallest_b(lambda B: head_path([32, 100], 1, False, B) == ("gemm", 128))
B_GEMM128_2NETS = 128 * 128 + 3

_TABLE = [
    # dims, nets, packed?, batches, expected path
    # ---- fused head (fused.h fused_head), inside k_mlp_fwd_fused<1, 2>
    ([12, 64, 6], 1, True, (1, 33, 65), ("fused", 1, False)),
    ([12, 64, 6], 2, True, (33, 97), ("fused", 1, False)),          # 97 rows, 2 nets: four tiles, the XCD-aware block map (fused.h:386)
    ([11, 64, 6], 1, True, (33,), ("fused", 1, False)),             # the learner's out2 = x[:, O:] at O = 11
    ([10, 32, 32], 1, True, (33,), ("fused", 1, False)),            # exactly 32 outputs: no pad column
    ([10, 32, 32], 2, True, (33,), ("fused", 1, False)),
    ([20, 64, 21], 1, True, (33,), ("fused", 1, False)),
    # ---- <1, 4>: a hidden layer wider than 512
    ([8, 544, 3], 1, True, (33,), ("fused", 1, True)),
    ([8, 544, 3], 2, True, (33,), ("fused", 1, True)),
    # ---- <2, 2>: 64-row blocks
    ([12, 64, 6], 2, True, (B_FUSED_R2_2NETS,), ("fused", 2, False)),
    ([12, 64, 6], 1, True, (B_FUSED_R2_1NET,), ("fused", 2, False)),
    # ---- k_skinny_fwd
    ([12, 64, 1], 1, False, (33,), ("skinny",)),
    ([12, 64, 1], 2, False, (33,), ("skinny",)),
    ([12, 64, 4], 1, False, (1, 33, 65), ("skinny",)),
    ([12, 64, 4], 2, False, (33,), ("skinny",)),
    ([40, 3], 1, False, (33,), ("skinny",)),                        # one layer: the input is x itself
    # ---- k_fwd_narrow<1, EPI, D>
    ([12, 32, 5], 1, False, (1, 33, 65), ("narrow", 1, 4)),
    ([12, 32, 5], 2, False, (33,), ("narrow", 1, 4)),
    ([12, 64, 20], 1, False, (33,), ("narrow", 1, 8)),
    ([12, 64, 20], 2, False, (33,), ("narrow", 1, 8)),
    ([12, 128, 21], 1, False, (33,), ("narrow", 1, 16)),
    ([12, 128, 32], 1, False, (33,), ("narrow", 1, 16)),
    ([12, 96, 32], 1, False, (33,), ("narrow", 1, 4)),              # K / 8 = 12: three trips of the depth-4 ring
    ([12, 96, 21], 2, False, (33,), ("narrow", 1, 4)),
    ([8, 1056, 2], 1, False, (33,), ("narrow", 1, 4)),              # K > 1024: the skinny kernel declines, N <= 4 lands here
    ([8, 1056, 4], 1, False, (33,), ("narrow", 1, 4)),              # ... and N = 4 on the 16-byte epilogue (bias quad clamped to N - 4 = 0)
    ([64, 20], 1, False, (33,), ("narrow", 1, 8)),                  # one layer
    # ---- k_fwd_narrow<2, EPI, D>
    ([12, 64, 33], 1, False, (1, 33, 65), ("narrow", 2, 8)),
    ([12, 64, 33], 1, True, (33,), ("narrow", 2, 8)),               # under the fused hidden stack (head not fusable: 33 outputs)
    ([12, 64, 51], 1, False, (33,), ("narrow", 2, 8)),
    ([12, 64, 64], 1, False, (33,), ("narrow", 2, 8)),
    ([12, 64, 64], 2, False, (33,), ("narrow", 2, 8)),
    ([12, 96, 33], 1, False, (33,), ("narrow", 2, 4)),
    ([12, 96, 51], 1, False, (33,), ("narrow", 2, 4)),
    ([12, 96, 51], 2, False, (33,), ("narrow", 2, 4)),
    ([12, 96, 64], 1, False, (33,), ("narrow", 2, 4)),
    # ---- k_gemm<FWD, 64, 64>; the hidden layer is 48 wide: not fusable, so k_gemm's ELU epilogue runs underneath
    ([16, 48, 70], 1, False, (1, 33, 65), ("gemm", 64)),            # edge tile
    ([16, 48, 70], 2, False, (33,), ("gemm", 64)),
    ([16, 48, 128], 1, False, (1, 33, 65), ("gemm", 64)),           # 65 rows: two full tiles (16-byte epilogue) over two ragged ones
    ([16, 48, 128], 2, False, (65,), ("gemm", 64)),
    # ---- k_gemm<FWD, 128, 128>
    ([32, 100], 2, False, (B_GEMM128_2NETS,), ("gemm", 128)),
    ([32, 100], 1, False, (B_GEMM128_1NET,), ("gemm", 128)),
]


def _name(dims, nets, packed, B):
    return "x".join(str(d) for d in dims) + f"-n{nets}-{'packed' if packed else 'layers'}-B{B}"


CASES = [Case(_name(dims, nets, packed, B), dims, nets, packed, B, path)
         for dims, nets, packed, Bs, path in _TABLE for B in Bs]
CASE_BY_NAME = {c.name: c for c in CASES}
assert len(CASE_BY_NAME) == len(CASES)

# every path tuple the forward can end in
PATHS = [("fused", 1, False), ("fused", 1, True), ("fused", 2, False), ("skinny",), ("narrow", 1, 4), ("narrow", 1, 8),
         ("narrow", 1, 16), ("narrow", 2, 4), ("narrow", 2, 8), ("gemm", 64), ("gemm", 128)]


def placements(case):
    """Second destinations the GPU test runs on this case.  out2 needs one net.  "aligned": column 8 of a (B, ld + 32) sentinel
    matrix; "misaligned": column 3 of a sentinel matrix with an odd row stride; "alias" (fused head only): out2 = x[:, O:] into the
    input tile the call reads, the learners' form (include/pqlk.h: columns >= dims[0] of x are ignored on the fused path)."""
    if case.nets != 1:
        return [None]
    return [None, "aligned", "misaligned"] + (["alias"] if case.path[0] == "fused" else [])


def cells():
    """(case, activation, placement) of every forward whose output the GPU test asserts."""
    return [(c, act, pl) for c in CASES for act in ACTS for pl in placements(c)]


def out2_geometry(case, place):
    """(rows, row stride, first column) of the matrix that holds out2; the alias form views the (B, ldx) input tile."""
    N, ldo = case.dims[-1], ld(case.dims[-1])
    if place == "aligned":
        return case.B, ldo + 32, 8
    if place == "misaligned":
        return case.B, ldo + 33, 3
    assert place == "alias"
    return case.B, ld(case.dims[0] + N), case.dims[0]


# ---------------------------------------------------------------- inputs
HEAD_GAIN = 4.0
DRAW_SCALE = 0.5


def weights(case):
    """[net][layer] -> (W (out, in), b (out,)), seeds and bounds of test_mlp_shape_sweep_vs_oracle.  The OUTPUT layer is
    multiplied by HEAD_GAIN: with |noise| <= NOISE_CLIP = 0.2 the outer clamp of TANH_NOISE binds only where |tanh z| > 0.8,
    |z| > 1.1, which pre-activations of the default 1 / sqrt(fan_in) scale almost never reach."""
    dims, out = case.dims, []
    for n in range(case.nets):
        net = []
        for l in range(len(dims) - 1):
            bound = 1.0 / np.sqrt(dims[l])
            w = dd.uniform((dims[l + 1], dims[l]), 300 * n + l, -bound, bound)
            b = dd.uniform((dims[l + 1],), 300 * n + l + 60, -bound, bound)
            if l == len(dims) - 2:
                w, b = (w * F32(HEAD_GAIN)).astype(F32), (b * F32(HEAD_GAIN)).astype(F32)
            net.append((w, b))
        out.append(net)
    return out


def x_input(case):
    return dd.uniform((case.B, case.dims[0]), 9, -2, 2)


# one-row cases have a handful of elements: the draw's seed is moved on until both clamps bind on some of them (found on the
# float64 reference alone, test_noise_design_makes_both_clamps_bind holds it there)
DRAW_SALT = {((12, 64, 6), 1): 3, ((12, 64, 4), 1): 1}


def draw_input(case):
    """(B, N) contiguous, uniform on +-DRAW_SCALE: NOISE_STD * draw leaves +-NOISE_CLIP on about half of the elements."""
    salt = DRAW_SALT.get((tuple(case.dims), case.B), 0)
    return dd.uniform((case.B, case.dims[-1]), 4000 + 7 * case.dims[-1] + case.dims[-2] + 1000 * salt, -DRAW_SCALE, DRAW_SCALE)


# ---------------------------------------------------------------- references
def elu64(z):
    return np.where(z > 0, z, np.expm1(np.minimum(z, 0.0)))


def forward64(case, net):
    """float64 pre-activation of the output layer from x through float64 hidden layers (the design of the inputs; the GPU
    checks use the kernel's own last hidden block instead)."""
    h = x_input(case).astype(np.float64)
    ws = weights(case)[net]
    for w, b in ws[:-1]:
        h = elu64(h @ w.astype(np.float64).T + b.astype(np.float64))
    w, b = ws[-1]
    return h @ w.astype(np.float64).T + b.astype(np.float64)


def preact64(h, W, b):
    """The head's pre-activation in float64 from ITS input (the stashed last hidden block, or x for one layer)."""
    return h.astype(np.float64) @ W.astype(np.float64).T + b.astype(np.float64)


def bound(h, W, b, k_pad):
    """2 (K_pad + 2) 2^-24 (|h| |W|^T + |b|): twice the first-order error bound of ANY fp32 summation order of K_pad products
    plus a bias."""
    return 2.0 * (k_pad + 2) * 2.0 ** -24 * (np.abs(h).astype(np.float64) @ np.abs(W).astype(np.float64).T + np.abs(b).astype(np.float64))


def smooth32(t, draw, std=NOISE_STD, clip=NOISE_CLIP):
    """clamp(t + clamp(std * draw, +-clip), +-1) in float32, one rounding per operation: the law of include/pqlk.h.  The inner
    clamp sits between the product and the sum, so no contraction can change a bit."""
    t, draw = np.asarray(t, dtype=F32), np.asarray(draw, dtype=F32)
    nz = F32(std) * draw
    nz = np.minimum(np.maximum(nz, -F32(clip)), F32(clip))
    return np.minimum(np.maximum(t + nz, F32(-1)), F32(1)).astype(F32)


def noise_shares(case):
    """On the float64 reference: share of elements on which the inner clamp binds, and on which the outer clamp binds."""
    draw = draw_input(case).astype(np.float64)
    inner = outer = total = 0
    for n in range(case.nets):
        t = np.tanh(forward64(case, n))
        raw = NOISE_STD * draw
        nz = np.clip(raw, -NOISE_CLIP, NOISE_CLIP)
        inner += int((np.abs(raw) > NOISE_CLIP).sum()); outer += int((np.abs(t + nz) > 1.0).sum()); total += t.size
    return inner / total, outer / total


# ---------------------------------------------------------------- checks (numpy in, AssertionError out)
# Measured on the MI355X over every case of the table: tanhf is at most TANH_MEASURED_ULPS ulps of the correctly rounded result
# away from the float64 tanh of the same float32 argument.  The bar is twice that, rounded up to a whole ulp.
TANH_MEASURED_ULPS = 1.403   # k_gemm<FWD, 128, 128>, [32, 100] at 16387 rows; every other path between 0.39 and 1.35
TANH_ULPS = 3
TANH_ABS_CAP = 1e-6


def ulps_off(got, want64):
    """|got - want64| in units of the float32 spacing at want64."""
    w32 = np.abs(want64).astype(F32)
    return np.abs(got.astype(np.float64) - want64) / np.spacing(np.maximum(w32, np.finfo(F32).tiny)).astype(np.float64)


def check_none(out, h, W, b, N, k_pad, what=""):
    """out: (B, ld) of one net.  |out - preact64| <= bound elementwise; pad columns exactly 0."""
    err = np.abs(out[:, :N].astype(np.float64) - preact64(h, W, b))
    lim = bound(h, W, b, k_pad)
    worst = float((err / np.maximum(lim, 1e-300)).max())
    assert np.all(err <= lim), f"{what}: |out - preact64| reaches {worst:.3f} of the bound"
    assert np.all(out[:, N:] == 0), f"{what}: pad columns not zero"
    return worst


def check_tanh(out, z, N, ulps, what=""):
    """out = tanhf(z) for z the ACT_NONE output of the same kernel: within `ulps` of float64 tanh(z), and under the absolute cap."""
    want = np.tanh(z[:, :N].astype(np.float64))
    off = ulps_off(out[:, :N], want)
    worst = float(off.max())
    assert worst <= ulps, f"{what}: tanh is {worst:.2f} ulps off (bar {ulps})"
    assert float(np.abs(out[:, :N].astype(np.float64) - want).max()) <= TANH_ABS_CAP, what
    assert np.all(out[:, N:] == 0), f"{what}: pad columns not zero"
    return worst


def check_noise(out, t, draw, N, what=""):
    """out == smooth32(t, draw) bit for bit, t the ACT_TANH output of the same kernel; draw (B, N) contiguous."""
    want = smooth32(t[:, :N], draw)
    bad = np.argwhere(out[:, :N].view(np.uint32) != want.view(np.uint32))
    assert bad.size == 0, f"{what}: {len(bad)} elements differ from smooth32, first at (row, col) {tuple(bad[0])}"
    assert np.all(out[:, N:] == 0), f"{what}: pad columns not zero"


def check_out2(mat, col0, out, N, sentinel, what=""):
    """mat: the whole matrix holding out2, slack behind it included, as (rows, stride) plus a flat tail.  out2 = mat[:, col0 : col0 + N]
    equals out[:, :N] bit for bit and every other element still holds the sentinel (`sentinel`: same shape as mat, what it held)."""
    got = mat[:, col0:col0 + N]
    bad = np.argwhere(got.view(np.uint32) != out[:, :N].view(np.uint32))
    assert bad.size == 0, f"{what}: out2 differs from the output block at {len(bad)} elements, first at (row, col) {tuple(bad[0])}"
    rest, keep = mat.copy(), sentinel.copy()
    rest[:, col0:col0 + N] = 0; keep[:, col0:col0 + N] = 0
    bad = np.argwhere(rest.view(np.uint32) != keep.view(np.uint32))
    assert bad.size == 0, f"{what}: {len(bad)} elements outside out2 were written, first at (row, col) {tuple(bad[0])}"


def bits_equal(a, b):
    return a.shape == b.shape and bool(np.all(a.view(np.uint32) == b.view(np.uint32)))


# ---------------------------------------------------------------- a float32 numpy model of one head, for the checks' own tests
def model_head(h, W, b, act, draw=None, *, swap_clamps=False, draw_stride=None):
    """What a correct head kernel leaves in one net's (B, ld) output block: float32 dot products (numpy's order), bias, activation
    (tanh correctly rounded from float64), zero pads.  swap_clamps / draw_stride build the wrong kernels the checks must catch:
    the outer clamp applied before the noise is added, the draw indexed with a row stride other than N."""
    B, N = h.shape[0], W.shape[0]
    out = np.zeros((B, ld(N)), dtype=F32)
    z = (h.astype(F32) @ W.astype(F32).T + b.astype(F32)).astype(F32)
    if act == ACT_NONE:
        out[:, :N] = z
        return out
    t = np.tanh(z.astype(np.float64)).astype(F32)
    if act == ACT_TANH:
        out[:, :N] = t
        return out
    flat = np.asarray(draw, dtype=F32).reshape(-1)
    stride = N if draw_stride is None else draw_stride
    idx = (np.arange(B)[:, None] * stride + np.arange(N)[None, :]) % flat.size
    d = flat[idx]
    if swap_clamps:
        nz = F32(NOISE_STD) * d
        v = np.minimum(np.maximum(t, F32(-1)), F32(1)) + nz
        out[:, :N] = np.minimum(np.maximum(v, -F32(NOISE_CLIP)), F32(NOISE_CLIP))
    else:
        out[:, :N] = smooth32(t, d)
    return out
