"""Cases, inputs, references and checks for tests/test_backward_paths_gpu.py and, in the TD family at the end of this file, for
tests/test_td_paths_gpu.py (plain numpy, no GPU, no library).

pqlk_mlp_backward picks, per call, between three implementations of the output layer's backward (skinny.h), per hidden layer a dW
and a dX k_gemm in two tile sizes, two main loops and three block orders (gemm.hip), and for the input gradient a GEMM or
k_dx_slice (narrow.h); pqlk_dpg_critic_backward adds the compact-row chain (minnet.h).  `backward_plan` restates that dispatch so
that every case can name the launches it reaches; tests/test_backward_cases_cpu.py holds the table against it and holds the mirror
against the three host-side quantities of the library that depend on the dispatch.

The backward never runs the forward: the activation stash is an INPUT.  Hidden activations come from {2, 1, 0.5, 0, -0.5, -0.75,
-1} (ELU' = 1, 1, 1, 1, 0.5, 0.25, 0), weights from {-1, 0, 1}, x and dy are integers in [-2, 2], the tanh outputs come from
{0, +-0.5, +-1} (1 - a^2 = 1, 0.75, 0): every product is a dyadic rational.  The library is built with -ffp-contract=off.  For an
output element sum_i t_i whose terms are all multiples of 2^-g, if sum_i |t_i| 2^g <= 2^24 then every partial sum in any order or
grouping is exactly representable in fp32: an MFMA chain, a split-slab sum, a wave fold and a float64 numpy matmul give the same
value.  `exactness_bits` measures that condition per case (the CPU test asserts it), and the checks are `==`: no tolerance
anywhere.  (Values are compared, so +0 == -0: the sign of a zero sum is a property of the summation order, not of the sum.)

Source lines cited below are those of pql_amd/csrc at the commit that added this file."""
import functools
from collections import namedtuple

import numpy as np

import detdata as dd
import reduction_cases as rc

F32, F64 = np.float32, np.float64
POISON, SLACK, IN_ONE = rc.POISON, rc.SLACK, rc.IN_ONE

# ---------------------------------------------------------------- the library's constants
SKINNY_MAX_N, SKINNY_MAX_K = 16, 1024     # skinny.h:9-10
SKB_ROWS = 64                             # skinny.h:285
KT, KT_MAX = 16, 32                       # gemm.hip:63-65 (PQLK_KT, KT_MAX)
MN_TILE = 128                             # minnet.h:16
LDS_BYTES = 160 * 1024                    # narrow.h:463
E_WORKSPACE = 6                           # include/pqlk.h:46


def ld(cols):
    """pqlk_ld (replay.hip:7): round up to 32 floats."""
    return (max(int(cols), 1) + 31) // 32 * 32


def round_up(a, m):
    return (a + m - 1) // m * m


def cdiv(a, m):
    return (a + m - 1) // m


# ---------------------------------------------------------------- mirror: the output layer (skinny.h)
def skinny_bwd_ok(n_out, k_padded):
    """skinny.h:476."""
    return n_out <= SKINNY_MAX_N and k_padded <= SKINNY_MAX_K


def skinny_bwd_ch(k_padded):
    """skinny.h:423: template CH of k_skinny_bwd."""
    c = cdiv(k_padded, 256)
    return c if c <= 2 else 4


def skinny_bwd_nb(n_out):
    """skinny.h:424: template NB of k_skinny_bwd."""
    return 1 if n_out == 1 else 4 if n_out <= 4 else 8 if n_out <= 8 else 16


def skinny_bwd_fused_ok(n_out, k_padded):
    """skinny.h:425-427."""
    return n_out <= SKINNY_MAX_N and k_padded <= SKINNY_MAX_K and skinny_bwd_nb(n_out) * skinny_bwd_ch(k_padded) <= 16


def skinny_bwd_rows(m, groups):
    """skinny.h:429-433: rows per block of k_skinny_bwd."""
    r = SKB_ROWS
    while r > 16 and cdiv(m, r) * groups < 512:
        r >>= 1
    return r


def skinny_bwd_blocks(m, groups):
    """skinny.h:434."""
    return cdiv(m, skinny_bwd_rows(m, groups))


def skinny_bwd_kernel(n_out, k_padded):
    """skinny.h:451-471 (launch_skinny_bwd without the TD head): (NB, CH) of k_skinny_bwd<NB, CH>."""
    ch = skinny_bwd_ch(k_padded)
    if n_out == 1:
        return (1, ch)                                             # :458-462
    if n_out <= 4:
        return (4, ch)                                             # :463-467
    if n_out <= 8 and ch <= 2:
        return (8, ch)                                             # :468-469
    return (16, 1)                                                 # :470


def skinny_dw_cls(k_padded, splits, groups):
    """skinny.h:508-511 (launch_skinny_dw): CLS of k_skinny_dw<CLS>."""
    return 16 if cdiv(k_padded, 64) * splits * groups >= 256 else 4


def skinny_dx_blocks(m):
    """skinny.h:493-495 (launch_skinny_dx): the grid is capped at 2048 blocks of four rows."""
    return min(cdiv(m, 4), 2048)


def head_is_fused(dims):
    """gemm.hip, head_is_fused (head_bwd_kind == HEAD_FUSED)."""
    L = len(dims) - 1
    return L >= 2 and skinny_bwd_ok(dims[L], ld(dims[L - 1])) and skinny_bwd_fused_ok(dims[L], ld(dims[L - 1]))


# ---------------------------------------------------------------- mirror: k_gemm (gemm.hip)
def launch_tile(mode, epi, M, ncols, gz):
    """gemm.hip:826-836: 128 for k_gemm<MODE, 128, 128>, else 64."""
    big = cdiv(M, 128) * cdiv(ncols, 128) * gz                     # :828
    return 128 if big >= 256 and ncols >= 128 and epi != "DTANH_SLICE" else 64   # :832


def gemm_plan(mode, epi, tile, M, N, K, lda, ldb, ncols_store, gz, splits=1, rows_per_split=0, col0=0, ncol=0):
    """gemm.hip:751-782 with PQLK_GEMM_DMA and PQLK_GEMM_XCD unset and every operand 16-byte aligned (the arena, the stash, the
    workspace and the tests' buffers all are; group strides are multiples of 32 floats): (grid, loop, xcd, n_base).  mode: "dW" |
    "dX" | "FWD" -- the forward (tests/forward_hidden_cases.py) has dX's grid and tile groups and never the LDS-DMA loop (:768)."""
    ncols, n_base = (N if mode == "dW" else ncols_store), 0        # :753-754
    if epi == "DTANH_SLICE":
        n_base = col0 & ~3                                         # :756
        ncols = col0 + ncol - n_base                               # :757
    grid = (cdiv(ncols, tile), cdiv(M, tile), gz)                  # :759
    tiles, group = grid[0] * grid[1] * grid[2], (grid[0] * grid[1] if mode == "dW" else grid[0])   # :761
    xcd = "groups" if tiles % (8 * group) == 0 else "runs" if tiles >= 64 else 0                   # :764-765
    dma = False
    if mode != "FWD" and epi in ("NONE", "DELU"):                  # :768
        dma = M % tile == 0 and lda % 4 == 0 and ldb % 4 == 0      # :769-770
        if mode == "dX":                                           # :771
            dma = dma and ncols % tile == 0 and N % tile == 0 and K % (4 * KT) == 0 and K <= lda and ncols <= ldb
        else:                                                      # :777-778
            dma = (dma and round_up(N, tile) <= ldb and rows_per_split % (4 * KT) == 0 and K % rows_per_split == 0
                   and K // rows_per_split == splits and M <= lda and N <= ldb)
    return grid, ("dma" if dma else "staged"), xcd, n_base


def gemm_launch(mode, epi, M, N, K, lda, ldb, ncols_store, gz, **kw):
    """One k_gemm launch tuple: (mode, epi, tile, loop, xcd, has_edge_tile).  An edge tile is one the epilogue does not take as a
    `whole` tile (gemm.hip:556, :662): a ragged last row tile or column tile; the slice epilogue is per element throughout."""
    ncols = N if mode == "dW" else ncols_store
    tile = launch_tile(mode, epi, M, ncols, gz)
    _, loop, xcd, _ = gemm_plan(mode, epi, tile, M, N, K, lda, ldb, ncols_store, gz, **kw)
    edge = M % tile != 0 or N % tile != 0 or epi == "DTANH_SLICE"
    return (mode, epi, tile, loop, xcd, edge)


# ---------------------------------------------------------------- mirror: the input-gradient slice (narrow.h)
def dx_slice_lds(groups, K):
    """narrow.h:456-459."""
    return max(4 * 32 * (groups * K // 4 + 4) * 4, 16384)


def dx_slice_ok(groups, K, ncol, lda):
    """narrow.h:461-464 for an EPI_DTANH_SLICE, zsum product."""
    return ncol <= 32 and K % 32 == 0 and 4 % groups == 0 and lda % 4 == 0 and dx_slice_lds(groups, K) <= LDS_BYTES


def dx_slice_depth(groups, K):
    """narrow.h:484, :500-502 (launch_dx_slice without the actor head): D of k_dx_slice<D>."""
    K8 = groups * K // 32
    return 16 if K8 % 16 == 0 else 4 if K8 % 4 == 0 else 1


# ---------------------------------------------------------------- mirror: pqlk_mlp_backward (gemm.hip, mlp_backward_impl)
def rows_per_split(B, splits):
    """gemm.hip, bwd_head and bwd_layer_dw."""
    return round_up(cdiv(B, splits), KT_MAX)


def empty_splits(B, splits):
    """Splits whose first row lies past the batch: their slabs must come out as zeros."""
    return sum(1 for s in range(splits) if s * rows_per_split(B, splits) >= B)


def backward_plan(dims, nets, B, splits, want_grads, dx_form, ldx=None):
    """One tuple per launch of pqlk_mlp_backward, in launch order.  dx_form: None | "full" | ("slice", col0, cols).
    ("skinny_bwd", NB, CH, rows) | ("skinny_dw", CLS) | ("skinny_dx",) | gemm_launch tuples | ("dx_slice", D, groups) |
    ("reduce", head partials folded?)."""
    L = len(dims) - 1
    ldx = ld(dims[0]) if ldx is None else ldx
    plan, head_parts = [], False
    for l in range(L - 1, -1, -1):                                 # mlp_backward_impl
        ld_out, ld_in = ld(dims[l + 1]), ld(dims[l])               # MlpGeom::ld
        in_ld = ldx if l == 0 else ld_in                           # bwd_layer_io
        skinny = l == L - 1 and skinny_bwd_ok(dims[l + 1], ld_in) and in_ld >= ld_in   # bwd_head
        if skinny:
            if want_grads and head_is_fused(dims):                 # HEAD_FUSED
                plan.append(("skinny_bwd",) + skinny_bwd_kernel(dims[l + 1], ld_in) + (skinny_bwd_rows(B, nets),))
                head_parts = True
                continue
            if want_grads:                                         # HEAD_SKINNY
                plan.append(("skinny_dw", skinny_dw_cls(ld_in, splits, nets)))
            if l > 0:
                plan.append(("skinny_dx",))
                continue
            if dx_form is None:                                    # bwd_layer_dx
                continue
        if want_grads and not skinny:                              # bwd_layer_dw
            plan.append(gemm_launch("dW", "NONE", dims[l + 1], ld_in, B, ld_out, in_ld, ld_out, nets * splits, splits=splits,
                                    rows_per_split=rows_per_split(B, splits)))
        if l > 0:                                                  # bwd_layer_dx
            plan.append(gemm_launch("dX", "DELU", B, dims[l], dims[l + 1], ld_out, ld_in, ld_in, nets))
        elif dx_form is not None:
            if dx_form == "full":
                plan.append(gemm_launch("dX", "NONE", B, dims[0], dims[1], ld_out, ld_in, ld_in, 1))
            else:
                _, col0, cols = dx_form
                if dx_slice_ok(nets, dims[1], cols, ld_out):
                    plan.append(("dx_slice", dx_slice_depth(nets, dims[1]), nets))
                else:
                    plan.append(gemm_launch("dX", "DTANH_SLICE", B, dims[0], dims[1], ld_out, ld_in, ld_in, 1, col0=col0, ncol=cols))
    if want_grads:                                                 # k_reduce_slabs
        plan.append(("reduce", head_parts))
    return plan


# ---------------------------------------------------------------- mirror: the host-side sizes
def net_stride(dims):
    """gemm.hip, mlp_geom (pqlk_mlp_net_stride)."""
    return sum(dims[l + 1] * ld(dims[l]) + ld(dims[l + 1]) for l in range(len(dims) - 1))


def layer_offsets(dims, layer):
    """gemm.hip, mlp_geom (pqlk_mlp_layer_offsets): (w_off, b_off) inside one net's block."""
    n = sum(dims[l + 1] * ld(dims[l]) + ld(dims[l + 1]) for l in range(layer))
    return n, n + dims[layer + 1] * ld(dims[layer])


def acts_floats(dims, nets, B):
    """gemm.hip, mlp_geom (pqlk_mlp_acts_floats)."""
    return sum(nets * B * ld(dims[l + 1]) for l in range(len(dims) - 1))


def act_offset(dims, nets, B, net, layer):
    """gemm.hip, mlp_geom (pqlk_mlp_act_offset): (offset, ld) of one net's block of one layer's activations in the stash."""
    return sum(nets * B * ld(dims[l + 1]) for l in range(layer)) + net * B * ld(dims[layer + 1]), ld(dims[layer + 1])


def max_hidden_ld(dims):
    """gemm.hip, mlp_geom (MlpGeom::max_hidden_ld)."""
    return max(ld(d) for d in dims[1:])


def head_part_floats(dims, nets, B):
    """gemm.hip, bwd_ws (BwdWs::head_part_floats)."""
    hf = dims[-1] * ld(dims[-2]) + ld(dims[-1])
    return max(skinny_bwd_blocks(B, nets), 2 * round_up(B, 128) // 32) * nets * hf


def bwd_ws_floats(dims, nets, B, splits):
    """gemm.hip, bwd_ws (pqlk_mlp_bwd_ws_floats)."""
    return 2 * nets * B * max_hidden_ld(dims) + splits * net_stride(dims) * nets + head_part_floats(dims, nets, B)


def bwd_ws_required(dims, nets, B, splits, want_grads):
    """gemm.hip, bwd_ws as mlp_backward_impl asks for it: what the call itself insists on (without grads neither slabs nor head partials)."""
    return bwd_ws_floats(dims, nets, B, splits) if want_grads else 2 * nets * B * max_hidden_ld(dims)


def norm_parts(dims, nets):
    """gemm.hip, pqlk_mlp_norm_parts (reduce_main_blocks, head_fold_blocks): the head's fold blocks exist when head_is_fused."""
    main = min(max(cdiv(net_stride(dims) * nets // 4, 256), 1), 1024)
    hq = (dims[-1] * ld(dims[-2]) + ld(dims[-1])) // 4 * nets
    return main + (cdiv(hq, 4) if head_is_fused(dims) else 0)


def minnet_ok(dims, nets, dx_cols):
    """gemm.hip, minnet_ok (compact_chain_ok) with dx and dx_tanh_of given."""
    L = len(dims) - 1
    if nets != 2 or L < 3 or dims[L] != 1 or dx_cols > 32 or not skinny_bwd_ok(1, ld(dims[L - 1])):
        return False
    return all(dims[l] % 32 == 0 for l in range(1, L)) and all(dims[l] % 128 == 0 for l in range(1, L - 1))


def dpg_ws_floats(dims, nets, B):
    """gemm.hip, compact_ws and pqlk_dpg_backward_ws_floats."""
    cap = 2 * round_up(B, MN_TILE)
    return max(bwd_ws_floats(dims, nets, B, 1), 2 * cap * max_hidden_ld(dims) + 2 * cap + 64)


def smallest(pred, lo=1, hi=1 << 20):
    for v in range(lo, hi):
        if pred(v):
            return v
    raise AssertionError("no value below the cap satisfies the predicate")


def default_splits(B, cap=16):
    """pql_amd/models/mlp.py default_splits."""
    return max(1, min(cap, B // 512))


# ---------------------------------------------------------------- the table
Case = namedtuple("Case", "name dims nets B splits form col0 cols ldx must")
FORMS = ("gdx", "g", "dx", "slice")       # grads + full dx | grads only | dx only (grads = NULL) | slice only (grads = NULL)


def _plan_of(dims, nets, B, splits, form, col0=0, cols=0, ldx=None):
    dx_form = {"gdx": "full", "g": None, "dx": "full", "slice": ("slice", col0, cols)}[form]
    return backward_plan(dims, nets, B, splits, form in ("gdx", "g"), dx_form, ldx)


def plan(case):
    return _plan_of(case.dims, case.nets, case.B, case.splits, case.form, case.col0, case.cols, case.ldx)


# thresholds found on the mirror (the CPU tests prove they are minimal)
B_ROWS32 = smallest(lambda B: skinny_bwd_rows(B, 2) == 32)                      # k_skinny_bwd at 32 rows per block, two nets
B_ROWS64 = smallest(lambda B: skinny_bwd_rows(B, 2) == 64)
B_DX_CAP = smallest(lambda B: cdiv(B, 4) > 2048)                                # k_skinny_dx walks its capped grid twice
WIDE = [8, 512, 512, 1]                                                         # the 128 x 128 tiles, two nets
B_DX128 = smallest(lambda B: launch_tile("dX", "DELU", B, 512, 2) == 128)
S_DW128 = smallest(lambda s: launch_tile("dW", "NONE", 512, 512, 2 * s) == 128, hi=65)
S_CLS16 = smallest(lambda s: skinny_dw_cls(1024, s, 2) == 16, hi=65)            # [8, 1024, 6], two nets

_SB = "skinny_bwd"
_TABLE = [
    # dims, nets, B, splits, form, {col0, cols, ldx}, launches the row is there for
    # ---- k_skinny_bwd<NB, CH>: all nine instantiations, one and two nets, B % 16 != 0, 16-row blocks
    ([8, 32, 1], 1, 37, 1, "gdx", {}, [(_SB, 1, 1, 16)]),
    ([8, 32, 1], 2, 37, 1, "g", {}, [(_SB, 1, 1, 16)]),
    ([8, 32, 1], 1, 1, 1, "gdx", {}, [(_SB, 1, 1, 16)]),                        # a lone row
    ([8, 32, 1], 2, 1, 1, "gdx", {}, [(_SB, 1, 1, 16)]),
    ([8, 288, 1], 1, 37, 1, "g", {}, [(_SB, 1, 2, 16)]),
    ([8, 288, 1], 2, 37, 1, "gdx", {}, [(_SB, 1, 2, 16)]),
    ([8, 544, 1], 1, 37, 1, "gdx", {}, [(_SB, 1, 4, 16)]),                      # 544 = three chunks of 256: CH = 4 with one idle
    ([8, 544, 1], 2, 37, 1, "g", {}, [(_SB, 1, 4, 16)]),
    ([8, 1024, 1], 1, 37, 1, "g", {}, [(_SB, 1, 4, 16)]),
    ([8, 1024, 1], 2, 37, 1, "gdx", {}, [(_SB, 1, 4, 16)]),
    ([8, 64, 3], 1, 37, 1, "gdx", {}, [(_SB, 4, 1, 16)]),
    ([8, 64, 3], 2, 37, 1, "g", {}, [(_SB, 4, 1, 16)]),
    ([8, 512, 4], 1, 37, 1, "g", {}, [(_SB, 4, 2, 16)]),
    ([8, 512, 4], 2, 37, 1, "gdx", {}, [(_SB, 4, 2, 16)]),
    ([8, 800, 2], 1, 37, 1, "gdx", {}, [(_SB, 4, 4, 16)]),
    ([8, 800, 2], 2, 37, 1, "g", {}, [(_SB, 4, 4, 16)]),
    ([8, 96, 5], 1, 37, 1, "g", {}, [(_SB, 8, 1, 16)]),                         # CH == 1 && NB >= 8: eight rows in flight, four per block
    ([8, 96, 5], 2, 37, 1, "gdx", {}, [(_SB, 8, 1, 16)]),
    ([8, 320, 8], 1, 37, 1, "gdx", {}, [(_SB, 8, 2, 16)]),
    ([8, 320, 8], 2, 37, 1, "g", {}, [(_SB, 8, 2, 16)]),
    ([8, 256, 16], 1, 37, 1, "g", {}, [(_SB, 16, 1, 16)]),
    ([8, 256, 16], 2, 37, 1, "gdx", {}, [(_SB, 16, 1, 16)]),
    ([8, 36, 12], 1, 37, 1, "gdx", {}, [(_SB, 16, 1, 16)]),                     # a last hidden width that is no multiple of 32
    ([8, 36, 12], 2, 37, 1, "g", {}, [(_SB, 16, 1, 16)]),
    # ---- 32- and 64-row blocks, one row past a block boundary
    ([8, 32, 1], 2, B_ROWS32, default_splits(B_ROWS32), "gdx", {}, [(_SB, 1, 1, 32)]),
    ([8, 32, 1], 2, B_ROWS64, default_splits(B_ROWS64), "gdx", {}, [(_SB, 1, 1, 64)]),
    # ---- the non-fused skinny head: k_skinny_dw<4> / <16> + k_skinny_dx
    ([8, 288, 9], 1, 37, 1, "gdx", {}, [("skinny_dw", 4), ("skinny_dx",)]),     # N % 4 != 0: scalar dY staging
    ([8, 288, 9], 2, 130, 64, "g", {}, [("skinny_dw", 16)]),                    # 64 splits of 32 rows, 59 of them empty
    ([8, 288, 12], 1, 37, 1, "g", {}, [("skinny_dw", 4), ("skinny_dx",)]),      # N % 4 == 0: 16-byte dY staging
    ([8, 288, 12], 2, 96, 8, "gdx", {}, [("skinny_dw", 4)]),                    # B = 96 in 8 splits: splits 3..7 are empty
    ([8, 544, 5], 1, 37, 1, "gdx", {}, [("skinny_dw", 4), ("skinny_dx",)]),
    ([8, 544, 5], 2, 1100, default_splits(1100), "g", {}, [("skinny_dw", 4)]),
    ([40, 3], 1, 37, 1, "gdx", {}, [("skinny_dw", 4), ("dX", "NONE", 64, "staged", 0, True)]),   # one layer: CrossQ's Linear
    ([40, 3], 2, 37, 1, "g", {}, [("skinny_dw", 4)]),
    ([8, 1024, 6], 2, 300, S_CLS16, "g", {}, [("skinny_dw", 16)]),
    ([8, 1024, 6], 2, 96, S_CLS16, "gdx", {}, [("skinny_dw", 16)]),             # ... with empty splits
    ([8, 1024, 6], 2, 300, S_CLS16 - 1, "g", {}, [("skinny_dw", 4)]),
    ([8, 64, 3], 2, B_DX_CAP, 1, "dx", {}, [("skinny_dx",), ("dX", "NONE", 64, "staged", "runs", True)]),   # grads = NULL: dX alone
    ([8, 288, 12], 1, 37, 1, "dx", {}, [("skinny_dx",)]),
    # ---- the GEMM head: more than 16 outputs, or a last hidden layer wider than 1024
    ([8, 64, 17], 1, 37, 1, "gdx", {}, [("dW", "NONE", 64, "staged", 0, True), ("dX", "DELU", 64, "staged", 0, True)]),
    ([8, 64, 51], 2, 70, 1, "g", {}, [("dW", "NONE", 64, "staged", 0, True)]),
    ([8, 1056, 4], 1, 37, 1, "gdx", {}, [("dX", "DELU", 64, "staged", 0, True)]),
    ([8, 1056, 4], 2, 37, 1, "dx", {}, [("dX", "DELU", 64, "staged", 0, True)]),
    # ---- k_gemm dW and dX(DELU) on 64 x 64 tiles: both loops, whole and ragged grids, short reductions
    ([8, 64, 64, 17], 1, 128, 1, "gdx", {}, [("dW", "NONE", 64, "dma", 0, False), ("dX", "DELU", 64, "dma", 0, False)]),   # dX: K = 64, one DMA group
    ([8, 64, 64, 17], 2, 64, 1, "g", {}, [("dW", "NONE", 64, "dma", 0, False)]),          # dW: 64 rows, one four-stage DMA group
    ([8, 64, 64, 17], 1, 96, 1, "g", {}, [("dW", "NONE", 64, "staged", 0, False)]),       # dW: 96 rows, register-staged interior loop
    ([8, 64, 96, 17], 1, 128, 1, "gdx", {}, [("dX", "DELU", 64, "staged", 0, False)]),    # dX: K = 96
    ([8, 64, 64, 17], 2, 96, 8, "gdx", {}, [("dW", "NONE", 64, "staged", "groups", False)]),   # empty splits on the GEMM dW
    ([8, 64, 64, 17], 2, 130, 64, "g", {}, [("dW", "NONE", 64, "staged", "groups", False)]),
    ([8, 64, 64, 17], 1, 1100, default_splits(1100), "g", {}, [("dW", "NONE", 64, "staged", 0, False)]),
    ([8, 64, 64, 17], 1, 512, 1, "g", {}, [("dX", "DELU", 64, "dma", "groups", False)]),
    ([8, 64, 64, 17], 1, 4100, 1, "g", {}, [("dX", "DELU", 64, "staged", "runs", True)]),
    ([8, 64, 64, 3], 1, 96, 8, "gdx", {}, [(_SB, 4, 1, 16), ("dW", "NONE", 64, "staged", "groups", False)]),   # fused head ignores splits, the layers below do not
    ([48, 100, 36, 12], 1, 130, 1, "gdx", {}, [("dW", "NONE", 64, "staged", 0, True), ("dX", "DELU", 64, "staged", 0, True)]),   # widths that are no multiples of 32
    ([88, 64, 3], 1, 128, 1, "gdx", {"ldx": 128}, [("dW", "NONE", 64, "dma", 0, True)]),  # the input tile is wider than pqlk_ld(88) = 96: the DMA loop loads 128 columns
    ([88, 64, 3], 2, 128, 2, "g", {"ldx": 128}, [("dW", "NONE", 64, "dma", 0, True)]),
    # ---- 128 x 128 tiles: the smallest batch (dX) and split count (dW) that select them, then whole tiles under the DMA loop
    (WIDE, 2, B_DX128, S_DW128, "g", {}, [("dW", "NONE", 128, "staged", "groups", False), ("dX", "DELU", 128, "staged", "groups", True)]),
    (WIDE, 2, 4096, S_DW128, "gdx", {}, [("dW", "NONE", 128, "dma", "groups", False), ("dX", "DELU", 128, "dma", "groups", False)]),
    (WIDE, 2, 96, S_DW128, "g", {}, [("dW", "NONE", 128, "staged", "groups", False)]),    # 128-row tiles over empty splits
    (WIDE, 2, 256, 2, "g", {}, [("dW", "NONE", 64, "dma", "runs", False)]),
    # ---- input gradient: k_dx_slice<D> at every depth, one and two nets
    ([40, 512, 1], 1, 37, 1, "slice", {"col0": 5, "cols": 32}, [("dx_slice", 16, 1)]),
    ([40, 256, 1], 2, 130, 1, "slice", {"col0": 8, "cols": 5}, [("dx_slice", 16, 2)]),    # col0 % 4 == 0: 16-byte weight staging
    ([40, 128, 1], 1, 130, 1, "slice", {"col0": 3, "cols": 1}, [("dx_slice", 4, 1)]),
    ([40, 64, 1], 2, 37, 1, "slice", {"col0": 7, "cols": 32}, [("dx_slice", 4, 2)]),
    ([40, 32, 1], 1, 37, 1, "slice", {"col0": 5, "cols": 5}, [("dx_slice", 1, 1)]),
    ([40, 32, 1], 2, 130, 1, "slice", {"col0": 8, "cols": 32}, [("dx_slice", 1, 2)]),
    ([40, 96, 1], 1, 1, 1, "slice", {"col0": 6, "cols": 1}, [("dx_slice", 1, 1)]),
    # ---- ... and the slice GEMM through each of its three doors
    ([48, 64, 1], 1, 70, 1, "slice", {"col0": 5, "cols": 40}, [("dX", "DTANH_SLICE", 64, "staged", 0, True)]),    # more than 32 columns
    ([24, 48, 3], 1, 70, 1, "slice", {"col0": 8, "cols": 5}, [("dX", "DTANH_SLICE", 64, "staged", 0, True)]),     # K % 32 != 0
    ([24, 1024, 1], 2, 130, 1, "slice", {"col0": 19, "cols": 5}, [("dX", "DTANH_SLICE", 64, "staged", 0, True)]),  # two nets x 1024 > 1264
    ([24, 1024, 1], 1, 37, 1, "slice", {"col0": 19, "cols": 5}, [("dx_slice", 16, 1)]),   # ... one net of the same width still fits
]


def _name(dims, nets, B, splits, form, kw):
    s = "x".join(str(d) for d in dims) + f"-n{nets}-B{B}-s{splits}-{form}"
    if form == "slice":
        s += f"-c{kw['col0']}+{kw['cols']}"
    return s + (f"-ldx{kw['ldx']}" if "ldx" in kw else "")


CASES = [Case(_name(dims, nets, B, splits, form, kw), list(dims), nets, B, splits, form, kw.get("col0", 0), kw.get("cols", 0),
              kw.get("ldx", ld(dims[0])), tuple(must)) for dims, nets, B, splits, form, kw, must in _TABLE]
CASE_BY_NAME = {c.name: c for c in CASES}
assert len(CASE_BY_NAME) == len(CASES)

# every launch tuple the table reaches: the CPU test holds the union of the rows' plans against this list.  (rows_per_block of
# k_skinny_bwd is a runtime argument of every instantiation: 32 and 64 are reached on <1, 1> only.)
LAUNCHES = [
    (_SB, 1, 1, 16), (_SB, 1, 2, 16), (_SB, 1, 4, 16), (_SB, 4, 1, 16), (_SB, 4, 2, 16), (_SB, 4, 4, 16), (_SB, 8, 1, 16), (_SB, 8, 2, 16),
    (_SB, 16, 1, 16), (_SB, 1, 1, 32), (_SB, 1, 1, 64),
    ("skinny_dw", 4), ("skinny_dw", 16), ("skinny_dx",),
    ("dW", "NONE", 64, "staged", 0, False), ("dW", "NONE", 64, "staged", 0, True), ("dW", "NONE", 64, "staged", "groups", False),
    ("dW", "NONE", 64, "staged", "groups", True), ("dW", "NONE", 64, "staged", "runs", True),
    ("dW", "NONE", 64, "dma", 0, False), ("dW", "NONE", 64, "dma", 0, True), ("dW", "NONE", 64, "dma", "runs", False),
    ("dW", "NONE", 128, "staged", "groups", False), ("dW", "NONE", 128, "dma", "groups", False),
    ("dX", "DELU", 64, "staged", 0, False), ("dX", "DELU", 64, "staged", 0, True), ("dX", "DELU", 64, "staged", "runs", True),
    ("dX", "DELU", 64, "staged", "groups", False),
    ("dX", "DELU", 64, "dma", 0, False), ("dX", "DELU", 64, "dma", "groups", False),
    ("dX", "DELU", 128, "staged", "groups", True), ("dX", "DELU", 128, "dma", "groups", False),
    ("dX", "NONE", 64, "staged", 0, True), ("dX", "NONE", 64, "staged", "runs", True), ("dX", "NONE", 64, "staged", "groups", True),
    ("dX", "DTANH_SLICE", 64, "staged", 0, True),
    ("dx_slice", 16, 1), ("dx_slice", 16, 2), ("dx_slice", 4, 1), ("dx_slice", 4, 2), ("dx_slice", 1, 1), ("dx_slice", 1, 2),
    ("reduce", False), ("reduce", True),
]

# rows on which pqlk_mlp_backward_layers is held against the single call: empty splits on either dW kernel, a non-fused skinny head
LAYERS_CASES = ["8x64x64x17-n2-B96-s8-gdx", "8x64x64x3-n1-B96-s8-gdx", "8x288x12-n2-B96-s8-gdx", "8x288x9-n2-B130-s64-g",
                "8x512x512x1-n2-B96-s8-g"]

# ---- pqlk_dpg_critic_backward
DpgCase = namedtuple("DpgCase", "name dims nets B col0 cols compact")
OWNERS = ("mixed", "ties", "net0", "net1")
DPG_CASES = [DpgCase(f"{'x'.join(map(str, dims))}-B{B}-c{col0}+{cols}", dims, 2, B, col0, cols, compact)
             for dims, compact in (([24, 128, 128, 1], True), ([24, 128, 128, 32, 1], True), ([24, 128, 128, 51], False))
             for col0, cols in ((8, 16), (19, 5)) for B in (1, 130, 257)]
DPG_BY_NAME = {c.name: c for c in DPG_CASES}


def as_case(c):
    """A DpgCase as the slice-only Case the shared inputs and references take."""
    return Case(c.name, list(c.dims), c.nets, c.B, 1, "slice", c.col0, c.cols, ld(c.dims[0]), ())


# ---------------------------------------------------------------- inputs
HVALS = np.array([2, 1, 0.5, 0, -0.5, -0.75, -1], dtype=F32)      # ELU' = 1, 1, 1, 1, 0.5, 0.25, 0
TVALS = np.array([0, 0.5, -0.5, 1, -1], dtype=F32)                # 1 - a^2 = 1, 0.75, 0.75, 0, 0
# seeds moved on where a stash patch of a handful of elements missed one of the three ELU' branches (design test, CPU)
STASH_SALT = {"8x512x512x1-n2-B3969-s8-g": 1, "24x128x128x32x1-B257-c8+16": 1, "24x128x128x32x1-B257-c19+5": 1}


def _seed(case, what, net=0, layer=0):
    return 7919 * sum((i + 1) * d for i, d in enumerate(case.dims)) + 131 * case.B + 17 * net + 3 * layer + 1000003 * what


def weights(case):
    """[net][layer] -> W (out, in) over {-1, 0, 1}."""
    dims = case.dims
    return [[(dd.integers((dims[l + 1], dims[l]), _seed(case, 1, n, l), 3) - 1).astype(F32) for l in range(len(dims) - 1)]
            for n in range(case.nets)]


def arena(case):
    """The parameter arena (include/pqlk.h layout): W (out, ld(in)) with zero pad columns, then ld(out) biases.  The backward
    reads no bias; they hold 1.0 so that one read by mistake moves a sum by a whole unit."""
    dims, ns = case.dims, net_stride(case.dims)
    out = np.zeros(ns * case.nets, dtype=F32)
    for n, net in enumerate(weights(case)):
        for l, w in enumerate(net):
            wo, bo = layer_offsets(dims, l)
            out[n * ns + wo: n * ns + bo].reshape(dims[l + 1], ld(dims[l]))[:, : dims[l]] = w
            out[n * ns + bo: n * ns + bo + dims[l + 1]] = 1.0
    return out


def hidden(case):
    """[net][layer] -> (B, dims[layer + 1]) stashed activations of the hidden layers, over HVALS."""
    salt = STASH_SALT.get(case.name, 0)
    return [[HVALS[dd.integers((case.B, case.dims[l + 1]), _seed(case, 2, n, l) + 977 * salt, len(HVALS))]
             for l in range(len(case.dims) - 2)] for n in range(case.nets)]


def stash(case, q=None):
    """The flat activation stash: hidden blocks with zero pad columns; the output layer's block, which pqlk_mlp_backward must
    not read, is NaN -- or holds q (nets, B) in column 0 for pqlk_dpg_critic_backward, which derives the owners from it."""
    dims, B = case.dims, case.B
    out = np.zeros(acts_floats(dims, case.nets, B), dtype=F32)
    for n, net in enumerate(hidden(case)):
        for l, h in enumerate(net):
            off, ldh = act_offset(dims, case.nets, B, n, l)
            out[off: off + B * ldh].reshape(B, ldh)[:, : dims[l + 1]] = h
    off, ldo = act_offset(dims, case.nets, B, 0, len(dims) - 2)
    out[off:] = np.nan
    if q is not None:
        blk = out[off:].reshape(case.nets, B, ldo)
        blk[:] = 0
        blk[:, :, 0] = q
    return out


def x_input(case):
    """(B, ldx): integers in [-2, 2], zero pad columns up to pqlk_ld(dims[0]), IN_ONE in the columns of a wider tile beyond."""
    out = np.zeros((case.B, case.ldx), dtype=F32)
    out[:, : case.dims[0]] = rc.ints((case.B, case.dims[0]), _seed(case, 3), -2, 2)
    out[:, ld(case.dims[0]):] = IN_ONE
    return out


def dy_input(case):
    """(nets, B, ld(out)): integers in [-2, 2], zero pad columns."""
    N = case.dims[-1]
    out = np.zeros((case.nets, case.B, ld(N)), dtype=F32)
    out[:, :, :N] = rc.ints((case.nets, case.B, N), _seed(case, 4), -2, 2)
    return out


def tanh_input(case):
    """(B, cols) over TVALS."""
    return TVALS[dd.integers((case.B, max(case.cols, 1)), _seed(case, 5), len(TVALS))]


def owner_input(case, pattern):
    """(B,) owner bytes (bit 0: net 0, bit 1: net 1) and a (2, B) integer Q block that says the same (minnet.h:22-27)."""
    B = case.B
    if pattern == "mixed":
        own = (dd.integers((B,), _seed(case, 6), 3) + 1).astype(np.uint8)       # 1, 2 or 3 (a tie)
    else:
        own = np.full(B, {"ties": 3, "net0": 1, "net1": 2}[pattern], dtype=np.uint8)
    q = np.zeros((2, B), dtype=F32)
    q[0] = rc.ints((B,), _seed(case, 7), -3, 3)
    q[1] = q[0] + np.where(own == 1, 1, np.where(own == 2, -1, 0)).astype(F32)
    return own, q


def dpg_dy_input(case, own):
    """(2, B, 32): integer dL/dQ in column 0, zero where the net does not own the row."""
    dy = dy_input(case)
    dy[0, :, 0] = np.where(own & 1, np.where(dy[0, :, 0] == 0, 1, dy[0, :, 0]), 0)
    dy[1, :, 0] = np.where(own & 2, np.where(dy[1, :, 0] == 0, -1, dy[1, :, 0]), 0)
    return dy


# ---------------------------------------------------------------- the float64 reference
def elu_prime(h):
    """ELU'(z) from the stashed h = ELU(z): 1 for h > 0, else h + 1."""
    return np.where(h > 0, 1.0, h.astype(F64) + 1.0)


def _chain(case, dy=None, measure=False, parts=None):
    """Walks the backward in float64: ({(net, layer): dW}, {(net, layer): db}, dx summed over the nets) and, with measure, one
    (name, sum_i |t_i| per output element, granularity g of the terms) per product of the chain.  parts: (W, H, x) of a case that
    brings its own weights, hidden activations and input (the TD family below)."""
    dims, B, L = case.dims, case.B, len(case.dims) - 1
    W, H, x = parts if parts is not None else (weights(case), hidden(case), x_input(case))
    x = x[:, : dims[0]].astype(F64)
    dy = dy_input(case) if dy is None else dy
    prods, dW, db, dx = [], {}, {}, np.zeros((B, dims[0]))
    dx_mass, dx_g = np.zeros((B, dims[0])), 0
    for n in range(case.nets):
        dz = dy[n][:, : dims[-1]].astype(F64)
        for l in range(L - 1, -1, -1):
            inp = x if l == 0 else H[n][l - 1].astype(F64)
            w = W[n][l].astype(F64)
            dW[n, l], db[n, l] = dz.T @ inp, dz.sum(0)
            v = dz @ w
            if measure:
                gz = _gran(dz)
                prods.append((f"dW{l} net {n}", np.abs(dz).T @ np.abs(inp), gz + _gran(inp)))
                prods.append((f"db{l} net {n}", np.abs(dz).sum(0), gz))
                if l > 0:
                    prods.append((f"dX{l} net {n}", np.abs(dz) @ np.abs(w), gz + _gran(w)))
                else:
                    dx_mass += np.abs(dz) @ np.abs(w)
                    dx_g = max(dx_g, gz + _gran(w))
            if l > 0:
                dz = v * elu_prime(H[n][l - 1])
                if measure:
                    prods.append((f"dX{l} * ELU' net {n}", np.abs(dz), _gran(dz)))
            else:
                dx += v
    if measure:
        prods.append(("dx", dx_mass, dx_g))
    return prods, dW, db, dx


@functools.lru_cache(maxsize=None)
def _reference(name, owner):
    case = CASE_BY_NAME[name] if name in CASE_BY_NAME else as_case(DPG_BY_NAME[name])
    dy = None if owner is None else dpg_dy_input(case, owner_input(case, owner)[0])
    _, dW, db, dx = _chain(case, dy)
    dims, ns = case.dims, net_stride(case.dims)
    grads = np.zeros(ns * case.nets, dtype=F64)
    for (n, l), g in dW.items():
        wo, bo = layer_offsets(dims, l)
        grads[n * ns + wo: n * ns + bo].reshape(dims[l + 1], ld(dims[l]))[:, : dims[l]] = g
        grads[n * ns + bo: n * ns + bo + dims[l + 1]] = db[n, l]
    out = {"grads": grads, "dx": dx}
    if case.form == "slice":
        a = tanh_input(case).astype(F64)
        out["slice"] = dx[:, case.col0: case.col0 + case.cols] * (1.0 - a * a)
    for v in out.values():
        v.setflags(write=False)
    return out


def reference(case, owner=None):
    """float64: "grads" (arena layout, zero pads), "dx" (B, dims[0]) summed over the nets, "slice" (B, cols) for a slice case.
    Computed once per case and shared; read-only.  owner: a pattern of OWNERS for the DPG cases (dy from dpg_dy_input)."""
    return _reference(case.name, owner)


def _gran(*arrays):
    """Smallest g with every element of every array a multiple of 2^-g."""
    for g in range(0, 48):
        if all(np.array_equal(np.round(a * 2.0 ** g), a * 2.0 ** g) for a in arrays):
            return g
    raise AssertionError("not dyadic")


def exactness_bits(case, owner=None):
    """Worst log2(sum_i |t_i| 2^g) over every output element of every product of the chain, g the granularity of the product's
    terms (the sum of its operands' granularities); the elementwise ELU' and tanh' factors count as one-term products.  At most
    24 means every partial sum of every order is exact in fp32."""
    dy = None if owner is None else dpg_dy_input(case, owner_input(case, owner)[0])
    prods, _, _, dx = _chain(case, dy, measure=True)
    worst = 0.0
    for _, mass, g in prods:
        if mass.size and mass.max() > 0:
            worst = max(worst, float(np.log2(mass.max() * 2.0 ** g)))
    if case.form == "slice":
        a = tanh_input(case).astype(F64)
        s = dx[:, case.col0: case.col0 + case.cols]
        out = np.abs(s * (1.0 - a * a))
        if out.max() > 0:
            worst = max(worst, float(np.log2(out.max() * 2.0 ** (_gran(s) + 2))))
    return worst


# ---------------------------------------------------------------- checks (numpy in, AssertionError out)
def _first_bad(got, want):
    bad = np.argwhere(~(got.astype(F64) == want))
    return bad


def check_grads(grads, case, ref=None, what=""):
    """grads: the whole gradient arena as the kernel left it.  Every element equals the float64 reference, pads are zero."""
    want = (ref or reference(case))["grads"]
    assert grads.shape == want.shape, what
    bad = _first_bad(grads, want)
    assert bad.size == 0, (f"{what}: {len(bad)} arena elements differ from the reference, first at {int(bad[0][0])}: "
                           f"{grads[bad[0][0]]} != {want[bad[0][0]]}")


def check_dx_full(dx, before, case, ref=None, what=""):
    """dx, before: (B, ld_dx) after and before the call.  Columns below dims[0] equal the reference, the pad up to pqlk_ld(dims[0])
    is zero, columns beyond are untouched."""
    want = (ref or reference(case))["dx"]
    K, ldk = case.dims[0], ld(case.dims[0])
    bad = _first_bad(dx[:, :K], want)
    assert bad.size == 0, f"{what}: {len(bad)} elements of dx differ, first at (row, col) {tuple(bad[0])}: {dx[tuple(bad[0])]} != {want[tuple(bad[0])]}"
    assert np.all(dx[:, K:ldk] == 0), f"{what}: pad columns of dx not zero"
    assert np.array_equal(dx[:, ldk:].view(np.uint32), before[:, ldk:].view(np.uint32)), f"{what}: columns past pqlk_ld(dims[0]) written"


def check_dx_slice(dx, before, case, ref=None, what="", rest="untouched"):
    """dx, before: (B, ld_dx).  The `cols` slice columns equal the reference; every other element still holds what it held
    (rest = "untouched") or is zero (rest = "zero": the compact path of pqlk_dpg_critic_backward)."""
    want = (ref or reference(case))["slice"]
    bad = _first_bad(dx[:, : case.cols], want)
    assert bad.size == 0, f"{what}: {len(bad)} slice elements differ, first at (row, col) {tuple(bad[0])}: {dx[tuple(bad[0])]} != {want[tuple(bad[0])]}"
    if rest == "zero":
        assert np.all(dx[:, case.cols:] == 0), f"{what}: columns past the slice not zero"
    else:
        assert np.array_equal(dx[:, case.cols:].view(np.uint32), before[:, case.cols:].view(np.uint32)), f"{what}: columns past the slice written"


def bits_equal(a, b):
    return a.shape == b.shape and bool(np.all(a.view(np.uint32) == b.view(np.uint32)))


def dx_geometry(case):
    """(ld_dx, ld_tanh) the GPU test uses: 32 spare columns behind the written ones; a tanh matrix with an odd row stride."""
    if case.form == "slice":
        return ld(case.cols) + 32, case.cols + 1
    return ld(case.dims[0]) + 32, 0


# ---------------------------------------------------------------- a plain numpy backward, for the checks' own tests
FAULTS = ("last_row", "stage", "no_elu", "stale_slab", "slice_shift", "pad", "nets_not_summed")


def model_backward(case, fault=None):
    """What a backward leaves in (grads arena, dx matrix with POISON where nothing is written), computed by plain numpy the way
    the kernels split the work (split slabs summed, nets summed), with one fault planted:
      last_row         the last batch row is dropped from every product
      stage            one 16-deep reduction stage is dropped: rows [0, 16) of every dW, the first 16 of layer 0's dX reduction
      no_elu           ELU' is taken as 1 for h <= 0
      stale_slab       the slab of every empty split holds POISON instead of zeros when the slabs are summed
      slice_shift      the slice starts at col0 & ~3
      pad              one pad column of the first layer's dW is not zero
      nets_not_summed  the input gradient is the last net's alone"""
    dims, B, L, nets = case.dims, case.B, len(case.dims) - 1, case.nets
    W, H = weights(case), hidden(case)
    x = x_input(case)[:, : dims[0]].astype(F64)
    dy = dy_input(case)
    rows = B - 1 if fault == "last_row" else B
    ns = net_stride(dims)
    grads = np.zeros(ns * nets, dtype=F64)
    dx = np.zeros((B, dims[0]))
    rps = rows_per_split(B, case.splits)
    for n in range(nets):
        dz = dy[n][:rows, : dims[-1]].astype(F64)
        for l in range(L - 1, -1, -1):
            inp = (x if l == 0 else H[n][l - 1].astype(F64))[:rows]
            lo = 16 if fault == "stage" else 0
            wo, bo = layer_offsets(dims, l)
            gw = grads[n * ns + wo: n * ns + bo].reshape(dims[l + 1], ld(dims[l]))
            gb = grads[n * ns + bo: n * ns + bo + ld(dims[l + 1])]
            for s in range(case.splits):           # split slabs, summed in split order
                a, b = max(s * rps, lo), min(rows, (s + 1) * rps)
                if s * rps >= B and fault == "stale_slab":
                    gw += POISON; gb += POISON
                elif a < b:
                    gw[:, : dims[l]] += dz[a:b].T @ inp[a:b]
                    gb[: dims[l + 1]] += dz[a:b].sum(0)
            w = W[n][l].astype(F64)
            if l > 0:
                f = elu_prime(H[n][l - 1][:rows])
                dz = (dz @ w) * (1.0 if fault == "no_elu" else f)
            else:
                k0 = 16 if fault == "stage" else 0
                v = dz[:, k0:] @ w[k0:]
                if fault == "nets_not_summed":
                    dx[:rows] = v
                else:
                    dx[:rows] += v
    if fault == "pad":
        wo, _ = layer_offsets(dims, 0)
        grads[wo + ld(dims[0]) - 1] = 2.0 ** -20
        assert ld(dims[0]) > dims[0]
    ld_dx, _ = dx_geometry(case)
    out = np.full((B, ld_dx), POISON, dtype=F32)
    if case.form == "slice":
        a = tanh_input(case).astype(F64)
        c0 = case.col0 & ~3 if fault == "slice_shift" else case.col0
        out[:rows, : case.cols] = (dx[:, c0: c0 + case.cols] * (1.0 - a * a))[:rows]
    else:
        out[:rows, : dims[0]] = dx[:rows]
        out[:rows, dims[0]: ld(dims[0])] = 0
    return grads.astype(F32), out


# ================================================================ the TD family
# pqlk_mlp_backward_td (k_skinny_bwd<1, CH, true>), pqlk_mlp_forward_td + pqlk_mlp_backward_td_tail (fused_head's TD part in
# fused.h), pqlk_mlp_backward_layers with the TD inputs, the squared-norm partials of k_reduce_slabs and the prenorm / loss fold
# of pqlk_adamw_polyak_fused: the scalar twin critic's step.  tests/test_td_paths_gpu.py runs the cases below, and
# tests/test_backward_cases_cpu.py holds this mirror against the library and the data against the conditions the `==` rest on.
#
# TD inputs: Q and Q' integers in [-2, 2], gamma^n = 0.5, r a multiple of 0.5, done in {0, 1} (one case per path: 0.5 on some
# rows), so y = r + ((1 - d) gamma^n) min(Q1', Q2'), dq = Q - y and dq^2 are small dyadic rationals.  2.0f / (float)B is exact
# for B a power of two, and a gradient element is then exactly summable under the same condition as above (`td_exactness_bits`).
# For any other B the head's dL/dQ is rounded once, dy = float32(2) / float32(B) * dq, and the checks are bit equality with
# pqlk_mlp_backward fed that dy, plus the bound `head_sum_bound` where the forward path sums the head in other groups.
from types import SimpleNamespace

GAMMA_N = 0.5
FUSED_NW = 8                              # pqlk_common.h


# ---------------------------------------------------------------- mirror: the fused forward (gemm.hip)
def fused_lds_bytes(dims, bld, R):
    """gemm.hip, fused_lds_bytes."""
    return max((32 * R * bld + (len(dims) - 2) * (bld - 4)) * 4, 8 * R * 16 * 64 * 4)


def buf_ld(dims):
    """gemm.hip, fusable: the row stride of the LDS activation tile, max(ld(in), hidden widths) + 4; 0 when not fusable."""
    if len(dims) < 3 or any(d % 32 != 0 or d > 1024 for d in dims[1:-1]):
        return 0
    bld = max([ld(dims[0])] + list(dims[1:-1])) + 4
    return bld if fused_lds_bytes(dims, bld, 1) <= LDS_BYTES else 0


def head_fusable(dims):
    """gemm.hip, head_fusable."""
    return len(dims) >= 3 and dims[-1] <= 32 and dims[-2] % 32 == 0


def fused_rows(dims, nets, B):
    """gemm.hip, fused_rows (PQLK_FUSED_ROWS unset): R, the 32-row tiles per block of k_mlp_fwd_fused."""
    bld = buf_ld(dims)
    wide = any(d > 512 for d in dims[1:-1])
    if not wide and fused_lds_bytes(dims, bld, 2) <= LDS_BYTES:
        b1, b2 = cdiv(B, 32) * nets, cdiv(B, 64) * nets
        if 2.0 * cdiv(b2, 256) <= 1.15 * cdiv(b1, 256):
            return 2
    return 1


def fwd_kernel(dims, nets, B):
    """gemm.hip, launch_fused_hidden: (R, TM) of k_mlp_fwd_fused<R, TM>."""
    return fused_rows(dims, nets, B), (4 if any(d > 512 for d in dims[1:-1]) else 2)


def td_forward_tiles(dims, nets, B):
    """gemm.hip, td_forward_tiles (PQLK_NO_FUSED_HEAD unset)."""
    bld = buf_ld(dims)
    if B <= 0 or not bld or not head_fusable(dims):
        return 0
    if nets != 2 or dims[-1] != 1 or not head_is_fused(dims):
        return 0
    if bld - dims[-2] < 256 or (len(dims) - 2) * (bld - 4) < 128:
        return 0
    return cdiv(B, 32 * fused_rows(dims, nets, B))


def td_forward_loss_parts(dims, nets, B):
    """gemm.hip, pqlk_td_forward_loss_parts."""
    return td_forward_tiles(dims, nets, B) * nets


def td_head_loss_parts(dims, nets, B):
    """gemm.hip, pqlk_td_head_loss_parts."""
    if B <= 0 or nets != 2 or dims[-1] != 1 or not head_is_fused(dims):
        return 0
    return skinny_bwd_blocks(B, nets) * nets


# ---------------------------------------------------------------- the tables
TdCase = namedtuple("TdCase", "name dims B splits path data")
# path "bwd": the stash is an input (pqlk_mlp_backward_td, pqlk_mlp_backward_layers + TD, pqlk_mlp_backward_norm)
# path "fwd": the forward is real (pqlk_mlp_forward_td + pqlk_mlp_backward_td_tail) on the exactly evaluable network below
# data "std" | "half" (done = 0.5 on some rows) | "int" (B = 8, dq a multiple of 4: integer gradients) | "head_only" ("int"
# with an all-dead last hidden layer: only the head's dW / db are non-zero)
_TD_BWD = [
    # CH = 1, tiny dims: a lone row, 15 | 16 | 17 on 16-row blocks, the 16 | 32 and 32 | 64 switches of skinny_bwd_rows with a ragged
    # last block behind each, and the power of two on 32-row blocks
    ([8, 32, 1], 1, "std"), ([8, 32, 1], 15, "std"), ([8, 32, 1], 16, "std"), ([8, 32, 1], 17, "std"),
    ([8, 32, 1], 4097, "std"),
    ([8, 32, 1], B_ROWS32 - 1, "std"), ([8, 32, 1], B_ROWS32, "std"), ([8, 32, 1], 8192, "std"),
    ([8, 32, 1], B_ROWS64 - 1, "std"), ([8, 32, 1], B_ROWS64, "std"),
    # CH = 2 (ld 288, 512) and CH = 4 (ld 1024)
    ([8, 288, 1], 16, "std"), ([8, 288, 1], 33, "std"), ([8, 512, 1], 32, "std"),
    ([8, 1024, 1], 16, "std"), ([8, 1024, 1], 65, "std"),
    # hidden layers below the head
    ([8, 64, 32, 1], 128, "half"), ([8, 64, 32, 1], 95, "std"), ([8, 64, 288, 1], 64, "std"),
    # integer gradients: the squared-norm partials
    ([8, 64, 32, 1], 8, "int"), ([8, 64, 32, 1], 8, "head_only"), ([8, 32, 288, 1], 8, "int"),
]
_TD_FWD = [
    # R = 1, Kh = 32: a lone row, 31 | 32 | 33, two and three tiles; R = 2 at its first batch (the last 64-row tile holds one row)
    # and at 8192
    ([8, 288, 32, 1], 1, "std"), ([8, 288, 32, 1], 31, "std"), ([8, 288, 32, 1], 32, "std"), ([8, 288, 32, 1], 33, "std"),
    ([8, 288, 32, 1], 65, "std"), ([8, 288, 32, 1], 95, "std"), ([8, 288, 32, 1], 4097, "std"), ([8, 288, 32, 1], 8192, "std"),
    ([8, 288, 32, 1], 8, "int"),
    # Kh = 256; Kh = 288 (two chunks of the quad loop) under TM = 4 and under TM = 2; an input wider than every hidden layer
    ([8, 512, 256, 1], 32, "std"), ([8, 512, 256, 1], 33, "std"),
    ([8, 544, 288, 1], 64, "std"), ([8, 544, 288, 1], 33, "std"),
    ([540, 32, 288, 1], 16, "std"),
    ([300, 64, 64, 1], 32, "half"), ([300, 64, 64, 1], 33, "std"),
]
TD_TAKEN, TD_REFUSED = [8, 288, 32, 1], [8, 256, 32, 1]     # buf_ld - Kh = 260 | 228: the eligibility edge of the forward path


def _td_name(dims, B, path, data):
    return "x".join(str(d) for d in dims) + f"-B{B}-{path}" + ("" if data == "std" else f"-{data}")


TD_CASES = [TdCase(_td_name(dims, B, path, data), list(dims), B, default_splits(B), path, data)
            for path, table in (("bwd", _TD_BWD), ("fwd", _TD_FWD)) for dims, B, data in table]
TD_BY_NAME = {c.name: c for c in TD_CASES}
assert len(TD_BY_NAME) == len(TD_CASES)
TD_BWD_NAMES = [c.name for c in TD_CASES if c.path == "bwd"]
TD_FWD_NAMES = [c.name for c in TD_CASES if c.path == "fwd"]
# the kernel instances the tables must reach (the CPU test holds the union against these)
TD_BWD_INSTANCES = [(1, 16), (1, 32), (1, 64), (2, 16), (4, 16)]        # (CH, rows per block) of k_skinny_bwd<1, CH, true>
TD_FWD_INSTANCES = [(1, 2), (2, 2), (1, 4)]                              # (R, TM) of k_mlp_fwd_fused<R, TM>
# rows on which the buckets of pqlk_mlp_backward_layers are held against the single pqlk_mlp_backward_td call
TD_LAYERS_NAMES = ["8x32x1-B17-bwd", "8x64x32x1-B128-bwd-half", "8x64x32x1-B95-bwd", "8x64x288x1-B64-bwd"]
# rows whose squared-norm partials are summed: integer gradients (bwd), dyadic ones with exact squares (fwd)
TD_NORM_BWD_NAMES = ["8x64x32x1-B8-bwd-int", "8x64x32x1-B8-bwd-head_only", "8x32x288x1-B8-bwd-int"]
TD_NORM_FWD_NAMES = ["8x288x32x1-B8-fwd-int"]
NORM_PLAIN_DIMS = [8, 512, 16]            # a non-fused head (16 outputs on K = 512) for pqlk_mlp_backward_norm


def is_pow2(B):
    return B & (B - 1) == 0


def td_instance(tc):
    """The kernel instance a case reaches: (CH, rows per block) on path "bwd", (R, TM) on path "fwd"."""
    if tc.path == "bwd":
        return skinny_bwd_ch(ld(tc.dims[-2])), skinny_bwd_rows(tc.B, 2)
    return fwd_kernel(tc.dims, 2, tc.B)


def td_as_case(tc):
    return Case(tc.name, list(tc.dims), 2, tc.B, tc.splits, "g", 0, 0, ld(tc.dims[0]), ())


# ---------------------------------------------------------------- an exactly evaluable network (path "fwd")
GATE = 48                                 # x[:, 0] on the rows whose gated units of layer 0 are dead


def exact_network(case, twin=False):
    """(W, bias, x): weights over {-1, 0, 1} with one or two non-zeros per hidden unit, integer biases, integer x, such that
    every hidden pre-activation is an integer >= 0 or <= -32 whatever the row: ELU gives z itself or (__expf(z) - 1.f = ) -1
    exactly, ELU' 1 or 0.  Units j % 4 == 3 are dead on every row (bias below -32 minus the largest sum), units j % 4 == 2 of
    layer 0 are dead on the rows with x[:, 0] = GATE (rows b % 4 == 1) and alive elsewhere, the others are alive: the bias lifts
    the smallest possible sum to 0.  The head has dims[-2] / 8 non-zero weights and a small integer bias.  twin: both nets hold
    net 0's weights and the head biases differ by 4, so that Q2 = Q1 + 4 on every row (data "int": dq a multiple of 4 on both)."""
    dims, B, L = case.dims, case.B, len(case.dims) - 1
    x = x_input(case)
    x[:, 0] = np.where(np.arange(B) % 4 == 1, GATE, 0)
    Ws, bs = [], []
    for net in range(case.nets):
        n = 0 if twin else net
        lo, hi = -2, 2                                             # range of the layer's inputs
        Wn, bn = [], []
        for l in range(L - 1):
            N, K = dims[l + 1], dims[l]
            first = 1 if l == 0 else 0                             # column 0 of x is the gate
            k1 = dd.integers((N,), _seed(case, 11, n, l), K - first) + first
            k2 = dd.integers((N,), _seed(case, 12, n, l), K - first) + first
            sg = dd.integers((N, 2), _seed(case, 13, n, l), 2) * 2 - 1
            two = (dd.integers((N,), _seed(case, 14, n, l), 2) == 1) & (k1 != k2)
            W = np.zeros((N, K), dtype=F32)
            W[np.arange(N), k1] = sg[:, 0]
            W[np.arange(N)[two], k2[two]] = sg[two, 1]
            pos, neg = (W > 0).sum(1), (W < 0).sum(1)
            smin, smax = pos * lo - neg * hi, pos * hi - neg * lo
            dead = np.arange(N) % 4 == 3
            b = np.where(dead, -32 - smax, -smin).astype(F32)
            if l == 0:
                gated = np.arange(N) % 4 == 2
                assert (smax - smin)[gated].max() <= GATE - 32
                W[gated, 0] = -1
            Wn.append(W); bn.append(b)
            lo, hi = -1, int((smax - smin)[~dead].max())
        Kh = dims[L - 1]
        W = np.zeros((1, Kh), dtype=F32)
        at = 8 * np.arange(Kh // 8) + dd.integers((Kh // 8,), _seed(case, 15, n), 8)
        W[0, at] = dd.integers((Kh // 8,), _seed(case, 16, n), 2) * 2 - 1
        Wn.append(W); bn.append(np.array([4 * net if twin else net - 1], dtype=F32))
        Ws.append(Wn); bs.append(bn)
    return Ws, bs, x


def exact_forward(case, W, bias, x):
    """float64: ([net][layer] hidden pre-activations z, [net][layer] hidden activations h as float32, Q (nets, B))."""
    dims, L = case.dims, len(case.dims) - 1
    Z, H, Q = [], [], np.zeros((case.nets, case.B))
    for n in range(case.nets):
        a, zn, hn = x[:, : dims[0]].astype(F64), [], []
        for l in range(L - 1):
            z = a @ W[n][l].astype(F64).T + bias[n][l].astype(F64)
            a = np.where(z >= 0, z, -1.0)
            zn.append(z); hn.append(a.astype(F32))
        Z.append(zn); H.append(hn)
        Q[n] = (a @ W[n][L - 1].astype(F64).T + bias[n][L - 1].astype(F64))[:, 0]
    return Z, H, Q


# ---------------------------------------------------------------- TD inputs and the problem of one case
HINT = np.array([2, 1, 0, -1], dtype=F32)                          # integer activations: ELU' = 1, 1, 1, 0


def _td_targets(case, data):
    """(qt (2, B), rew, done): row b % 3 == 0 has net 1 as the minimum, 1 is a tie, 2 has net 0."""
    B, pat = case.B, np.arange(case.B) % 3
    qt = np.zeros((2, B))
    qt[0] = rc.ints((B,), _seed(case, 21), -1, 1)
    qt[1] = qt[0] + np.where(pat == 0, -1, np.where(pat == 1, 0, 1))
    rew = rc.ints((B,), _seed(case, 22), -4, 4).astype(F64) * 0.5
    done = (dd.integers((B,), _seed(case, 23), 4) == 0).astype(F64)
    if data == "half":
        done[np.arange(B) % 5 == 2] = 0.5
    return qt, rew, done


@functools.lru_cache(maxsize=6)
def td_problem(name):
    """Everything of one TD case, float64 unless said: case, W, bias (fwd; None on path bwd, whose arena holds 1.0), H (float32),
    x (float32), q, qt (2, B), rew, done, y, dq (2, B), dy (2, B, 32) float32 = float32(2) / float32(B) * dq."""
    tc = TD_BY_NAME[name]
    case = td_as_case(tc)
    B, L = tc.B, len(tc.dims) - 1
    qt, rew, done = _td_targets(case, tc.data)
    cmin = ((1.0 - done) * GAMMA_N) * np.minimum(qt[0], qt[1])
    if tc.path == "fwd":
        W, bias, x = exact_network(case, twin=tc.data == "int")
        _, H, q = exact_forward(case, W, bias, x)
        if tc.data == "int":                                       # Q2 = Q1 + 4: dq = 4 k on net 0, 4 k + 4 on net 1
            assert B == 8 and np.array_equal(q[1], q[0] + 4)
            rew = q[0] - 4.0 * rc.ints((B,), _seed(case, 25), -1, 1) - cmin
    else:
        W, bias, x = weights(case), None, x_input(case)
        if tc.data in ("int", "head_only"):
            H = [[HINT[dd.integers((B, tc.dims[l + 1]), _seed(case, 2, n, l), len(HINT))] for l in range(L - 1)] for n in range(2)]
            if tc.data == "head_only":
                for n in range(2):
                    H[n][L - 2][:] = -1
            assert B == 8                                          # dq a multiple of B / 2 = 4 on both nets: Q1 - Q2 in {0, +-4}
            q = np.zeros((2, B))
            q[0] = rc.ints((B,), _seed(case, 24), -2, 2)
            q[1] = np.where(np.abs(q[0]) == 2, -q[0], q[0])
            rew = q[0] - 4.0 * rc.ints((B,), _seed(case, 25), -1, 1) - cmin
        else:
            H = hidden(case)
            q = rc.ints((2, B), _seed(case, 24), -2, 2).astype(F64)
    y = rew + cmin
    dq = q - y[None, :]
    dy = np.zeros((2, B, 32), dtype=F32)
    dy[:, :, 0] = (F32(2) / F32(B)) * dq.astype(F32)
    assert np.array_equal(dq.astype(F32).astype(F64), dq)
    p = SimpleNamespace(tc=tc, case=case, W=W, bias=bias, H=H, x=x, q=q, qt=qt, rew=rew, done=done, y=y, dq=dq, dy=dy)
    for v in [x, q, qt, rew, done, y, dq, dy] + [h for net in H for h in net]:
        v.setflags(write=False)
    return p


def td_arena(p):
    """The parameter arena of a TD case: as `arena`, with the network's own biases on path "fwd"."""
    out = arena(p.case) if p.bias is None else np.zeros(net_stride(p.case.dims) * 2, dtype=F32)
    if p.bias is not None:
        dims, ns = p.case.dims, net_stride(p.case.dims)
        for n in range(2):
            for l, w in enumerate(p.W[n]):
                wo, bo = layer_offsets(dims, l)
                out[n * ns + wo: n * ns + bo].reshape(dims[l + 1], ld(dims[l]))[:, : dims[l]] = w
                out[n * ns + bo: n * ns + bo + dims[l + 1]] = p.bias[n][l]
    return out


def td_stash(p, last_hidden=True):
    """The online stash: hidden blocks with zero pads, Q in column 0 of the output block and zeros beside it.  On path "fwd" this
    is what the forward must leave; last_hidden = False leaves the last hidden layer's block NaN (pqlk_mlp_forward_td)."""
    dims, B = p.case.dims, p.case.B
    out = np.zeros(acts_floats(dims, 2, B), dtype=F32)
    for n in range(2):
        for l, h in enumerate(p.H[n]):
            off, ldh = act_offset(dims, 2, B, n, l)
            blk = out[off: off + B * ldh].reshape(B, ldh)
            blk[:, : dims[l + 1]] = h
            if l == len(dims) - 3 and not last_hidden:
                blk[:] = np.nan
    off, ldo = act_offset(dims, 2, B, 0, len(dims) - 2)
    out[off:].reshape(2, B, ldo)[:, :, 0] = p.q
    return out


def td_target_stash(p):
    """The target critic's stash: NaN but for Q' in column 0 of the output block -- nothing else of it may be read."""
    dims, B = p.case.dims, p.case.B
    out = np.full(acts_floats(dims, 2, B), np.nan, dtype=F32)
    off, ldo = act_offset(dims, 2, B, 0, len(dims) - 2)
    out[off:].reshape(2, B, ldo)[:, :, 0] = p.qt
    return out


def _arena_of(dims, dW, db):
    ns = net_stride(dims)
    grads = np.zeros(ns * 2, dtype=F64)
    for (n, l), g in dW.items():
        wo, bo = layer_offsets(dims, l)
        grads[n * ns + wo: n * ns + bo].reshape(dims[l + 1], ld(dims[l]))[:, : dims[l]] = g
        grads[n * ns + bo: n * ns + bo + dims[l + 1]] = db[n, l]
    return grads


@functools.lru_cache(maxsize=6)
def td_reference(name):
    """float64, read-only: "grads" (arena layout) of the chain fed p.dy, "head_mass" (arena layout) sum_b |dy_b h_bk| on the
    head's elements (0 elsewhere), "sumsq" sum g^2."""
    p = td_problem(name)
    dims, L = p.case.dims, len(p.case.dims) - 1
    _, dW, db, _ = _chain(p.case, p.dy, parts=(p.W, p.H, p.x))
    grads = _arena_of(dims, dW, db)
    ady = np.abs(p.dy[:, :, :1].astype(F64))
    mass = _arena_of(dims, {(n, L - 1): ady[n].T @ np.abs(p.H[n][L - 2].astype(F64)) for n in range(2)},
                     {(n, L - 1): ady[n].sum(0) for n in range(2)})
    out = {"grads": grads, "head_mass": mass, "sumsq": float((grads * grads).sum())}
    grads.setflags(write=False); mass.setflags(write=False)
    return out


def head_range(dims, net):
    """[start, end) of a net's head block (W row, then the bias block) in the arena."""
    ns = net_stride(dims)
    wo, _ = layer_offsets(dims, len(dims) - 2)
    return net * ns + wo, (net + 1) * ns


def head_sum_bound(p, ref):
    """(B + 8) 2^-24 sum_b |dy_b h_bk| per arena element: the standard bound on an fp32 sum of B products taken in any order
    against its float64 value (each product and each of at most B - 1 additions rounds once; 8 spare roundings for the fold of
    partials)."""
    return (p.case.B + 8) * 2.0 ** -24 * ref["head_mass"]


def td_loss_parts(name):
    """float64 sum of dq^2 per (row block, net), in the order the kernels leave them: [block][net].  Row blocks of
    skinny_bwd_rows(B, 2) rows on path "bwd", of 32 R rows on path "fwd"."""
    p = td_problem(name)
    rows = skinny_bwd_rows(p.case.B, 2) if p.tc.path == "bwd" else 32 * fused_rows(p.case.dims, 2, p.case.B)
    sq = p.dq * p.dq
    return np.array([sq[n, r0: r0 + rows].sum() for r0 in range(0, p.case.B, rows) for n in range(2)])


def td_exactness_bits(name):
    """`exactness_bits` of the chain fed p.dy, and of the loss partials: log2 of the largest partial times 2^(2 g), g the
    granularity of dq."""
    p = td_problem(name)
    prods, _, _, _ = _chain(p.case, p.dy, measure=True, parts=(p.W, p.H, p.x))
    worst = 0.0
    for _, mass, g in prods:
        if mass.size and mass.max() > 0:
            worst = max(worst, float(np.log2(mass.max() * 2.0 ** g)))
    parts = td_loss_parts(name)
    return worst, float(np.log2(max(parts.max(), 2.0 ** -40) * 4.0 ** _gran(p.dq)))


def sumsq_bits(grads):
    """log2 of sum (g 2^k)^2, k the granularity of the gradient: at most 24 means every g^2 and every partial sum of them in any
    order or grouping is exact in fp32.  Returns (bits, k)."""
    k = _gran(grads)
    return float(np.log2(max(float(((grads * 2.0 ** k) ** 2).sum()), 1.0))), k


def norm_plain_case():
    """pqlk_mlp_backward_norm on a non-fused head: 16 outputs on K = 512, integer stash, integer dy."""
    return Case("8x512x16-n2-B16-norm", list(NORM_PLAIN_DIMS), 2, 16, 1, "g", 0, 0, 32, ())


def norm_plain_parts(case):
    """(W, H, x) with integer activations for `norm_plain_case`."""
    H = [[HINT[dd.integers((case.B, case.dims[l + 1]), _seed(case, 2, n, l), len(HINT))] for l in range(len(case.dims) - 2)]
         for n in range(case.nets)]
    return weights(case), H, x_input(case)


def norm_plain_stash(case):
    _, H, _ = norm_plain_parts(case)
    out = np.zeros(acts_floats(case.dims, case.nets, case.B), dtype=F32)
    for n in range(case.nets):
        for l, h in enumerate(H[n]):
            off, ldh = act_offset(case.dims, case.nets, case.B, n, l)
            out[off: off + case.B * ldh].reshape(case.B, ldh)[:, : case.dims[l + 1]] = h
    off, _ = act_offset(case.dims, case.nets, case.B, 0, len(case.dims) - 2)
    out[off:] = np.nan
    return out


def norm_plain_reference(case):
    _, dW, db, _ = _chain(case, dy_input(case), parts=norm_plain_parts(case))
    return _arena_of(case.dims, dW, db)


# ---------------------------------------------------------------- operand order (B = 1, values that are no dyadic rationals)
# found by search: with these, forming (1 - d) (gamma^n min Q') instead of ((1 - d) gamma^n) min Q', or contracting the product
# and the addition of r into one fma, moves the last bit of the head's db for the Q of either path (the CPU test holds that)
ORDER = dict(gamma_n=0.99, rew=-0.7488293647766113, done=0.16398358345031738, qt=(-1.7941311597824097, -2.2908599376678467),
             q=(-1.8804951906204224, -0.17266710102558136))
ORDER_BWD_NAME, ORDER_FWD_NAME = "8x32x1-B1-bwd", "8x288x32x1-B1-fwd"


def td_db_in_order(q, order="documented"):
    """The head's db at B = 1 (2.0f / B = 2) for Q = q in numpy float32: 2 (Q - (r + ((1 - d) gamma^n) min(Q1', Q2'))) in that
    order, or in one of the two orders it must not be taken in."""
    r, d, g = F32(ORDER["rew"]), F32(ORDER["done"]), F32(ORDER["gamma_n"])
    t = np.minimum(F32(ORDER["qt"][0]), F32(ORDER["qt"][1]))
    if order == "documented":
        y = F32(r + F32(F32(F32(1) - d) * g) * t)
    elif order == "gamma_first":
        y = F32(r + F32(F32(1) - d) * F32(g * t))
    else:                                                          # "fma": the product is not rounded before r is added
        y = F32(F64(r) + F64(F32(F32(F32(1) - d) * g)) * F64(t))
    return F32(F32(2) * F32(F32(q) - y))


def order_problem(name):
    """The one-row problem of `name` with the TD inputs of ORDER (and, on path "bwd", its Q)."""
    p = td_problem(name)
    q = p.q if p.tc.path == "fwd" else np.array([[F32(v)] for v in ORDER["q"]], dtype=F64)
    qt = np.array([[F32(v)] for v in ORDER["qt"]], dtype=F64)
    rew, done = np.array([F32(ORDER["rew"])], dtype=F64), np.array([F32(ORDER["done"])], dtype=F64)
    return SimpleNamespace(tc=p.tc, case=p.case, W=p.W, bias=p.bias, H=p.H, x=p.x, q=q, qt=qt, rew=rew, done=done, dq=p.dq, dy=p.dy)
