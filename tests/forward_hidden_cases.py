"""Cases, inputs, references and checks for tests/test_forward_hidden_gpu.py (plain numpy, no GPU, no library).

The hidden layers of pqlk_mlp_forward run either inside k_mlp_fwd_fused<R, TM> (fused.h: one launch, activations of a row tile
resident in LDS, a ring of weight quads per wave, the stash written from the NEXT layer's main loop or from the epilogue) or as one
k_gemm<FWD, EPI_ELU> launch per layer (gemm.hip: two tile sizes, three tile orders).  The stashed hidden blocks are what the
backward reads for ELU' and dW.  `ring`, `waves`, `stash_route`, `defer_walk`, `block_map` and `hidden_gemms` restate, per case and layer, which branch of either kernel a shape
reaches; the dispatch itself (fusable, fused_rows, fused_wide, gemm_tile, gemm_plan) is the mirror the head and backward cases
already hold against the library.  tests/test_forward_hidden_cases_cpu.py holds the table against the explicit list COVERAGE.

Two data designs per case:
  exact  integer inputs, up to eight integer weights per hidden unit, biases that make every pre-activation an integer >= 0 or
         <= -32: ELU is z or exactly -1 in fp32 (__expf(-32) - 1.f == -1.f), every partial sum of every order is an integer below
         2^24, so each hidden block must equal the float64 activations BIT FOR BIT.  In every 32-unit output tile every reduction
         step of 8 meets a non-zero weight of a unit that is alive on every row: a dropped or misplaced step moves an integer.
  dense  the weights of forward_head_cases.weights, x uniform on +-2: layer by layer from the kernel's own previous block,
         |got - elu64(z)| <= bound(h_prev, W, b, k_pad) + [z < 0] (2^-23 + 2^-24), z the float64 pre-activation.  2^-23 is the
         absolute error of __expf that gemm.hip:156 states, 2^-24 the rounding of the subtraction; ELU is 1-Lipschitz.

Columns [dims[0], ldx) of x are IGNORED on the fused path (include/pqlk.h) and hold GARBAGE = 1e30 in every fused case.  The arena's
pad columns are zero, so a finite value there meets a zero weight and changes no bit even unmasked (1e30 * 0 = 0): only a NaN shows
whether the mask inside the last quad (fused.h, `if (c + 3 >= w)`) is there.  The GPU test therefore runs its second call with NaN
in the same columns and asks for the same bits; `model_hidden(..., garbage=nan)` is the matching fault model.

Source lines cited below are those of pql_amd/csrc at the commit that added this file."""
import functools
from collections import namedtuple

import numpy as np

import backward_cases as bc
import detdata as dd
import forward_head_cases as fc
import reduction_cases as rc

F32, F64 = np.float32, np.float64
POISON, SLACK = rc.POISON, rc.SLACK
GARBAGE = 1.0e30
ld, cdiv = fc.ld, bc.cdiv
fusable, fused_rows, fused_wide, gemm_tile, head_fusable = fc.fusable, fc.fused_rows, fc.fused_wide, fc.gemm_tile, fc.head_fusable
FUSED_NW = fc.FUSED_NW                     # fused.h:70
FUSED_THREADS = 64 * FUSED_NW              # fused.h:150, the stride of the deferred stash walk in 16-byte quads
EXPF_ABS, SUB_ABS = 2.0 ** -23, 2.0 ** -24

Case = namedtuple("Case", "name dims nets packed B ldx stash_all")


# ---------------------------------------------------------------- mirror: what is missing from the head and backward cases
def on_fused_path(case):
    """pqlk_mlp_forward (gemm.hip:1118): packed weights given and the stack fusable."""
    return bool(case.packed and fusable(case.dims))


def n_hidden(case):
    return len(case.dims) - 2


def kernel(case):
    """gemm.hip, launch_fused_hidden: (R, TM) of k_mlp_fwd_fused<R, TM>."""
    return fused_rows(case.dims, case.nets, fusable(case.dims), case.B), (4 if fused_wide(case.dims) else 2)


def tpw_of(ntiles):
    """fused.h:403: output tiles per wave of a layer."""
    return 4 if ntiles > 2 * FUSED_NW else 2 if ntiles > FUSED_NW else 1


def ring(case, l):
    """fused.h:378 (D), :463 (K8), :166-168 (G, rem): ring depth, reduction steps of 8, whole ring groups, remainder steps of
    hidden layer l.  rem > 0 only on layer 0: every other layer's input width is a multiple of 32."""
    D = 2 if kernel(case)[1] == 4 else 4
    K8 = cdiv(case.dims[l], 8)
    return D, K8, K8 // D, K8 % D


def waves(ntiles):
    """fused.h:137-138: (tiles per wave, active waves, the last active wave holds fewer tiles than the others)."""
    tpw = tpw_of(ntiles)
    return tpw, min(FUSED_NW, cdiv(ntiles, tpw)), ntiles % tpw != 0


def row_tiles(case):
    """fused.h:385, :400: (tiles per net, some tile is full, the last tile is ragged)."""
    rows = 32 * kernel(case)[0]
    return cdiv(case.B, rows), case.B >= rows, case.B % rows != 0


def stash_route(case, l, full_tile):
    """fused.h:469-474: how hidden layer l's block leaves the block of a full / ragged row tile: "deferred" (from layer l + 1's main
    loop), "epilogue", or None (not at all)."""
    if l == n_hidden(case) - 1:                                    # :471 keep_last (no TD head here)
        return "epilogue" if case.stash_all or not head_fusable(case.dims) else None
    if not case.stash_all:
        return None
    return "deferred" if full_tile else "epilogue"                 # :469, :473


def written(case, l):
    """Whether the call writes hidden block l at all (include/pqlk.h: stash_all = 0 is a statement about the fused path)."""
    return not on_fused_path(case) or stash_route(case, l, True) is not None


def defer_walk(case, l):
    """fused.h:146-191 for the deferred stash of hidden layer l (written while layer l + 1 runs): (nprev4, loop trips an active
    wave offers, most and fewest quads a thread owns, layer l + 1 has idle waves)."""
    nprev4 = case.dims[l + 1] // 4                                 # :475
    _, _, G, _ = ring(case, l + 1)
    total = 32 * kernel(case)[0] * nprev4
    return nprev4, max(G - 2, 0), cdiv(total, FUSED_THREADS), total // FUSED_THREADS, waves(case.dims[l + 2] // 32)[1] < FUSED_NW


def block_map(case):
    """fused.h:386-393: "xcd" (even XCD groups take net 0) iff nets == 2 and tiles % 4 == 0, else net-major."""
    tiles = row_tiles(case)[0]
    return "xcd" if case.nets == 2 and tiles % 4 == 0 else "one_net" if case.nets == 1 else "two_nets"


def hidden_gemms(case):
    """gemm.hip:1129-1164 for the hidden layers of the per-layer path: (tile, xcd order, has an edge tile) per layer.  An edge tile
    is one the epilogue does not take as `full` (gemm.hip:662)."""
    out = []
    for l in range(n_hidden(case)):
        N, K = case.dims[l + 1], ld(case.dims[l])
        tile = gemm_tile(case.B, ld(N), case.nets)
        _, loop, xcd, _ = bc.gemm_plan("FWD", "ELU", tile, case.B, N, K, case.ldx if l == 0 else K, K, ld(N), case.nets)
        assert loop == "staged"                                    # gemm.hip:174: no LDS-DMA loop on the forward
        out.append((tile, xcd, case.B % tile != 0 or N % tile != 0))
    return out


def path_name(case):
    if on_fused_path(case):
        R, TM = kernel(case)
        return f"k_mlp_fwd_fused<{R},{TM}>"
    return "k_gemm<FWD,ELU>" + "".join(f"[{t},{x},{'edge' if e else 'whole'}]" for t, x, e in hidden_gemms(case))


# ---------------------------------------------------------------- the table
smallest_b = fc.smallest_b
R2_DIMS = [72, 288, 32, 3]
B_R2_2NETS = smallest_b(lambda B: fused_rows(R2_DIMS, 2, fusable(R2_DIMS), B) == 2)      # 4097: the last 64-row tile holds one row
B_R2_1NET = smallest_b(lambda B: fused_rows(R2_DIMS, 1, fusable(R2_DIMS), B) == 2)       # 8193
B_R2_LAST33 = 64 * 64 + 33                                                                # the last 64-row tile holds 33 rows
B_R2_XCD = 64 * 68                                                                        # 68 tiles: tiles % 4 == 0
G128_DIMS = [32, 128, 128, 1]
B_GEMM128 = smallest_b(lambda B: gemm_tile(B, 128, 2) == 128)                             # 128 row tiles x one column tile x two nets

_W = "ldx+32"
_TABLE = [
    # dims, nets, packed?, [(B, flags...)]       flags: "ldx+32" (a wider input tile), "s0" (stash_all = 0)
    # ---- k_mlp_fwd_fused<1, 2>: the batches of one 32-row tile and around it; layer 0 shorter than the ring (K8 = 1 < D = 4)
    ([3, 32, 1], 1, True, [(1,), (31,), (32,), (33, _W), (97,)]),
    ([3, 32, 1], 2, True, [(128,)]),                                # four tiles, two nets: the XCD-aware block map
    ([10, 32, 64, 2], 1, True, [(33, _W)]),                         # deferred stash of 8 quads per row, no loop trip to carry it
    ([10, 32, 64, 2], 2, True, [(33,)]),                            # two nets, two tiles: net-major map
    ([30, 32, 64, 2], 1, True, [(33,)]),                            # K8 == D on layer 0
    ([13, 96, 32, 3], 1, True, [(33,), (32,)]),                     # 24 quads per row, one loop trip for two quads per thread
    ([13, 96, 32, 3], 2, True, [(33, "s0")]),                       # fused head, stash_all = 0: every hidden block untouched
    ([33, 96, 64, 40], 1, True, [(33,), (33, "s0")]),               # 40 outputs: the head is not fused, stash_all = 0 keeps the last block
    ([60, 64, 32, 3], 1, True, [(33,)]),                            # layer 0: two whole groups, no remainder
    ([90, 96, 32, 3], 1, True, [(33, _W)]),                         # layer 0: three whole groups, no remainder
    ([72, 288, 32, 3], 1, True, [(33,), (97,)]),                    # 9 tiles: two per wave, the fifth wave half filled, three idle; 72 quads
    ([229, 512, 256, 51], 2, True, [(96,)]),                        # 16 tiles: two per wave, none idle; 8 tiles: one per wave, none idle
    ([229, 512, 256, 51], 1, True, [(33, "s0")]),
    ([8, 32, 288, 32, 3], 1, True, [(33,)]),                        # tiles per wave 1 -> 2 -> 1
    ([8, 32, 288, 32, 3], 2, True, [(31,)]),
    ([300, 64, 64, 1], 1, True, [(33,)]),                           # an input wider than every hidden layer
    ([300, 64, 64, 1], 2, True, [(97, _W)]),
    # ---- k_mlp_fwd_fused<2, 2>: 64-row blocks
    (R2_DIMS, 2, True, [(B_R2_2NETS,)]),
    (R2_DIMS, 1, True, [(B_R2_1NET,)]),
    ([229, 512, 256, 51], 2, True, [(B_R2_LAST33,)]),
    ([10, 32, 64, 2], 2, True, [(B_R2_XCD,)]),
    # ---- k_mlp_fwd_fused<1, 4>: a hidden layer wider than 512, ring depth 2; layer 0 of 1 .. 7 reduction steps
    ([8, 544, 288, 32, 3], 1, True, [(33,)]),                       # tiles per wave 4 -> 2 -> 1; 17 tiles: the fifth wave holds one; 136 quads
    ([8, 544, 288, 32, 3], 2, True, [(128,)]),
    ([14, 544, 32, 3], 1, True, [(33,)]),                           # K8 = 2 == D
    ([17, 1024, 32, 2], 1, True, [(33,), (1,)]),                    # 32 tiles: four per wave, none idle; 256 quads; K8 = 3
    ([30, 1024, 96, 2], 1, True, [(32, _W)]),                       # K8 = 4
    ([40, 640, 1], 1, True, [(32,)]),                               # 20 tiles: four per wave, three idle; K8 = 5
    ([47, 544, 32, 3], 2, True, [(33,)]),                           # K8 = 6
    ([55, 544, 32, 3], 1, True, [(33, "s0")]),                      # K8 = 7
    # ---- the per-layer path, k_gemm<FWD, 64, 64, EPI_ELU>: widths that are no multiples of 32, then every tile order
    ([48, 100, 36, 12], 1, False, [(130,), (2082,)]),               # 6 and 66 tiles of layer 0: dispatch order, contiguous runs
    ([16, 48, 128, 5], 1, False, [(500,)]),                         # 8 row tiles: whole groups, edge tiles
    ([16, 48, 128, 5], 2, False, [(250,)]),
    (G128_DIMS, 1, False, [(128,), (512,), (2112,)]),               # whole tiles only: dispatch order, whole groups, runs
    # ---- k_gemm<FWD, 128, 128, EPI_ELU>
    (G128_DIMS, 2, False, [(B_GEMM128,), (16384,), (16385,), (16512,)]),
]


def _name(dims, nets, packed, B, wide, s0):
    return ("x".join(str(d) for d in dims) + f"-n{nets}-{'packed' if packed else 'layers'}-B{B}" + ("-wide" if wide else "")
            + ("-s0" if s0 else ""))


CASES = [Case(_name(dims, nets, packed, b[0], _W in b, "s0" in b), list(dims), nets, packed, b[0],
              ld(dims[0]) + (32 if _W in b else 0), 0 if "s0" in b else 1)
         for dims, nets, packed, Bs in _TABLE for b in Bs]
CASE_BY_NAME = {c.name: c for c in CASES}
assert len(CASE_BY_NAME) == len(CASES)
DESIGNS = ("exact", "dense")


def cells():
    return [(c, d) for c in CASES for d in DESIGNS]


# ---------------------------------------------------------------- what the table must reach
_GCLASSES = [(0, True), (1, False), (1, True), (2, False), (2, True), (3, False), (3, True)]   # G == 0 leaves only the remainder
COVERAGE = (
    [("kernel", R, TM) for R, TM in ((1, 2), (2, 2), (1, 4))]
    # fused_layer's groups: G = 0 (remainder only), 1 (last group only), 2 (peeled + last), >= 3 (the loop runs), with and
    # without remainder steps.  (rem > 0 is reachable on layer 0 only.)
    + [("ring", D, g, rem) for D in (4, 2) for g, rem in _GCLASSES]
    + [("layer0", D, rel) for D in (4, 2) for rel in ("K8<D", "K8==D")]
    # tiles per wave: (1, "partial") does not exist (one tile per wave fills every active wave)
    + [("tpw", 1, "idle"), ("tpw", 1, "all"), ("tpw", 2, "partial"), ("tpw", 2, "idle"), ("tpw", 2, "all"),
       ("tpw", 4, "partial"), ("tpw", 4, "idle"), ("tpw", 4, "all")]
    + [("tpw_in", TM, t) for TM, t in ((2, 1), (2, 2), (4, 1), (4, 2), (4, 4))]
    + [("tpw_seq", (4, 2, 1)), ("tpw_seq", (1, 2, 1))]
    + [("defer", q) for q in (8, 24, 72, 136, 256)]
    + [("defer", s) for s in ("no_trips", "trips<quads", "trips>quads", "idle_consumer", "R2")]
    + [("route", r) for r in ("deferred", "epilogue_ragged", "epilogue_last", None)]
    + [("map", m) for m in ("xcd", "one_net", "two_nets")] + [("map", "xcd", k) for k in ((1, 2), (2, 2), (1, 4))]
    + [("mask", r) for r in (1, 2, 3)] + [("ldx_wide",), ("input_wider",)]
    + [("stash0", "fused_head"), ("stash0", "plain_head")]
    + [("B", b) for b in (1, 31, 32, 33, 97)] + [("B", 128, "two_nets")]
    + [("R2", s) for s in ("first_2nets", "first_1net", "last33", "tiles%4")]
    + [("width", w) for w in (32, 96, 256, 288, 512, 544, 1024)]
    + [("gemm", tile, xcd, edge) for tile, xcd, edge in
       ((64, 0, False), (64, 0, True), (64, "groups", False), (64, "groups", True), (64, "runs", False), (64, "runs", True),
        (128, "groups", False), (128, "groups", True), (128, "runs", False), (128, "runs", True))]
    + [("gemm", "pad_width"), ("gemm", "two_nets")]
)
# not reachable: the 128 tile needs at least 256 tiles (gemm.hip:832), dispatch order fewer than 64 (gemm.hip:765)
UNREACHABLE = [("gemm", 128, 0, False), ("gemm", 128, 0, True)]


def reached(case):
    """The items of COVERAGE this case reaches."""
    dims, H, out = case.dims, n_hidden(case), set()
    if not on_fused_path(case):
        for l, g in enumerate(hidden_gemms(case)):
            out.add(("gemm",) + g)
            if dims[l + 1] % 32 != 0 and l + 1 < H:
                out.add(("gemm", "pad_width"))                     # the next layer reads K = pqlk_ld(width) columns
        if case.nets == 2:
            out.add(("gemm", "two_nets"))
        return out
    R, TM = kernel(case)
    tiles, has_full, has_ragged = row_tiles(case)
    out.add(("kernel", R, TM))
    seq = []
    for l in range(H):
        D, K8, G, rem = ring(case, l)
        out.add(("ring", D, min(G, 3), rem > 0))
        assert rem == 0 or l == 0
        if l == 0 and K8 <= D:
            out.add(("layer0", D, "K8<D" if K8 < D else "K8==D"))
        tpw, active, partial = waves(dims[l + 1] // 32)
        seq.append(tpw)
        out.add(("tpw_in", TM, tpw))
        out.add(("tpw", tpw, "idle" if active < FUSED_NW else "all"))
        if partial:
            out.add(("tpw", tpw, "partial"))
        out.add(("width", dims[l + 1]))
        for full in ([True] if has_full else []) + ([False] if has_ragged else []):
            r = stash_route(case, l, full)
            out.add(("route", ("epilogue_last" if l == H - 1 else "epilogue_ragged") if r == "epilogue" else r))
            if r == "deferred":
                nprev4, trips, most, fewest, idle = defer_walk(case, l)
                out.add(("defer", nprev4))
                out.add(("defer", "no_trips" if trips == 0 else "trips<quads" if trips < most else "trips>quads" if trips > most else "trips==quads"))
                if idle:
                    out.add(("defer", "idle_consumer"))
                if R == 2:
                    out.add(("defer", "R2"))
    out.add(("tpw_seq", tuple(seq)))
    m = block_map(case)
    out.add(("map", m))
    if m == "xcd":
        out.add(("map", "xcd", (R, TM)))
    out.add(("mask", dims[0] % 4))
    if case.ldx > ld(dims[0]):
        out.add(("ldx_wide",))
    if dims[0] > max(dims[1:-1]):
        out.add(("input_wider",))
    if not case.stash_all:
        out.add(("stash0", "fused_head" if head_fusable(dims) else "plain_head"))
    if R == 1 and case.B == 128 and case.nets == 2:
        out.add(("B", 128, "two_nets"))
    if R == 1:
        out.add(("B", case.B))
    if R == 2:
        for tag, hit in (("first_2nets", case.nets == 2 and case.B == B_R2_2NETS), ("first_1net", case.nets == 1 and case.B == B_R2_1NET),
                         ("last33", case.B % 64 == 33), ("tiles%4", tiles % 4 == 0)):
            if hit:
                out.add(("R2", tag))
    return out


# ---------------------------------------------------------------- inputs
GATE = 128                                 # x[:, 0] on the rows whose gated units of layer 0 are dead
WVALS = np.array([1, 2, 3, -1, -2, -3], dtype=F32)
MAX_NNZ = 8


def _seed(case, what, net=0, layer=0):
    return bc._seed(case, what, net, layer)


def _exact_layer(case, n, l, lo, hi):
    """W (N, K), bias (N,) and the range of the alive units' outputs, for inputs in [lo, hi] (column 0 of x, the gate, aside).
    Units j % 4 == 3 are dead on every row, units j % 4 == 2 of layer 0 are dead on the gated rows (backward_cases.exact_network);
    units j % 4 < 2, alive on every row, carry one non-zero weight per reduction step of 8 of their 32-unit tile, column 0 (above
    layer 0) and column K - 1 among them."""
    N, K = case.dims[l + 1], case.dims[l]
    first = 1 if l == 0 else 0
    K8 = cdiv(K, 8)
    assert K - first >= 1
    W = np.zeros((N, K), dtype=F32)
    val = WVALS[dd.integers((cdiv(N, 32), K8), _seed(case, 31, n, l), len(WVALS))]
    pick = dd.integers((cdiv(N, 32), K8), _seed(case, 32, n, l), 8)
    for t in range(cdiv(N, 32)):
        units = [j for j in range(32 * t, min(N, 32 * t + 32)) if j % 4 < 2]
        assert K8 <= MAX_NNZ * len(units), (case.name, l, t)
        for s in range(K8):
            c0, c1 = max(8 * s, first), min(8 * s + 8, K)
            c = c0 + int(pick[t, s]) % (c1 - c0)
            if s == 0 and l > 0:
                c = 0
            if s == K8 - 1:
                c = K - 1
            W[units[s % len(units)], c] = val[t, s]
    want = 1 + dd.integers((N,), _seed(case, 33, n, l), MAX_NNZ)
    rows = np.arange(N)
    for e in range(MAX_NNZ):                                       # fill up to `want` non-zeros per unit
        cols = first + dd.integers((N,), _seed(case, 34 + e, n, l), K - first)
        v = WVALS[dd.integers((N,), _seed(case, 44 + e, n, l), len(WVALS))]
        m = ((W != 0).sum(1) < want) & (W[rows, cols] == 0)
        W[rows[m], cols[m]] = v[m]
    assert (W != 0).sum(1).max() <= MAX_NNZ and (W != 0).sum(1).min() >= 1
    P, M = np.where(W > 0, W, 0).sum(1), -np.where(W < 0, W, 0).sum(1)
    smin, smax = P * lo - M * hi, P * hi - M * lo
    dead = rows % 4 == 3
    b = np.where(dead, -32 - smax, -smin).astype(F32)
    if l == 0:
        gated = rows % 4 == 2
        assert (smax - smin)[gated].max() <= GATE - 32
        W[gated, 0] = -1
    return W, b, int((smax - smin)[~dead].max())


@functools.lru_cache(maxsize=4)
def _network(name, design):
    case = CASE_BY_NAME[name]
    dims, B, H = case.dims, case.B, n_hidden(case)
    dense = fc.weights(case)
    if design == "dense":
        x, nets = fc.x_input(case), dense
    else:
        x = rc.ints((B, dims[0]), _seed(case, 30), -2, 2)
        x[:, 0] = np.where(np.arange(B) % 4 == 1, GATE, 0)
        nets = []
        for n in range(case.nets):
            lo, hi, net = -2, 2, []
            for l in range(H):
                W, b, top = _exact_layer(case, n, l, lo, hi)
                net.append((W, b))
                lo, hi = -1, top
            nets.append(net + [dense[n][-1]])                      # the output layer is not the subject: any head
    x.setflags(write=False)
    return nets, x


def network(case, design):
    """([net][layer] -> (W (out, in), b (out,)), x (B, dims[0])) of a design; shared and read-only."""
    return _network(case.name, design)


def x_tile(case, design, garbage=GARBAGE):
    """The (B, ldx) input tile: `garbage` in columns [dims[0], ldx) on the fused path, which ignores them; zeros on the per-layer
    path, which requires them (include/pqlk.h)."""
    out = np.full((case.B, case.ldx), garbage if on_fused_path(case) else 0.0, dtype=F32)
    out[:, : case.dims[0]] = network(case, design)[1]
    return out


def arena(case, design):
    """The parameter arena (include/pqlk.h layout, zero pad columns)."""
    dims, ns = case.dims, bc.net_stride(case.dims)
    out = np.zeros(ns * case.nets, dtype=F32)
    for n, net in enumerate(network(case, design)[0]):
        for l, (w, b) in enumerate(net):
            wo, bo = bc.layer_offsets(dims, l)
            out[n * ns + wo: n * ns + bo].reshape(dims[l + 1], ld(dims[l]))[:, : dims[l]] = w
            out[n * ns + bo: n * ns + bo + dims[l + 1]] = b
    return out


# ---------------------------------------------------------------- references
elu64, preact64, bound, bits_equal = fc.elu64, fc.preact64, fc.bound, fc.bits_equal


@functools.lru_cache(maxsize=4)
def _exact_reference(name):
    case = CASE_BY_NAME[name]
    nets, x = network(case, "exact")
    out, bits = [], 0.0
    for net in nets:
        a, hs = x.astype(F64), []
        for W, b in net[:-1]:
            W, b = W.astype(F64), b.astype(F64)
            z = a @ W.T + b
            assert np.array_equal(z, np.round(z)) and bool(((z >= 0) | (z <= -32)).all()), name
            bits = max(bits, float(np.log2((np.abs(a) @ np.abs(W).T + np.abs(b)).max())))
            a = np.where(z >= 0, z, -1.0)
            h = a.astype(F32)
            h.setflags(write=False)
            hs.append(h)
        out.append(hs)
    return out, bits


def exact_reference(case):
    """[net][layer] -> (B, dims[layer + 1]) float32 image of the float64 hidden activations of the exact design."""
    return _exact_reference(case.name)[0]


def exactness_bits(case):
    """log2 of the largest sum_k |h_k W_jk| + |b_j| over every hidden unit and row: at most 24 means every partial sum, in any
    order or grouping, is an integer that fp32 holds exactly."""
    return _exact_reference(case.name)[1]


def exact_feasible(case):
    """The conditions the `==` of the exact design rests on; the name of the first one that fails, or None."""
    if exactness_bits(case) > 24:
        return "a partial sum can pass 2^24"
    nets, _ = network(case, "exact")
    ref = exact_reference(case)
    for n, net in enumerate(nets):
        for l, (W, b) in enumerate(net[:-1]):
            N, K = W.shape
            alive = np.arange(N) % 4 < 2
            if int((W != 0).sum(1).max()) > MAX_NNZ + (l == 0) or not set(np.unique(np.abs(W))) <= {0.0, 1.0, 2.0, 3.0}:
                return f"weights of layer {l}"
            if not (W[:, 0] != 0).any() or not (W[:, K - 1] != 0).any():
                return f"column 0 or {K - 1} of layer {l} meets no weight"
            for t in range(cdiv(N, 32)):
                rows = slice(32 * t, min(N, 32 * t + 32))
                for s in range(cdiv(K, 8)):
                    if not (W[rows, 8 * s: 8 * s + 8][alive[rows]] != 0).any():
                        return f"layer {l} tile {t} step {s} meets no weight of an alive unit"
            h = ref[n][l]
            if not bool((h[:, alive] >= 0).all()) or not bool((h[:, np.arange(N) % 4 == 3] == -1).all()):
                return f"alive / dead units of layer {l}"
            if l == 0 and case.B >= 4 and not (bool((h[1::4, 2::4] == -1).all()) and bool((h[0::4, 2::4] >= 0).all())):
                return "gated units"
    return None


# ---------------------------------------------------------------- checks (numpy in, AssertionError out)
# Largest measured share of the dense bar on the MI355X over every case of the table, per path (the bar is not derived from it; a
# share above 1 would be a finding).  Fused: k_mlp_fwd_fused<2, 2> on [10, 32, 64, 2], two nets, 4352 rows (<1, 2> reaches 0.045,
# <1, 4> 0.052); per-layer: k_gemm<FWD, 128, 128, EPI_ELU> on [32, 128, 128, 1] at 16257 rows (the 64 tile reaches 0.051).
MEASURED_SHARE = {"fused": 0.060, "gemm": 0.079}


def hidden_block(case, stash, net, l):
    """(B, ld) view of one net's hidden block l in a flat stash."""
    off, ldh = bc.act_offset(case.dims, case.nets, case.B, net, l)
    return stash[off: off + case.B * ldh].reshape(case.B, ldh)


def hidden_floats(case):
    """Floats of the stash in front of the output layer's block."""
    return bc.act_offset(case.dims, case.nets, case.B, 0, n_hidden(case))[0]


def _bits_differ(a, b):
    return np.argwhere(np.ascontiguousarray(a).view(np.uint32) != np.ascontiguousarray(b).view(np.uint32))


def check_stash(case, design, stash, full=None, what=""):
    """stash: the flat activation stash as the call left it over POISON.  Every hidden block the call must not write still holds
    POISON bit for bit; every other one has zero pad columns and meets the design's reference (exact: bit equality with the
    float64 activations; dense: the bar of the module docstring, from the kernel's own previous block).  full: the stash of the
    same case under stash_all = 1, needed when stash_all = 0 -- it supplies the previous block, and the blocks written must equal
    its bits.  Returns the worst share of the dense bar (0.0 for the exact design)."""
    dims, B, H = case.dims, case.B, n_hidden(case)
    what = what or f"{case.name} {design}"
    nets, x = network(case, design)
    ref = exact_reference(case) if design == "exact" else None
    poison = np.full(1, POISON, dtype=F32).view(np.uint32)[0]
    worst = 0.0
    for n in range(case.nets):
        for l in range(H):
            N, blk = dims[l + 1], hidden_block(case, stash, n, l)
            if not written(case, l):
                bad = np.argwhere(blk.view(np.uint32) != poison)
                assert bad.size == 0, f"{what}: stash_all = 0 wrote hidden block {l} of net {n}, first at (row, col) {tuple(bad[0])}"
                continue
            assert np.all(blk[:, N:] == 0), f"{what}: pad columns of hidden block {l} of net {n} are not zero"
            if full is not None:
                bad = _bits_differ(blk, hidden_block(case, full, n, l))
                assert bad.size == 0, f"{what}: hidden block {l} of net {n} differs from the stash_all = 1 run at {len(bad)} elements"
            if design == "exact":
                bad = _bits_differ(blk[:, :N], ref[n][l])
                assert bad.size == 0, (f"{what}: hidden block {l} of net {n} differs from the float64 activations at {len(bad)} elements, first "
                                       f"at (row, col) {tuple(bad[0])}: {blk[tuple(bad[0])]} != {ref[n][l][tuple(bad[0])]}")
                continue
            if l == 0:
                prev = x
            else:
                src = stash if written(case, l - 1) else full
                assert src is not None, "a stash_all = 0 case needs the stash_all = 1 stash for the previous block"
                prev = hidden_block(case, src, n, l - 1)[:, : dims[l]]
            W, b = nets[n][l]
            with np.errstate(invalid="ignore", over="ignore"):
                z = preact64(prev, W, b)
                lim = bound(prev, W, b, ld(dims[l])) + (z < 0) * (EXPF_ABS + SUB_ABS)
                err = np.abs(blk[:, :N].astype(F64) - elu64(z))
                ok = err <= lim
            share = float(np.max(np.where(ok, err / np.maximum(lim, 1e-300), np.inf)))
            assert bool(ok.all()), (f"{what}: hidden block {l} of net {n} misses the bar at {int((~ok).sum())} elements, first at (row, col) "
                                    f"{tuple(np.argwhere(~ok)[0])}")
            worst = max(worst, share)
    return worst


def check_same_hidden(case, a, b, what=""):
    """The hidden blocks of two stashes of the same case are bit-identical (include/pqlk.h: fused and per-layer paths)."""
    n = hidden_floats(case)
    bad = _bits_differ(a[:n], b[:n])
    assert bad.size == 0, f"{what}: hidden activations differ at {len(bad)} elements, first at float {int(bad[0][0])}"


# ---------------------------------------------------------------- a float32 numpy forward, for the checks' own tests
FAULTS = ("drop_last_step", "quad_mask", "swap_tiles", "stash_row_shift", "stash0_write", "pad_nonzero", "neighbour_bias", "elu_positive_only")


def fault_applies(case, fault):
    """Whether the fault can be planted in this case and leaves a trace in a block the call writes."""
    dims, H = case.dims, n_hidden(case)
    fused = on_fused_path(case)
    seen = lambda l0: any(written(case, l) for l in range(l0, H))  # noqa: E731  (a wrong layer shows in every block above it)
    swap_l = next((l for l in range(H) if dims[l + 1] >= 64), H)
    return {"drop_last_step": seen(0),
            "quad_mask": fused and dims[0] % 4 != 0 and seen(0),
            "swap_tiles": seen(swap_l),
            "stash_row_shift": fused and H >= 2 and bool(case.stash_all) and row_tiles(case)[1],
            "stash0_write": fused and not case.stash_all,
            "pad_nonzero": any(d % 32 != 0 for d in dims[1:-1]),
            "neighbour_bias": H >= 2 and seen(0),
            "elu_positive_only": seen(0)}[fault]


def model_hidden(case, design, fault=None, garbage=GARBAGE, stash_all=None):
    """The flat stash a forward leaves over POISON, computed in float32 numpy (numpy's summation order, ELU correctly rounded from
    float64; the output layer's block is zeros), with one fault planted:
      drop_last_step     the last reduction step of 8 of layer 0 is dropped
      quad_mask          the input is masked by whole quads: columns [dims[0], round_up(dims[0], 4)) of x reach the products
                         (visible only with garbage = nan, see the module docstring)
      swap_tiles         output tiles 0 and 1 of the first layer that has two change places
      stash_row_shift    row 5 of a deferred-stashed block holds row 6 (the next layer still reads the right one)
      stash0_write       hidden block 0 is written under stash_all = 0
      pad_nonzero        one pad column of a hidden block is not zero
      neighbour_bias     every hidden layer adds the bias of the hidden layer next to it
      elu_positive_only  negative pre-activations pass through unchanged"""
    sa = case.stash_all if stash_all is None else stash_all
    case = case._replace(stash_all=sa)
    assert fault is None or fault_applies(case, fault), fault
    dims, B, H = case.dims, case.B, n_hidden(case)
    nets, _ = network(case, design)
    xt, k0, w = x_tile(case, design, garbage), ld(dims[0]), dims[0]
    xin = xt[:, :k0].copy()
    if on_fused_path(case):                                         # fused.h:447-452
        keep = min(cdiv(w, 4) * 4, k0) if fault == "quad_mask" else w
        xin[:, keep:] = 0
    out = np.full(bc.acts_floats(dims, case.nets, B), POISON, dtype=F32)
    out[hidden_floats(case):] = 0
    swap_l = next((l for l in range(H) if dims[l + 1] >= 64), None)
    shift_l = next((l for l in range(H - 1) if stash_route(case, l, True) == "deferred"), None)
    for n in range(case.nets):
        h = xin
        for l in range(H):
            W, b = nets[n][l]
            N, K = W.shape
            Wp = np.zeros((N, h.shape[1]), dtype=F32); Wp[:, :K] = W
            hh = h
            if fault == "drop_last_step" and l == 0:
                keep = 8 * (cdiv(K, 8) - 1)
                hh, Wp = h[:, :keep], Wp[:, :keep]
            if fault == "neighbour_bias":
                b = np.resize(nets[n][l + 1 if l + 1 < H else l - 1][1], N)
            with np.errstate(invalid="ignore", over="ignore"):
                z = ((hh @ Wp.T).astype(F32) + b.astype(F32)).astype(F32)
                a = z if fault == "elu_positive_only" else np.where(z > 0, z, np.expm1(np.minimum(z.astype(F64), 0.0))).astype(F32)
            if fault == "swap_tiles" and l == swap_l:
                a = np.concatenate([a[:, 32:64], a[:, :32], a[:, 64:]], axis=1)
            if written(case, l) or (fault == "stash0_write" and l == 0):
                blk = hidden_block(case, out, n, l)
                blk[:, :N], blk[:, N:] = a, 0
                if fault == "stash_row_shift" and l == shift_l:
                    blk[5, :N] = a[6]
                if fault == "pad_nonzero" and N % 32 != 0:
                    blk[B - 1, N] = 2.0 ** -20
            h = a
    return out
