"""The law of one pqlk_philox_draws call (include/pqlk.h, pql_amd/csrc/philox.hip's header) as a numpy model, the table of the grid,
counter and step-counter edges at which that kernel can go wrong, and the checks tests/test_draws_gpu.py applies to what the kernel
wrote (plain numpy, no GPU, no library); tests/test_draw_cases_cpu.py proves what they guarantee -- the counter layout against
rocRAND's own blocks, the vectorised model against a per-element loop, and every wrong law in FAULTS rejected by a named case.

The law.  With cap_blocks = CUs x (threads per CU / 256) of the device (2048 on MI355X):
    T(numel)  = 256 * min(cap_blocks, ceil(numel / 256))                       threads that torch launches for a draw of numel values
    inc(numel) = 4 * ceil(numel / (4 T)), 0 for 0                              what the draw moves the generator's offset by
    inc_step  = inc(n_idx) + inc(n_normal)
    off_c     = base_offset + (step - base_step + c) * inc_step                chunk c; step = step_dev[0], or base_step for NULL
    the index part starts at off_c, the normal part at off_c + inc(n_idx)
    element li of a part: thread = li % T, k = li // T: component k % 4 of the Philox4x32-10 block with
        key (seed lo, seed hi), counter (b lo, b hi, thread lo, thread hi), b = off / 4 + k // 4 (a 64-bit sum)
    index  = word % range
    normal: of a block (x, y, z, w) the four values are sin(v1) s1, cos(v1) s1, sin(v2) s2, cos(v2) s2 with
        u = 2^-32 + float32(x) 2^-32,  v = c + float32(y) c,  c = float32(2 pi 2^-32),  s = sqrt(-2 log u)
    in float64 from the float32-converted words."""
import collections
import functools
import math

import numpy as np

from droq_cases import MASK32, SEED, philox4x32_10

F32, F64, U32, U64, I64 = np.float32, np.float64, np.uint32, np.uint64, np.int64

MI355X_BLOCKS = 2048                      # 256 CUs x (2048 threads / 256)
SMALL_SEED = 5
CARRY = (1 << 34) - 8                     # offset of block index 2^32 - 2: two blocks below the carry into the second counter word
RANGE_MAX = (1 << 28) - 1                 # the documented limit (torch draws 64-bit values from 2^28 on)
RANGE_PER = 1 << 24                       # what prioritized replay passes
IDX_SENTINEL, NRM_SENTINEL, STEP_GUARD = -7, 777.0, -3      # fills of the guarded output buffers / the guard around step_dev
BAR_CEILING = 1e-3                        # a misplaced normal is off by 0.1 to 1: no bar above this tells placement from rounding
TWO_PI_2POW32_INV = F32(2.0 * math.pi * 2.0 ** -32)         # rocRAND's ROCRAND_2POW32_INV_2PI
TWO_POW32_INV = 2.0 ** -32


# =========================================================================== the law
def threads(numel, cap_blocks):
    return 256 * min(cap_blocks, -(-numel // 256))


def inc(numel, cap_blocks):
    return 0 if numel <= 0 else 4 * -(-numel // (4 * threads(numel, cap_blocks)))


def block(seed, b, thread):
    """The block of subsequence `thread` at block index b = offset / 4, as rocrand_init(seed, thread, offset) + rocrand4 returns it
    (b, thread: python ints or integer arrays below 2^64).  Four uint32 arrays."""
    b, thread = np.asarray(b, U64), np.asarray(thread, U64)
    return philox4x32_10((seed & MASK32, seed >> 32), (b & U64(MASK32), b >> U64(32), thread & U64(MASK32), thread >> U64(32)))


def box_muller(x, y):
    """(sin(v) s, cos(v) s) of the words (x, y), float64 from the float32-converted words.  float32(x) is 2^32 for the 128 largest
    words, which puts u one step above 1 where the float32 sum the kernels form rounds to 1: u is held to 1 (s = 0) there."""
    xf, yf = np.asarray(x, U32).astype(F32).astype(F64), np.asarray(y, U32).astype(F32).astype(F64)
    u = np.minimum(TWO_POW32_INV + xf * TWO_POW32_INV, 1.0)
    v = F64(TWO_PI_2POW32_INV) + yf * F64(TWO_PI_2POW32_INV)
    s = np.sqrt(-2.0 * np.log(u))
    return np.sin(v) * s, np.cos(v) * s


# A wrong law is the right one with one of these switched on: what a plausible mistake in the kernel or its host side would compute.
FAULTS = (
    "second_trip_dropped",        # the loops run once: elements from 4 T on are never written
    "second_trip_first_block",    # the second rocrand4 call returns the first block again
    "stride_t",                   # li += T instead of 4 T: the trips overlap, the last writer (component 0 of block k) wins
    "components_contiguous",      # a thread's four values side by side (element 4 thread + component) instead of T apart
    "normals_not_advanced",       # the normal part starts at off_c instead of off_c + inc(n_idx)
    "chunk_stride_idx",           # chunk c at c * inc(n_idx) instead of c * inc_step
    "step_ignored",               # step - base_step taken as 0
    "null_step_zero",             # step_dev = NULL read as step 0 instead of base_step
    "seed_low_word",              # the key's second word dropped
    "block_low_word",             # the counter's second word dropped
    "sincos_swapped",             # cos(v) s, sin(v) s
)


def _element_map(numel, t, fault):
    """(thread, block past the part's first, component) of every element."""
    li = np.arange(numel, dtype=I64)
    thread, k = li % t, li // t
    blk, comp = k // 4, k % 4
    if fault == "second_trip_first_block":
        blk = np.zeros_like(k)
    elif fault == "stride_t":
        blk, comp = k, np.zeros_like(k)
    elif fault == "components_contiguous":
        r = li % (4 * t)
        thread, comp = r // 4, r % 4
    return thread, blk, comp


def part_words(seed, off, numel, cap_blocks, fault=None):
    """All four words of every element's block and the element's component, by the law as stated: one block evaluation per element."""
    t = threads(numel, cap_blocks)
    thread, blk, comp = _element_map(numel, t, fault)
    if fault == "seed_low_word":
        seed &= MASK32
    b = np.asarray(off // 4, U64) + blk.astype(U64)
    if fault == "block_low_word":
        b &= U64(MASK32)
    return block(seed, b, thread), comp, (blk >= 1 if fault == "second_trip_dropped" else None)


def part_indices(seed, off, numel, rng_range, cap_blocks, fault=None):
    """(indices int64, words uint32) of torch.randint(range, (numel,)) at offset off."""
    w, comp, unwritten = part_words(seed, off, numel, cap_blocks, fault)
    word = np.choose(comp, w)
    idx = (word.astype(U64) % U64(rng_range)).astype(I64)
    if unwritten is not None:
        idx[unwritten] = IDX_SENTINEL
    return idx, word


def part_normals(seed, off, numel, cap_blocks, fault=None):
    """(normals float64, words (numel, 2) uint32: the pair each value is made of) of empty(numel).normal_() at offset off."""
    w, comp, unwritten = part_words(seed, off, numel, cap_blocks, fault)
    x, y = np.where(comp < 2, w[0], w[2]), np.where(comp < 2, w[1], w[3])
    a, b = box_muller(x, y)
    if fault == "sincos_swapped":
        a, b = b, a
    nrm = np.where(comp % 2 == 0, a, b)
    if unwritten is not None:
        nrm[unwritten] = NRM_SENTINEL
    return nrm, np.stack((x, y), axis=-1)


Draws = collections.namedtuple("Draws", "idx idx_words normals normal_words inc_idx inc_step off0")


def model_draws(seed, base_offset, base_step, step, range, n_idx, n_normal, chunks, cap_blocks, fault=None):  # noqa: A002
    """What pqlk_philox_draws(seed, base_offset, base_step, step_dev -> step (None: NULL), range, n_idx, n_normal, chunks) writes:
    idx (chunks, n_idx) int64 and normals (chunks, n_normal) float64, with the raw words, the two increments and chunk 0's offset."""
    inc_idx, inc_nrm = inc(n_idx, cap_blocks), inc(n_normal, cap_blocks)
    inc_step = inc_idx + inc_nrm
    ahead = 0 if step is None else step - base_step
    if fault == "step_ignored":
        ahead = 0
    elif fault == "null_step_zero" and step is None:
        ahead = -base_step
    stride = inc_idx if fault == "chunk_stride_idx" else inc_step
    off0 = base_offset + ahead * inc_step
    idx, iw, nrm, nw = [], [], [], []
    for c in np.arange(chunks).tolist():
        off = (off0 + c * stride) % (1 << 64)
        i, w = part_indices(seed, off, n_idx, range, cap_blocks, fault) if n_idx else (np.zeros(0, I64), np.zeros(0, U32))
        off_n = off if fault == "normals_not_advanced" else off + inc_idx
        n, v = part_normals(seed, off_n, n_normal, cap_blocks, fault) if n_normal else (np.zeros(0, F64), np.zeros((0, 2), U32))
        idx.append(i), iw.append(w), nrm.append(n), nw.append(v)
    out = Draws(np.stack(idx), np.stack(iw), np.stack(nrm), np.stack(nw), inc_idx, inc_step, off0)
    for a in out[:4]:
        a.setflags(write=False)
    return out


def slow_part(seed, off, numel, cap_blocks):
    """The law once more, one element and one counter at a time in python integers: [(word, x, y, component)] per element."""
    t, out = threads(numel, cap_blocks), []
    for li in np.arange(numel).tolist():
        thread, k = li % t, li // t
        b = (off // 4 + k // 4) % (1 << 64)
        w = [int(v) for v in philox4x32_10((seed & MASK32, seed >> 32), (b & MASK32, b >> 32, thread & MASK32, thread >> 32))]
        comp = k % 4
        out.append((w[comp], w[comp & 2], w[(comp & 2) + 1], comp))
    return out


# =========================================================================== the cases
Case = collections.namedtuple("Case", "name n_idx n_normal chunks range seed base_offset base_step step")

STEP_FORMS = {"null": (0, None), "null5": (5, None), "equal": (5, 5), "ahead": (5, 7)}      # (base_step, step_dev[0] or None = NULL)


def cases(cap_blocks=MI355X_BLOCKS):
    """The smallest shapes at which each edge of the launch exists (t = the thread count at the cap), crossed sparsely with the two
    seeds, the offsets {0, 4, CARRY (+-)} and the step forms.  Names do not depend on cap_blocks."""
    t = 256 * cap_blocks
    shapes = {
        "lone": (1, 0, 1, 1),                           # a lone value, range 1
        "ragged": (255, 257, 3, 977),                   # below / above one block, normals the larger part; inc_step = 8
        "idxwide": (1025, 5, 2, 3),                     # indices the larger part: the normal part is masked by tid < t_nrm
        "nrmonly": (0, 1000, 4, 1),                     # normals only (range unused)
        "idxonly": (1000, 0, 4, RANGE_MAX),             # indices only, the largest range
        "cap": (t, t + 1, 2, RANGE_PER),                # exactly the cap, and the first use of a second component
        "four": (4 * t, 4 * t + 1, 2, 1_000_003),       # exactly four values per thread, and the second trip's first element
        "idxtrip": (4 * t + 1, 5, 1, RANGE_PER),        # the second trip in the index loop, under a narrower normal part
    }
    table = [
        ("lone", SMALL_SEED, 0, "null"),
        ("lone", SEED, CARRY, "ahead"),                 # inc_step = 4: two steps ahead is block 2^32 exactly
        ("ragged", SMALL_SEED, 0, "null"),
        ("ragged", SEED, 4, "equal"),
        ("ragged", SEED, CARRY, "null"),                # chunk 0 below the carry, chunk 1 at block 2^32, chunk 2 above it
        ("ragged", SEED, CARRY - 16, "ahead"),          # the same three offsets, reached through step_dev[0] - base_step = 2
        ("ragged", SMALL_SEED, 4, "ahead"),
        ("ragged", SEED, 0, "null5"),                   # NULL with base_step != 0: still step - base_step = 0
        ("idxwide", SMALL_SEED, 4, "null"),
        ("idxwide", SEED, CARRY, "equal"),
        ("nrmonly", SEED, CARRY, "null"),               # inc_step = 4: blocks 2^32 - 2 .. 2^32 + 1
        ("nrmonly", SMALL_SEED, 0, "ahead"),
        ("idxonly", SEED, 0, "equal"),
        ("idxonly", SMALL_SEED, CARRY, "null"),
        ("cap", SEED, 4, "null"),
        ("four", SEED, CARRY, "null"),                  # chunk 0's normal part: block 2^32 - 1, then 2^32 on its second trip
        ("idxtrip", SMALL_SEED, CARRY + 4, "equal"),    # the index part: block 2^32 - 1, then 2^32 on its second trip
    ]
    out = []
    for shape, seed, off, form in table:
        base_step, step = STEP_FORMS[form]
        name = f"{shape}-{'s64' if seed >> 32 else 's5'}-{'o%d' % off if off < 64 else 'carry%+d' % (off - CARRY)}-{form}"
        out.append(Case(name, *shapes[shape], seed, off, base_step, step))
    return out


CASE_NAMES = [c.name for c in cases()]
assert len(set(CASE_NAMES)) == len(CASE_NAMES)


def case(name, cap_blocks):
    return cases(cap_blocks)[CASE_NAMES.index(name)]


@functools.lru_cache(maxsize=None)
def model(c, cap_blocks, fault=None):
    """model_draws of a case: computed once, shared, never written to."""
    return model_draws(c.seed, c.base_offset, c.base_step, c.step, c.range, c.n_idx, c.n_normal, c.chunks, cap_blocks, fault)


EDGES = (
    "below_one_block", "ragged_block", "exactly_cap", "second_component", "exactly_four", "second_trip_normals", "second_trip_indices",
    "idx_larger", "normals_larger", "normals_only", "indices_only", "high_key_word", "low_key_only",
    "below_carry", "at_carry", "above_carry", "carry_inside_a_part",
    "step_null", "step_null_base_nonzero", "step_equal", "step_ahead", "range_1", "range_max", "range_per", "many_chunks",
)


def edges(c, cap_blocks):
    """Which of EDGES a case reaches, worked out from its numbers."""
    tmax, e = 256 * cap_blocks, set()
    parts = [n for n in (c.n_idx, c.n_normal) if n]
    for n in parts:
        t = threads(n, cap_blocks)
        e |= {"below_one_block"} if n < 256 else set()
        e |= {"ragged_block"} if t > n else set()               # the last block has threads with nothing to write
        e |= {"exactly_cap"} if n == tmax else set()
        e |= {"second_component"} if t < n else set()
        e |= {"exactly_four"} if n == 4 * tmax else set()
    e |= {"second_trip_indices"} if c.n_idx > 4 * tmax else set()
    e |= {"second_trip_normals"} if c.n_normal > 4 * tmax else set()
    if c.n_idx and c.n_normal:
        ti, tn = threads(c.n_idx, cap_blocks), threads(c.n_normal, cap_blocks)
        e |= {"idx_larger"} if ti > tn else {"normals_larger"} if tn > ti else set()
    e |= {"normals_only"} if not c.n_idx else {"indices_only"} if not c.n_normal else set()
    e.add("high_key_word" if c.seed >> 32 else "low_key_only")
    inc_idx, inc_nrm = inc(c.n_idx, cap_blocks), inc(c.n_normal, cap_blocks)
    off0 = c.base_offset + (0 if c.step is None else c.step - c.base_step) * (inc_idx + inc_nrm)
    for ch in np.arange(c.chunks).tolist():
        off = off0 + ch * (inc_idx + inc_nrm)
        for first, n in ((off // 4, inc_idx // 4), ((off + inc_idx) // 4, inc_nrm // 4)):
            if n:
                last = first + n - 1
                e |= {"below_carry"} if first < 1 << 32 else set()
                e |= {"at_carry"} if first <= 1 << 32 <= last else set()
                e |= {"above_carry"} if last > 1 << 32 else set()
                e |= {"carry_inside_a_part"} if first < 1 << 32 <= last else set()
    e.add("step_null" if c.step is None else "step_equal" if c.step == c.base_step else "step_ahead")
    e |= {"step_null_base_nonzero"} if c.step is None and c.base_step else set()
    if c.n_idx:
        e |= {"range_1"} if c.range == 1 else {"range_max"} if c.range == RANGE_MAX else {"range_per"} if c.range == RANGE_PER else set()
    e |= {"many_chunks"} if c.chunks > 1 else set()
    return frozenset(e)


# =========================================================================== the checks of tests/test_draws_gpu.py
def check_indices(want, got_idx):
    """Every index of every chunk is the model's, exactly."""
    got = np.asarray(got_idx)
    assert got.dtype == I64 and got.shape == want.idx.shape, (got.dtype, got.shape, want.idx.shape)
    bad = np.argwhere(got != want.idx).tolist()
    assert not bad, (f"{len(bad)} indices differ, first at (chunk, element) {tuple(bad[0])}: "
                     f"{got[tuple(bad[0])]} != {want.idx[tuple(bad[0])]}")


def normal_distance(want, got_nrm):
    """Largest |got - model| over all chunks; inf where a value is not finite.  0.0 for an absent part."""
    got = np.asarray(got_nrm)
    assert got.dtype == F32 and got.shape == want.normals.shape, (got.dtype, got.shape, want.normals.shape)
    if got.size == 0:
        return 0.0
    d = np.abs(got.astype(F64) - want.normals)
    return float(np.where(np.isfinite(d), d, np.inf).max())


def check_normals(want, got_nrm, bar):
    assert bar <= BAR_CEILING, bar
    d = normal_distance(want, got_nrm)
    assert d < bar, f"largest distance from the float64 model {d:.3e}, bar {bar:.3e}"
    return d


def check_case(want, got_idx, got_nrm, bar):
    check_indices(want, got_idx)
    return check_normals(want, got_nrm, bar)


def as_written(d):
    """A model's draws in the form the kernel writes them: (int64 indices, float32 normals)."""
    return d.idx, d.normals.astype(F32)
