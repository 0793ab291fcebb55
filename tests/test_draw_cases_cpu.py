"""What tests/draw_cases.py guarantees to tests/test_draws_gpu.py, shown without a GPU: the model's counter layout is rocRAND's, its
increments are the library's, its vectorised form is the per-element law, its table reaches every edge of the launch, and the checks
the GPU test applies reject each plausible wrong law at a case this file names."""
import math

import numpy as np
import pytest

import draw_cases as dc

SMALL_CAP = 8        # a device of 8 blocks: every case keeps its meaning (the five small shapes stay below the cap), at 1 / 256 of the size

# rocrand_init(seed, subsequence, offset) + two rocrand4 calls, from a host build of rocRAND's philox4x32_10 device header
ROCRAND_BLOCKS = [
    ((5, 0, 0), (3289868317, 299389332, 4225117243, 4147765880), (1491303360, 670720010, 2467182222, 513040669)),
    ((5, 3, 64), (2327574856, 293174555, 972350515, 1606605970), (4203100695, 4084067740, 3676938430, 1589154191)),
    ((9223372036854788153, 524287, 17179869176), (2383212454, 524339855, 258394936, 3315094045),
     (2706412518, 2228864791, 1213056281, 3422982375)),
    ((9223372036854788153, 1, 17179869180), (2284722643, 1762504333, 1295986419, 2374707282),
     (2544248799, 3999520736, 436402922, 948928331)),
    ((7, 2, 17179869184), (2440874810, 1341044302, 2345721605, 1160622502), (2623237634, 1321769321, 4262032186, 4204637216)),
]


@pytest.mark.parametrize("row", ROCRAND_BLOCKS, ids=lambda r: "-".join(map(str, r[0])))
def test_counter_layout_is_rocrands(row):
    """Rows 3 to 5 have the key's second word set and sit below, across and above the carry of offset / 4 into the second counter word."""
    (seed, subsequence, offset), first, second = row
    assert offset % 4 == 0
    assert tuple(int(w) for w in dc.block(seed, offset // 4, subsequence)) == first
    assert tuple(int(w) for w in dc.block(seed, offset // 4 + 1, subsequence)) == second
    both = dc.block(seed, np.array([offset // 4, offset // 4 + 1], dtype=np.uint64), np.array([subsequence] * 2, dtype=np.uint64))
    assert [tuple(int(w[i]) for w in both) for i in (0, 1)] == [first, second]          # the array form the model uses


def test_increment_is_the_librarys():
    """Without a device the library stands in the MI355X's 2048 blocks."""
    from pql_amd import _lib as L
    numels = {n for c in dc.cases() for n in (c.n_idx, c.n_normal)}
    numels |= {0, 1, 8192, 8192 * 16, 2048 * 256, 2048 * 256 * 4, 2048 * 256 * 4 + 1, 32768 * 21}      # those of tests/test_host_cpu.py
    numels |= {2048 * 256 * 8, 2048 * 256 * 8 + 1}
    for n in sorted(numels):
        assert dc.inc(n, dc.MI355X_BLOCKS) == L.lib.pqlk_philox_increment(n), n
    assert [dc.inc(n, dc.MI355X_BLOCKS) for n in (0, 1, 2048 * 256 * 4, 2048 * 256 * 4 + 1)] == [0, 4, 4, 8]
    assert [dc.threads(n, dc.MI355X_BLOCKS) for n in (1, 256, 257, 2048 * 256, 2048 * 256 + 1)] == [256, 256, 512, 524288, 524288]


def test_box_muller_is_the_formula():
    """The vectorised Box-Muller against the formula in python floats; 4e-15 = a few float64 ulp of values below 7, for the two
    libms.  The 128 largest words, whose float32 value is 2^32, give s = 0 as the float32 sum does."""
    c = float(dc.TWO_PI_2POW32_INV)
    assert c == float(np.float32(1.46291807926715968105133780430e-9))            # rocrand_common.h: ROCRAND_2POW32_INV_2PI
    for x, y in ((0, 0), (1, 2), (0x7FFFFFFF, 0x80000000), (123456789, 987654321), (0xFFFFFF7F, 0xFFFFFFFF), (16777217, 16777219)):
        xf, yf = float(np.float32(x)), float(np.float32(y))
        u, v = 2.0 ** -32 + xf * 2.0 ** -32, c + yf * c
        s = math.sqrt(-2.0 * math.log(u))
        a, b = dc.box_muller(x, y)
        assert abs(float(a) - math.sin(v) * s) <= 4e-15 and abs(float(b) - math.cos(v) * s) <= 4e-15, (x, y)
    for x in (0xFFFFFF80, 0xFFFFFFFF):
        a, b = dc.box_muller(x, 12345)
        assert float(a) == 0.0 and float(b) == 0.0
    a, _ = dc.box_muller(0xFFFFFF7F, 1 << 30)                                     # the largest word below: float32 gives 2^32 - 256
    assert float(a) > 0.0


def _slow_case(c, cap):
    """A case by slow_part, in python integers; normals through the same box_muller (held to the formula above)."""
    inc_idx = dc.inc(c.n_idx, cap)
    inc_step = inc_idx + dc.inc(c.n_normal, cap)
    ahead = 0 if c.step is None else c.step - c.base_step
    idx, nrm = [], []
    for ch in range(c.chunks):
        off = c.base_offset + (ahead + ch) * inc_step
        idx.append([w % c.range for w, _, _, _ in dc.slow_part(c.seed, off, c.n_idx, cap)])
        el = dc.slow_part(c.seed, off + inc_idx, c.n_normal, cap)
        a, b = dc.box_muller([e[1] for e in el], [e[2] for e in el]) if el else (np.zeros(0), np.zeros(0))
        nrm.append([(b if e[3] % 2 else a)[i] for i, e in enumerate(el)])
    return np.array(idx, dtype=np.int64).reshape(c.chunks, c.n_idx), np.array(nrm, dtype=np.float64).reshape(c.chunks, c.n_normal)


@pytest.mark.parametrize("name", dc.CASE_NAMES)
def test_vectorised_model_is_the_per_element_law(name):
    """Every case on a device of 8 blocks, so that the capped and the two-trip cases are small too, and the five shapes below the
    cap at the MI355X's 2048 blocks as well (they do not depend on the cap: the two models must agree, and with each other)."""
    caps = (SMALL_CAP, dc.MI355X_BLOCKS) if name.split("-")[0] not in ("cap", "four", "idxtrip") else (SMALL_CAP,)
    for cap in caps:
        c = dc.case(name, cap)
        want, (idx, nrm) = dc.model(c, cap), _slow_case(c, cap)
        assert np.array_equal(want.idx, idx) and np.array_equal(want.normals, nrm), cap
        assert want.idx.shape == (c.chunks, c.n_idx) and want.normals.shape == (c.chunks, c.n_normal)
        if c.n_idx:
            assert 0 <= want.idx.min() and want.idx.max() < c.range
            assert np.array_equal(want.idx_words.astype(np.int64) % c.range, want.idx)
    if len(caps) == 2:
        assert all(np.array_equal(a, b) for a, b in zip(dc.model(dc.case(name, caps[0]), caps[0])[:4],
                                                        dc.model(dc.case(name, caps[1]), caps[1])[:4]))


def test_step_ahead_is_the_null_form_further_on():
    """step_dev[0] = 7 with base_step = 5 is step_dev = NULL at base_offset + 2 inc_step; NULL does not look at base_step."""
    for cap in (SMALL_CAP, dc.MI355X_BLOCKS):
        for c in dc.cases(cap):
            if max(c.n_idx, c.n_normal) > 4096:
                continue
            want = dc.model(c, cap)
            ahead = 0 if c.step is None else c.step - c.base_step
            for base_step in (0, 5):
                null = dc.model(c._replace(step=None, base_step=base_step, base_offset=c.base_offset + ahead * want.inc_step), cap)
                assert all(np.array_equal(a, b) for a, b in zip(want[:4], null[:4])), c.name


@pytest.mark.parametrize("cap", [SMALL_CAP, dc.MI355X_BLOCKS, 304 * 8])
def test_table_reaches_every_edge(cap):
    reached = {c.name: dc.edges(c, cap) for c in dc.cases(cap)}
    union = set().union(*reached.values())
    assert union == set(dc.EDGES), set(dc.EDGES) ^ union
    at = lambda name: reached[name]   # noqa: E731
    # the edges of the kernel that the suite had never run, each at the case built for it
    assert {"below_one_block", "ragged_block", "normals_larger", "many_chunks"} <= at("ragged-s5-o0-null")
    assert {"exactly_cap", "second_component", "range_per"} <= at("cap-s64-o4-null")
    assert {"exactly_four", "second_trip_normals", "carry_inside_a_part"} <= at("four-s64-carry+0-null")
    assert {"second_trip_indices", "idx_larger", "carry_inside_a_part", "range_per"} <= at("idxtrip-s5-carry+4-equal")
    assert {"idx_larger", "high_key_word", "step_equal"} <= at("idxwide-s64-carry+0-equal")
    assert {"normals_only", "below_carry", "at_carry", "above_carry"} <= at("nrmonly-s64-carry+0-null")
    assert {"indices_only", "range_max"} <= at("idxonly-s64-o0-equal")
    assert {"below_carry", "at_carry", "above_carry", "high_key_word", "step_null"} <= at("ragged-s64-carry+0-null")
    assert {"below_carry", "at_carry", "above_carry", "step_ahead"} <= at("ragged-s64-carry-16-ahead")
    assert {"step_null_base_nonzero"} <= at("ragged-s64-o0-null5")
    assert {"range_1", "below_one_block"} <= at("lone-s5-o0-null") and {"range_1", "at_carry", "step_ahead"} <= at("lone-s64-carry+0-ahead")
    # the two large rows come in one form each
    assert [n.split("-")[0] for n in reached].count("cap") == 1 and [n.split("-")[0] for n in reached].count("four") == 1
    # within the ABI: offsets are multiples of 4, ranges below 2^28, the largest launch is the cap
    for c in dc.cases(cap):
        assert c.base_offset % 4 == 0 and 0 < c.range < 1 << 28 and c.n_idx + c.n_normal > 0 and 1 <= c.chunks <= 65535
        assert max(c.n_idx, c.n_normal) <= 4 * 256 * cap + 1


# Each wrong law, and the cases whose checks must reject it (every one of them is rejected; others may reject it too).
REJECTED_BY = {
    "second_trip_dropped": ("four-s64-carry+0-null", "idxtrip-s5-carry+4-equal"),
    "second_trip_first_block": ("four-s64-carry+0-null", "idxtrip-s5-carry+4-equal"),
    "stride_t": ("cap-s64-o4-null", "four-s64-carry+0-null", "idxtrip-s5-carry+4-equal"),
    "components_contiguous": ("ragged-s5-o0-null", "idxonly-s64-o0-equal", "nrmonly-s5-o0-ahead", "cap-s64-o4-null"),
    "normals_not_advanced": ("ragged-s5-o0-null", "idxwide-s5-o4-null", "cap-s64-o4-null"),
    "chunk_stride_idx": ("ragged-s5-o0-null", "idxwide-s5-o4-null", "nrmonly-s64-carry+0-null", "four-s64-carry+0-null"),
    "step_ignored": ("ragged-s64-carry-16-ahead", "ragged-s5-o4-ahead", "nrmonly-s5-o0-ahead"),
    "null_step_zero": ("ragged-s64-o0-null5",),
    "seed_low_word": ("ragged-s64-o4-equal", "idxonly-s64-o0-equal", "nrmonly-s64-carry+0-null", "four-s64-carry+0-null"),
    "block_low_word": ("ragged-s64-carry+0-null", "ragged-s64-carry-16-ahead", "idxwide-s64-carry+0-equal", "nrmonly-s64-carry+0-null",
                       "idxonly-s5-carry+0-null", "four-s64-carry+0-null", "idxtrip-s5-carry+4-equal"),
    "sincos_swapped": ("ragged-s5-o0-null", "nrmonly-s5-o0-ahead", "idxwide-s5-o4-null"),
}
# ... and where a fault can only show at certain cases, those are ALL that reject it: the table has no second witness to lose
ONLY_REJECTED_BY = ("second_trip_dropped", "second_trip_first_block", "stride_t", "step_ignored", "null_step_zero", "block_low_word")


def _rejects(c, cap, fault):
    want, got = dc.model(c, cap), dc.as_written(dc.model(c, cap, fault))
    try:
        dc.check_case(want, *got, dc.BAR_CEILING)      # the largest bar the GPU test may use: rejected here, rejected at any smaller one
    except AssertionError:
        return True
    return False


def test_checks_accept_the_model_itself():
    for c in dc.cases(SMALL_CAP):
        want = dc.model(c, SMALL_CAP)
        assert dc.check_case(want, *dc.as_written(want), dc.BAR_CEILING) <= 1e-6      # float32 rounding of values below 7


@pytest.mark.parametrize("fault", dc.FAULTS)
def test_each_wrong_law_is_rejected(fault):
    assert set(REJECTED_BY) == set(dc.FAULTS)
    rejecting = {c.name for c in dc.cases(SMALL_CAP) if _rejects(c, SMALL_CAP, fault)}
    print(f"{fault}: rejected by {sorted(rejecting)}")
    assert set(REJECTED_BY[fault]) <= rejecting, set(REJECTED_BY[fault]) - rejecting
    if fault in ONLY_REJECTED_BY:
        assert rejecting == set(REJECTED_BY[fault])


def test_checks_reject_an_unwritten_or_extra_element():
    """One element left at the buffer's fill, one non-finite normal, a wrong dtype: each is a failure, not a distance."""
    c = dc.case("ragged-s5-o0-null", SMALL_CAP)
    want = dc.model(c, SMALL_CAP)
    idx, nrm = (a.copy() for a in dc.as_written(want))
    bad = idx.copy(); bad[2, 254] = dc.IDX_SENTINEL
    with pytest.raises(AssertionError, match=r"\(2, 254\)"):
        dc.check_indices(want, bad)
    for v in (dc.NRM_SENTINEL, np.nan, np.inf):
        bad = nrm.copy(); bad[1, 256] = v
        with pytest.raises(AssertionError):
            dc.check_normals(want, bad, dc.BAR_CEILING)
    with pytest.raises(AssertionError):
        dc.check_indices(want, idx.astype(np.int32))
    with pytest.raises(AssertionError):
        dc.check_normals(want, nrm, 2 * dc.BAR_CEILING)           # a bar above the ceiling is itself refused
