"""The table of tests/gather_cases.py means what tests/test_gather_kernels_gpu.py assumes: the layout mirror is the library's,
every case reaches the kernel it names and the cases together reach all 58 instantiations of the fused gather and every runtime
variant, the numpy normalisation is the oracle's, the clamp binds on a real share of the elements, the host refuses what it says
it refuses, and the checks fail on the wrong outputs they are there to catch.  No GPU needed."""
import ctypes as C

import numpy as np
import pytest
import torch

import gather_cases as gc

F32, F16 = gc.F32, gc.F16
E_NULL, E_ALIGN, E_UNSUPPORTED = 1, 4, 5

# every instantiation of the fused gather in pql_amd/csrc/replay.hip
INSTANTIATIONS = [
    "k_replay_gather_fast<true, 1>", "k_replay_gather_fast<true, 2>", "k_replay_gather_fast<true, 4>", "k_replay_gather_fast<true, 8>",
    "k_replay_gather_fast<false, 1>", "k_replay_gather_fast<false, 2>", "k_replay_gather_fast<false, 4>", "k_replay_gather_fast<false, 8>",
    "k_replay_gather_obs<true, 1>", "k_replay_gather_obs<true, 2>", "k_replay_gather_obs<true, 4>",
    "k_replay_gather_obs<false, 1>", "k_replay_gather_obs<false, 2>", "k_replay_gather_obs<false, 4>",
    "k_replay_gather_fused<true, 4, 1>", "k_replay_gather_fused<true, 2, 2>", "k_replay_gather_fused<true, 1, 4>",
    "k_replay_gather_fused<true, 1, 16>",
    "k_replay_gather_fused<false, 4, 1>", "k_replay_gather_fused<false, 2, 2>", "k_replay_gather_fused<false, 1, 4>",
    "k_replay_gather_fused<false, 1, 16>",
    "k_replay_gather_fast_h8<true, 1>", "k_replay_gather_fast_h8<true, 2>", "k_replay_gather_fast_h8<true, 4>",
    "k_replay_gather_fast_h8<true, 8>",
    "k_replay_gather_fast_h8<false, 1>", "k_replay_gather_fast_h8<false, 2>", "k_replay_gather_fast_h8<false, 4>",
    "k_replay_gather_fast_h8<false, 8>",
    "k_replay_gather_fast_f16<true, 1>", "k_replay_gather_fast_f16<true, 2>", "k_replay_gather_fast_f16<true, 4>",
    "k_replay_gather_fast_f16<true, 8>",
    "k_replay_gather_fast_f16<false, 1>", "k_replay_gather_fast_f16<false, 2>", "k_replay_gather_fast_f16<false, 4>",
    "k_replay_gather_fast_f16<false, 8>",
    "k_replay_gather_obs_h8<true, 1>", "k_replay_gather_obs_h8<true, 2>", "k_replay_gather_obs_h8<true, 4>",
    "k_replay_gather_obs_h8<false, 1>", "k_replay_gather_obs_h8<false, 2>", "k_replay_gather_obs_h8<false, 4>",
    "k_replay_gather_obs_f16<true, 1>", "k_replay_gather_obs_f16<true, 2>", "k_replay_gather_obs_f16<true, 4>",
    "k_replay_gather_obs_f16<false, 1>", "k_replay_gather_obs_f16<false, 2>", "k_replay_gather_obs_f16<false, 4>",
    "k_replay_gather_fused_f16<true, 4, 1>", "k_replay_gather_fused_f16<true, 2, 2>", "k_replay_gather_fused_f16<true, 1, 4>",
    "k_replay_gather_fused_f16<true, 1, 16>",
    "k_replay_gather_fused_f16<false, 4, 1>", "k_replay_gather_fused_f16<false, 2, 2>", "k_replay_gather_fused_f16<false, 1, 4>",
    "k_replay_gather_fused_f16<false, 1, 16>",
]

# (storage, A): the smallest O on each side of the 64 | 65, 128 | 129 and 256 | 257 chunk seams
SEAMS = {(F32, 4): [(124, 125), (252, 253), (508, 509)], (F32, 8): [(120, 121), (248, 249), (504, 505)],
         (F32, -1): [(256, 257), (512, 513), (1024, 1025)], (F16, 4): [(248, 249), (504, 505), (1016, 1017)],
         (F16, 8): [(240, 241), (496, 497), (1008, 1009)], (F16, -1): [(512, 513), (1024, 1025), (2048, 2049)]}


# --------------------------------------------------------------------------- the mirrors against the library and the table
def test_layout_mirror_is_the_librarys():
    """pqlk_replay_rec_ld_ex is a host call: it loads without a GPU"""
    from pql_amd import _lib as L
    rec_ld = L.lib.pqlk_replay_rec_ld_ex
    for dtype in (F32, F16):
        for A in [-1] + list(range(1, 25)):
            for O in range(1, 2101):
                assert rec_ld(O, A, dtype) == gc.layout(O, A, dtype).ld, (dtype, O, A)
    for cols in (0, 1, 31, 32, 33, 100, 2048):
        assert int(L.lib.pqlk_ld(cols)) == gc.ld(cols)
    for O, A in ((5, 3), (8, 2), (13, -1)):      # the fields of both layouts: 16-byte starts, no overlap, everything inside `used`
        for dtype in (F32, F16):
            lay = gc.layout(O, A, dtype)
            per_word = 1 if dtype == F32 else 2
            assert lay.field * per_word >= O and lay.field % 4 == 0 and lay.used % 4 == 0 and lay.ld % 32 == 0 and lay.ld >= lay.used
            if A >= 0:
                assert (lay.off_nobs, lay.off_act) == (lay.field, 2 * lay.field) and lay.off_rd >= lay.off_act + A and lay.used == lay.off_rd + 4
            else:
                assert lay.used == lay.field


def test_seams_are_where_the_chunk_counts_say():
    for (dtype, A), pairs in SEAMS.items():
        for (lo, hi), edge in zip(pairs, (64, 128, 256)):
            n = lambda O: gc.layout(O, A, dtype).used >> 2     # noqa: E731
            assert n(lo) <= edge < n(hi) and n(lo - 1) <= edge and hi == lo + 1, (dtype, A, lo, hi)
            assert n(lo + 1) > edge, "the smallest O on the far side"
            for O in (lo, hi):
                assert any((c.dtype, c.O, c.A) == (dtype, O, A) for c in gc.CASES), (dtype, O, A)
    assert gc.layout(2044, 4, F32).used >> 2 == gc.MAX_CHUNKS and gc.layout(2045, 4, F32).used >> 2 > gc.MAX_CHUNKS
    # the narrow seam: 512 B in use
    assert gc.layout(120, 4, F16).used * 4 <= 512 < gc.layout(121, 4, F16).used * 4
    assert gc.layout(256, -1, F16).used * 4 <= 512 < gc.layout(257, -1, F16).used * 4
    assert gc.layout(117, 3, F16).used * 4 == 512
    have = {(c.dtype, c.O, c.A) for c in gc.CASES}
    assert {(F16, 120, 4), (F16, 121, 4), (F16, 256, -1), (F16, 257, -1), (F32, 1024, 4), (F16, 1024, 4), (F32, 2044, 4)} <= have
    for dtype in (F32, F16):
        assert {(dtype, 1, 1), (dtype, 5, 3), (dtype, 8, 2)} <= have
        assert {(dtype, O, -1) for O in (1, 5, 9, 17, 33, 65, 129)} <= have


@pytest.mark.parametrize("name", [c.name for c in gc.CASES])
def test_case_reaches_the_kernel_it_names(name):
    c = gc.CASE_BY_NAME[name]
    ld_sa, ld_o = gc.lds(c)
    assert ld_sa % 32 == 0 and ld_o % 32 == 0
    for norm in ((True, False) if gc.has_stats(c) else (False,)):
        for b, flags in gc.base_batches(c):
            path = gc.gather_path(c.O, c.A, c.dtype, ld_sa, ld_o, flags, b, gc.all_dests(c), norm)
            assert path == (c.template, norm, c.shape, c.variant), (b, flags, path)
    if c.extra == 32:       # the fast kernel within its pad bound of 64 columns: 64 more and it is the generic kernel's
        assert 32 <= ld_sa - c.O - c.A <= 64 and 32 <= ld_o - c.O <= 64 and gc.kind(c.template) == "fast"
        wider = gc.gather_path(c.O, c.A, c.dtype, ld_sa + 64, ld_o + 64, 0, 1, gc.all_dests(c))
        assert wider[0].startswith("fused")
    if gc.lean(c):          # the forced one-wave-per-CU run: some wave makes a second trip, and that trip is ragged
        b, flags = gc.base_batches(c)[-1]
        la = gc.launch_of(c, b, flags)
        assert la.blocks == 64 and b == la.blocks * la.rows_blk + 1 and 200 < b <= 64 * 256 + 1
    assert gc.CAP >= 200 and 0 < gc.START < gc.CAP


def test_every_instantiation_and_runtime_variant_is_reached():
    assert len(INSTANTIATIONS) == 58 and len(set(INSTANTIATIONS)) == 58
    reached = gc.reached()
    assert set(reached) == set(INSTANTIATIONS), set(reached) ^ set(INSTANTIATIONS)

    def variants(template):
        return set().union(*(v for k, v in reached.items() if k.startswith(f"k_replay_gather_{template}<")))

    assert variants("fast") == {1, 2} and variants("fast_f16") == {1, 2} and variants("fast_h8") == {1}
    assert variants("obs") == set(range(7)) and variants("obs_h8") == set(range(1, 7)) and variants("obs_f16") == {6}
    both = {gc.TRANSITION, gc.OBS_ONLY}
    for t in ("fused", "fused_f16"):
        for norm in ("true", "false"):
            # (4, 1) on an obs-only ring needs a destination that is not 16-byte aligned: not run
            assert reached[f"k_replay_gather_{t}<{norm}, 4, 1>"] == {gc.TRANSITION}
            assert reached[f"k_replay_gather_{t}<{norm}, 2, 2>"] == both
        # an obs-only record of more than 256 chunks (fp16: of more than 128) is wider than the statistics may be
        assert reached[f"k_replay_gather_{t}<false, 1, 4>"] == both and reached[f"k_replay_gather_{t}<false, 1, 16>"] == both
        assert reached[f"k_replay_gather_{t}<true, 1, 16>"] == {gc.TRANSITION}
    assert reached["k_replay_gather_fused<true, 1, 4>"] == both and reached["k_replay_gather_fused_f16<true, 1, 4>"] == {gc.TRANSITION}
    assert gc.layout(gc.GATHER_MAX_OBS, -1, F32).used >> 2 <= 256 and gc.layout(gc.GATHER_MAX_OBS, -1, F16).used >> 2 <= 128
    for name in gc.PAST_CAP:
        c = gc.CASE_BY_NAME[name]
        la = gc.launch_of(c, gc.past_cap_rows(c))
        assert la.blocks == gc.GENERIC_MAX_BLOCKS and gc.past_cap_rows(c) > la.blocks * la.rows_blk and gc.has_stats(c)
    assert sorted((gc.CASE_BY_NAME[n].dtype, gc.CASE_BY_NAME[n].shape) for n in gc.PAST_CAP) == sorted(
        (d, s) for d in (F32, F16) for s in ((4, 1), (2, 2), (1, 4), (1, 16)))
    assert [gc.past_cap_rows(gc.CASE_BY_NAME[n]) for n in gc.PAST_CAP[:4]] == [32771, 16387, 8195, 8195]
    for t, name in gc.REPRESENTATIVES.items():
        assert gc.CASE_BY_NAME[name].template == t
    for name in gc.PLAIN_PAST_CAP:      # records of more than 64 chunks: the plain gather's chunk loop takes a second step
        c = gc.CASE_BY_NAME[name]
        assert gc.layout(c.O, c.A, c.dtype).used >> 2 > 64 and c.O % 4
    assert set(gc.REPRESENTATIVES) == {i[len("k_replay_gather_"): i.index("<")] for i in INSTANTIATIONS}
    assert sum(c.strided for c in gc.CASES) == 2 and {c.dtype for c in gc.CASES if c.strided} == {F32, F16}


def test_factor_runs_vary_one_thing_on_every_template():
    for t, name in gc.REPRESENTATIVES.items():
        c = gc.CASE_BY_NAME[name]
        runs = gc.factor_runs(c)
        flags = [f for _, f, _, _ in runs]
        assert 0 in flags and any(f & gc.PADS_ZERO for f in flags) and any(f & gc.NT_LOADS for f in flags) and any(f & gc.NT_STORES for f in flags)
        dests = {d for _, _, _, d in runs if d is not None}
        want = {("x_sa",), ("xn_obs",)} if c.A < 0 else {("x_sa",), ("xn_sa", "rew", "done"), ("xn_obs",), ("x_sa", "xn_sa", "rew", "done")}
        assert dests == want, t
        Rs = {gc.launch_of(c, gc.factor_batch(c, f), f, n, d).shape for _, f, n, d in runs}
        assert Rs == ({1, 2, 4, 8} if gc.kind(t) == "fast" else {1, 2, 4} if gc.kind(t) == "obs" else {c.shape}), (t, Rs)
        for _, f, n, d in runs:       # a factor run never leaves its template and ends on a ragged block or trip
            b = gc.factor_batch(c, f)
            la = gc.launch_of(c, b, f, n, d)
            assert la.template == t and b > 2 * la.rows_blk and b % la.rows_blk != 0
            if (f >> 8) & 15:         # a rows-in-flight override makes a second trip at that R
                assert la.shape == (f >> 8) & 15 and la.blocks == 64 and b == 64 * la.rows_blk + 1


# --------------------------------------------------------------------------- the reference and the data
@pytest.mark.parametrize("clamp", [True, False])
def test_numpy_norm_is_the_oracles(clamp):
    from oracle.pql_ref_cpu import normalize_ref
    for O in (5, 124, 1024):
        d = gc.data(O, 4)
        x = d.ring("obs")
        want = normalize_ref(torch.from_numpy(x), (torch.from_numpy(d.mean), torch.from_numpy(d.var), gc.EPS), clamp=clamp).numpy()
        got = gc.normalize(x, d.mean, d.var, clamp)
        assert got.dtype == np.float32 and np.array_equal(gc.bits(got), gc.bits(want))
        assert not np.isnan(got).any()


def test_clamp_binds_on_a_real_share_of_every_clamped_case():
    for c in gc.CASES:
        if gc.has_stats(c):
            share = gc.data(c.O, c.A).clamped_share(c.dtype)
            assert 0.05 <= share <= 0.50, (c.name, share)
            for f in ("obs",) + (("nobs",) if c.A >= 0 else ()):
                y = gc.data(c.O, c.A).normed(f, c.dtype, True, True)
                assert np.isfinite(y).all() and np.abs(y).max() == 5.0


def test_data_holds_what_the_cases_need():
    d = gc.data(8, 2)
    raw = d.src["done"][:, 0]
    assert (raw == 2.5).any() and (np.signbit(raw) & (raw == 0)).any() and set(np.unique(d.ring("done"))) == {0.0, 1.0}
    assert d.head > 0 and d.head < gc.CAP and np.array_equal(d.ring("obs")[gc.START], d.src["obs"][0])
    assert np.array_equal(d.ring("obs")[0], d.src["obs"][d.head])
    for b in (7, 8, 37, 1025):
        idx = gc.indices(b, 5)
        vals, counts = np.unique(idx, return_counts=True)
        assert {0, gc.CAP - 1, -1, gc.CAP, gc.CAP + 5} <= set(vals.tolist()) and (counts[(vals > 0) & (vals < gc.CAP - 1)] > 1).any()
        assert idx[-1] == gc.CAP - 1
        assert np.array_equal(gc.sources(idx), np.where((idx < 0) | (idx >= gc.CAP), 0, idx))
    assert gc.indices(1, 5).tolist() == [gc.CAP - 1] and len(gc.indices(3, 5)) == 3
    # the fp16 ring stores something else than the fp32 ring, and the records say so
    assert not np.array_equal(d.ring("obs", F16), d.ring("obs", F32))
    for dtype in (F32, F16):
        w = gc.expected_records(dtype, d)
        lay = gc.layout(8, 2, dtype)
        assert w.shape == (gc.CAP, lay.ld) and not w[:, lay.used:].any() and w[:, lay.off_rd + 2: lay.off_rd + 4].sum() == 0
        assert set(np.unique(w[:, lay.off_rd + 1]).tolist()) == {0, 0x3F800000}
    h = gc.expected_records(F16, gc.data(5, 3))
    lay = gc.layout(5, 3, F16)
    assert np.array_equal(h[:, 2] & 0xFFFF, gc.data(5, 3).ring("obs").astype(np.float16).view(np.uint16)[:, 4]) and not (h[:, 2] >> 16).any()
    assert not h[:, 3].any() and np.array_equal(h[:, lay.off_act + 2], gc.data(5, 3).ring("act").view(np.uint32)[:, 2]) and not h[:, lay.off_act + 3].any()


# --------------------------------------------------------------------------- what the host refuses
def test_host_refusals_of_the_fused_gather():
    from pql_amd import _lib as L
    P = C.c_void_p(0x1000)          # never dereferenced: every call below is refused before a launch

    def call(O, A, dtype, b=4, mean=P, var=P, x_sa=P, ld_sa=None, xn_sa=None, xn_obs=None, ld_o=None):
        ring = L.PqlReplayDesc(0x1000, 100, O, A, int(L.lib.pqlk_replay_rec_ld_ex(O, A, dtype)), dtype)
        ld_sa = gc.ld(O + max(A, 0)) if ld_sa is None else ld_sa
        ld_o = gc.ld(O) if ld_o is None else ld_o
        return L.lib.pqlk_replay_gather_fused(C.byref(ring), P, b, mean, var, gc.EPS, gc.CLAMP5, x_sa, ld_sa, xn_sa, xn_obs, ld_o, None, None, None)

    for dtype in (F32, F16):
        assert call(1025, -1, dtype) == E_UNSUPPORTED                                  # statistics wider than GATHER_MAX_OBS
        assert call(1025, 4, dtype) == E_UNSUPPORTED
        assert call(8, -1, dtype, xn_sa=P) == E_UNSUPPORTED                            # xn_sa on an obs-only ring
        assert call(8, 2, dtype, ld_sa=40) == E_ALIGN and call(8, 2, dtype, xn_sa=P, x_sa=None, ld_sa=40) == E_ALIGN   # ld % 32
        assert call(40, 2, dtype, ld_sa=32) == E_ALIGN                                 # too small for O + A
        assert call(31, 2, dtype, ld_sa=32) == E_ALIGN                                 # O fits, O + A does not
        assert call(8, 2, dtype, xn_obs=P, ld_o=40) == E_ALIGN and call(40, 2, dtype, xn_obs=P, ld_o=32) == E_ALIGN
        assert call(8, 2, dtype, var=None) == E_NULL and call(8, 2, dtype, mean=None) == E_NULL   # one statistic without the other
    # more than 1024 chunks: refused with rows to gather, accepted as the empty call it is with none
    for O, A, dtype in ((2045, 4, F32), (4097, -1, F32), (4089, 4, F16), (8193, -1, F16)):
        assert gc.layout(O, A, dtype).used >> 2 > gc.MAX_CHUNKS >= gc.layout(O - 1, A, dtype).used >> 2
        assert call(O, A, dtype, mean=None, var=None) == E_UNSUPPORTED
        assert call(O, A, dtype, b=0, mean=None, var=None) == 0


def test_host_refusals_of_insert_and_plain_gather():
    """pqlk_replay_insert and pqlk_replay_gather check in one order whatever the storage format: null, shape, dtype, rec_ld,
    range / required pointers, and only then the empty call.  The last column is an unknown dtype code: what is checked before
    the dtype answers as for a known one, everything after it is PQLK_E_SHAPE."""
    from pql_amd import _lib as L
    P = C.c_void_p(0x1000)          # never dereferenced: every call below is refused, or is empty, before a launch
    OK, E_SHAPE, E_RANGE, UNKNOWN = 0, 2, 3, 2
    O, A = 8, 2

    def ring(dtype, A=A, records=0x1000, cap=100, O=O, off=0):
        rec_ld = gc.layout(max(O, 1), A, dtype if dtype in (F32, F16) else F32).ld + off
        return L.PqlReplayDesc(records, cap, O, A, rec_ld, dtype)

    def insert(r, dst=0, m=4, obs=P, ld_obs=O, act=P, rew=P, nobs=P, done=P):
        return L.lib.pqlk_replay_insert(None if r is None else C.byref(r), dst, m, obs, ld_obs, act, A, rew, 1, nobs, O, done, 1, None)

    def gather(r, idx=P, b=4, obs=P, act=P, rew=P, nobs=P, done=P):
        return L.lib.pqlk_replay_gather(None if r is None else C.byref(r), idx, b, obs, act, rew, nobs, done, None)

    # (what, call(dtype), code for fp32 and fp16 rings, code for the unknown dtype)
    rows = [
        ("insert: null ring", lambda d: insert(None), E_NULL, E_NULL),
        ("insert: null records", lambda d: insert(ring(d, records=0)), E_NULL, E_NULL),
        ("insert: null obs", lambda d: insert(ring(d), obs=None), E_NULL, E_NULL),
        ("insert: null obs before a bad shape", lambda d: insert(ring(d, O=0), obs=None), E_NULL, E_NULL),
        ("insert: obs_dim 0", lambda d: insert(ring(d, O=0)), E_SHAPE, E_SHAPE),
        ("insert: obs_dim -3", lambda d: insert(ring(d, O=-3)), E_SHAPE, E_SHAPE),
        ("insert: capacity 0", lambda d: insert(ring(d, cap=0)), E_SHAPE, E_SHAPE),
        ("insert: capacity -1", lambda d: insert(ring(d, cap=-1)), E_SHAPE, E_SHAPE),
        ("insert: m -1", lambda d: insert(ring(d), m=-1), E_SHAPE, E_SHAPE),
        ("insert: rec_ld + 32", lambda d: insert(ring(d, off=32)), E_SHAPE, E_SHAPE),
        ("insert: rec_ld - 32", lambda d: insert(ring(d, off=-32)), E_SHAPE, E_SHAPE),
        ("insert: wrong rec_ld before the range", lambda d: insert(ring(d, off=32), dst=98), E_SHAPE, E_SHAPE),
        ("insert: rows 98..101 of 100", lambda d: insert(ring(d), dst=98), E_RANGE, E_SHAPE),
        ("insert: row 100 of 100, m 1", lambda d: insert(ring(d), dst=100, m=1), E_RANGE, E_SHAPE),
        ("insert: dst_start -1", lambda d: insert(ring(d), dst=-1), E_RANGE, E_SHAPE),
        ("insert: dst_start -1 of an empty call", lambda d: insert(ring(d), dst=-1, m=0), E_RANGE, E_SHAPE),
        ("insert: range before a missing pointer", lambda d: insert(ring(d), dst=98, act=None), E_RANGE, E_SHAPE),
        ("insert: no act", lambda d: insert(ring(d), act=None), E_NULL, E_SHAPE),
        ("insert: no rew", lambda d: insert(ring(d), rew=None), E_NULL, E_SHAPE),
        ("insert: no next_obs", lambda d: insert(ring(d), nobs=None), E_NULL, E_SHAPE),
        ("insert: no done", lambda d: insert(ring(d), done=None), E_NULL, E_SHAPE),
        ("insert: no done of an empty call", lambda d: insert(ring(d), m=0, done=None), E_NULL, E_SHAPE),
        ("insert: missing pointer before ld_obs", lambda d: insert(ring(d), act=None, ld_obs=O - 1), E_NULL, E_SHAPE),
        ("insert: ld_obs < O", lambda d: insert(ring(d), ld_obs=O - 1), E_SHAPE, E_SHAPE),
        ("insert: ld_obs < O of an empty call", lambda d: insert(ring(d), m=0, ld_obs=O - 1), E_SHAPE, E_SHAPE),
        ("insert: ld_obs < O, obs-only", lambda d: insert(ring(d, A=-1), ld_obs=O - 1, act=None, rew=None, nobs=None, done=None), E_SHAPE, E_SHAPE),
        ("insert: empty call", lambda d: insert(ring(d), m=0), OK, E_SHAPE),
        ("insert: empty call at the end of the ring", lambda d: insert(ring(d), dst=100, m=0), OK, E_SHAPE),
        ("insert: empty call, obs-only, obs alone", lambda d: insert(ring(d, A=-1), m=0, act=None, rew=None, nobs=None, done=None), OK, E_SHAPE),
        ("gather: null ring", lambda d: gather(None), E_NULL, E_NULL),
        ("gather: null records", lambda d: gather(ring(d, records=0)), E_NULL, E_NULL),
        ("gather: null idx", lambda d: gather(ring(d), idx=None), E_NULL, E_NULL),
        ("gather: null obs", lambda d: gather(ring(d), obs=None), E_NULL, E_NULL),
        ("gather: null idx before a bad shape", lambda d: gather(ring(d, cap=0), idx=None), E_NULL, E_NULL),
        ("gather: obs_dim 0", lambda d: gather(ring(d, O=0)), E_SHAPE, E_SHAPE),
        ("gather: capacity 0", lambda d: gather(ring(d, cap=0)), E_SHAPE, E_SHAPE),
        ("gather: b -1", lambda d: gather(ring(d), b=-1), E_SHAPE, E_SHAPE),
        ("gather: rec_ld + 32", lambda d: gather(ring(d, off=32)), E_SHAPE, E_SHAPE),
        ("gather: wrong rec_ld before a missing pointer", lambda d: gather(ring(d, off=32), act=None), E_SHAPE, E_SHAPE),
        ("gather: no act", lambda d: gather(ring(d), act=None), E_NULL, E_SHAPE),
        ("gather: no rew", lambda d: gather(ring(d), rew=None), E_NULL, E_SHAPE),
        ("gather: no next_obs", lambda d: gather(ring(d), nobs=None), E_NULL, E_SHAPE),
        ("gather: no done", lambda d: gather(ring(d), done=None), E_NULL, E_SHAPE),
        ("gather: no done of an empty call", lambda d: gather(ring(d), b=0, done=None), E_NULL, E_SHAPE),
        ("gather: empty call", lambda d: gather(ring(d), b=0), OK, E_SHAPE),
        ("gather: empty call, obs-only, obs alone", lambda d: gather(ring(d, A=-1), b=0, act=None, rew=None, nobs=None, done=None), OK, E_SHAPE),
    ]
    for what, call, known, unknown in rows:
        for dtype, want in ((F32, known), (F16, known), (UNKNOWN, unknown)):
            assert call(dtype) == want, (what, dtype)
    assert insert(ring(UNKNOWN)) == E_SHAPE and gather(ring(UNKNOWN)) == E_SHAPE     # nothing wrong but the dtype

    # the fused gather asks the same of the descriptor, in the same order, before its own checks
    def fused(r, idx=P, b=4, x_sa=P):
        return L.lib.pqlk_replay_gather_fused(None if r is None else C.byref(r), idx, b, None, None, gc.EPS, 0, x_sa, 32, None, None, 32, None, None, None)

    for dtype in (F32, F16, UNKNOWN):
        after = (lambda code: E_SHAPE if dtype == UNKNOWN else code)    # noqa: E731
        assert fused(None) == E_NULL and fused(ring(dtype, records=0)) == E_NULL and fused(ring(dtype), idx=None) == E_NULL
        assert fused(ring(dtype, O=0)) == E_SHAPE and fused(ring(dtype, cap=0)) == E_SHAPE and fused(ring(dtype), b=-1) == E_SHAPE
        assert fused(ring(dtype, off=32)) == E_SHAPE and fused(ring(dtype, off=32), b=0) == E_SHAPE
        assert fused(ring(dtype), b=0) == after(OK) and fused(ring(dtype), b=0, x_sa=None) == after(OK)
    assert fused(ring(UNKNOWN)) == E_SHAPE


# --------------------------------------------------------------------------- the checks fail on wrong outputs
def _want(name="f32_5_3", b=37, flags=gc.CLAMP5):
    c = gc.CASE_BY_NAME[name]
    idx = gc.indices(b, 11)
    return c, idx, gc.expected(c, idx, True, flags)


def _copy(want):
    return {k: v.copy() for k, v in want.items()}


def test_check_passes_on_the_reference_and_fails_on_each_wrong_output():
    c, idx, want = _want()
    O, A, b = c.O, c.A, len(idx)
    gc.check_outputs(_copy(want), want, c, "self")

    def fails(mutate, word):
        got = _copy(want)
        mutate(got)
        with pytest.raises(AssertionError, match=word):
            gc.check_outputs(got, want, c, "mutated")

    def ulp(g):
        g["xn_obs"][b - 1, O - 1] = np.nextafter(g["xn_obs"][b - 1, O - 1], np.float32(9))
    fails(ulp, "observation column")

    def neighbour(g):       # row 5 taken from the record next to the one asked for
        idx2 = idx.copy()
        idx2[5] = (idx2[5] + 1) % gc.CAP
        g["x_sa"][5] = gc.expected(c, idx2, True, gc.CLAMP5)["x_sa"][5]
    fails(neighbour, "row 5")

    def neighbour_rew(g):
        g["rew"][6] = g["rew"][7]
    fails(neighbour_rew, "rew")

    def pad(g):
        g["xn_sa"][0, gc.lds(c)[0] - 1] = np.float32(1e-30)
    fails(pad, "pad column")

    def negative_zero_pad(g):
        g["x_sa"][3, O + A] = np.float32(-0.0)
    fails(negative_zero_pad, "pad column")

    def action_of_xn_sa(g):
        g["xn_sa"][2, O + 1] = want["x_sa"][2, O + 1]
    fails(action_of_xn_sa, "untouched action column")

    def guard(g):
        g["done"][b] = 0.0
    fails(guard, "guard row")

    def guard_tile(g):
        g["x_sa"][b + 1, 0] = want["x_sa"][b - 1, 0]
    fails(guard_tile, "guard row")

    # clamp missing on one element
    unclamped = gc.expected(c, idx, True, 0)
    r, col = np.argwhere(gc.bits(unclamped["x_sa"]) != gc.bits(want["x_sa"]))[0]
    assert abs(want["x_sa"][r, col]) == 5.0 and abs(unclamped["x_sa"][r, col]) > 5.0

    def no_clamp(g):
        g["x_sa"][r, col] = unclamped["x_sa"][r, col]
    fails(no_clamp, "observation column")

    # a missing destination is no pass
    got = _copy(want)
    del got["done"]
    with pytest.raises(AssertionError):
        gc.check_outputs(got, want, c, "short")


def test_reference_follows_flags_formats_and_destinations():
    c, idx, want = _want()
    O, A, b = c.O, c.A, len(idx)
    ld_sa, ld_o = gc.lds(c)
    d = gc.data(O, A)
    src = gc.sources(idx)
    assert src[np.flatnonzero(idx == -1)[0]] == 0 and src[np.flatnonzero(idx == gc.CAP + 5)[0]] == 0
    assert want["x_sa"].shape == (b + 2, ld_sa) and want["xn_obs"].shape == (b + 2, ld_o) and want["rew"].shape == (b + 2,)
    assert np.array_equal(want["x_sa"][:b, O: O + A], d.src["act"][(src - gc.START) % gc.CAP])
    assert (want["xn_sa"][:b, O: O + A] == gc.POISON).all() and (want["x_sa"][:b, O + A:] == 0).all() and (want["x_sa"][b:] == gc.POISON).all()
    assert set(np.unique(want["done"][:b]).tolist()) <= {0.0, 1.0}
    pz = gc.expected(c, idx, True, gc.CLAMP5 | gc.PADS_ZERO)
    assert (pz["x_sa"][:b, O + A:] == gc.POISON).all() and (pz["xn_obs"][:b, O:] == gc.POISON).all()
    assert np.array_equal(pz["x_sa"][:b, : O + A], want["x_sa"][:b, : O + A])
    raw = gc.expected(c, idx, False, 0)
    assert np.array_equal(raw["xn_obs"][:b, :O], d.src["nobs"][(src - gc.START) % gc.CAP])
    assert set(gc.expected(c, idx, True, 0, ("xn_sa", "rew", "done"))) == {"xn_sa", "rew", "done"}
    h = gc.CASE_BY_NAME["f16_5_3"]
    wh = gc.expected(h, idx, False, 0)
    assert np.array_equal(wh["x_sa"][:b, :O], gc.q16(raw["x_sa"][:b, :O])) and np.array_equal(wh["x_sa"][:b, O:], raw["x_sa"][:b, O:])
    with pytest.raises(AssertionError, match="observation column"):
        gc.check_outputs(wh, raw, c, "fp16 against fp32")
    o = gc.CASE_BY_NAME["f32_5_obs"]
    wo = gc.expected(o, idx, True, gc.CLAMP5)
    assert set(wo) == {"x_sa", "xn_obs"} and np.array_equal(wo["x_sa"][:b, :5], wo["xn_obs"][:b, :5]) and (wo["x_sa"][:b, 5:] == 0).all()
    plain = gc.expected_plain(c, idx)
    assert plain["obs"].shape == (b + 2, O) and plain["act"].shape == (b + 2, A) and plain["rew"].shape == (b + 2, 1)
    assert np.array_equal(plain["nobs"][:b], raw["xn_obs"][:b, :O]) and (plain["done"][b:] == gc.POISON).all()
    words = gc.expected_records(F32, d)
    bad = words.copy()
    bad[7, gc.layout(O, A, F32).used] = 1          # a pad word that is not zero
    gc.check_records(words.copy(), words, "self")
    with pytest.raises(AssertionError, match="ring row 7"):
        gc.check_records(bad, words, "pad word")
