"""Every replay ring kernel of pql_amd/csrc/replay.hip against the CPU reference of the record law in tests/gather_cases.py:
pqlk_replay_insert and pqlk_replay_gather on multi-chunk records of both storage formats, and all 58 instantiations of
pqlk_replay_gather_fused with every runtime variant (halves, lgp, ring kind) -- at one row, around the rows a block takes per
trip, on a wave's ragged second trip, past the generic kernels' block cap, and with clamp, pad, non-temporal, rows-in-flight and
destination choices varied one at a time.  The table, the dispatch mirror and the checks are proved without a GPU in
tests/test_gather_cases_cpu.py.

Everything is bit for bit; there are no tolerances.  Every destination (rew and done included) has two rows of poison behind row
b - 1 and slack in front and behind, which must come back intact; the index vector has slack holding the index of a ring row,
so that a kernel which reads and stores a row >= b shows in the guard rows.  The expected values come from host copies of the
inserted rows, never from the ring.  The clamped inputs hold no NaN (the kernels' fminf(fmaxf(.)) turns a NaN into -5 where
torch.clamp keeps it): nothing here asserts that either way.  Every destination pointer is 16-byte aligned."""
import ctypes as C
import time

import numpy as np
import pytest
import torch

import gather_cases as gc
from guarded import Guarded
from reduction_cases import IN_BIG, SLACK, T
from support import dev  # noqa: F401

pytestmark = pytest.mark.gpu

POISON = float(gc.POISON)
CAP, START = gc.CAP, gc.START


def _launched(rcode, what):
    from pql_amd import _lib as L
    if rcode < 0:      # a HIP error: nothing more may be started on this device
        pytest.exit(f"{what}: HIP error {rcode}", returncode=3)
    L.check(rcode)
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"{what}: {e}", returncode=3)


class _Ring:
    """A ring of CAP records filled through pqlk_replay_insert: source rows [0, head) to ring rows [START, CAP), the rest to
    [0, CAP - head).  The records start as poison, with slack around them."""

    def __init__(self, dev, case):
        from pql_amd import _lib as L
        self.dev, self.case = dev, case
        self.d = d = gc.data(case.O, case.A)
        self.lay = lay = gc.layout(case.O, case.A, case.dtype)
        self.records = Guarded(dev, (CAP, lay.ld), POISON, off=SLACK)
        self.desc = L.PqlReplayDesc(self.records.t.data_ptr(), CAP, case.O, case.A, lay.ld, case.dtype)
        extra = 3 if case.strided else 0      # source strides larger than the widths, junk between the rows
        self.src = {}
        for f, a in d.src.items():
            g = Guarded(dev, (CAP, a.shape[1] + extra), IN_BIG, off=SLACK)
            g.t[:, : a.shape[1]] = T(a).to(dev)
            self.src[f] = g
        for dst, lo, hi in ((START, 0, d.head), (0, d.head, CAP)):
            args = []
            for f in ("obs", "act", "rew", "nobs", "done"):
                g = self.src.get(f)
                args += [None, 0] if g is None else [L.ptr(g.t[lo:]), g.t.stride(0)]
            _launched(L.lib.pqlk_replay_insert(C.byref(self.desc), dst, hi - lo, *args, L.stream(dev)), f"insert {case.name}")
        self.mean, self.var = T(d.mean).to(dev), T(d.var).to(dev)

    def words(self):
        return self.records.t.cpu().numpy().view(np.uint32)

    def fused(self, case, idx, norm, flags, dests, what):
        """one pqlk_replay_gather_fused into fresh poisoned destinations of the case's widths: {name: the whole buffer, guard rows
        included}"""
        from pql_amd import _lib as L
        b = len(idx)
        ld_sa, ld_o = gc.lds(case)
        shapes = {"x_sa": (b + gc.GUARD_ROWS, ld_sa), "xn_sa": (b + gc.GUARD_ROWS, ld_sa), "xn_obs": (b + gc.GUARD_ROWS, ld_o),
                  "rew": (b + gc.GUARD_ROWS,), "done": (b + gc.GUARD_ROWS,)}
        bufs = {name: Guarded(self.dev, shapes[name], POISON, off=SLACK) for name in dests}
        gi = Guarded(self.dev, (b,), gc.TRIPWIRE, init=idx, off=SLACK, dtype=torch.int64)
        p = lambda name: bufs[name].ptr if name in bufs else None      # noqa: E731
        for g in bufs.values():
            assert g.t.data_ptr() % 16 == 0
        _launched(L.lib.pqlk_replay_gather_fused(
            C.byref(self.desc), gi.ptr, b, L.ptr(self.mean) if norm else None, L.ptr(self.var) if norm else None, gc.EPS, flags,
            p("x_sa"), ld_sa, p("xn_sa"), p("xn_obs"), ld_o, p("rew"), p("done"), L.stream(self.dev)), what)
        for name, g in bufs.items():
            assert g.intact(), f"{what}: slack around {name} was written"
        assert gi.intact() and np.array_equal(gi.t.cpu().numpy(), idx), f"{what}: the index vector changed"
        return {name: g.t.cpu().numpy() for name, g in bufs.items()}

    def run(self, case, b, norm, flags, dests=None, seed=0):
        """a fused gather of b rows into the destinations of `case` (a case of this ring's record), checked against the reference;
        returns the launch it made"""
        assert (case.dtype, case.O, case.A) == (self.case.dtype, self.case.O, self.case.A)
        dests = gc.all_dests(case) if dests is None else dests
        la = gc.launch_of(case, b, flags, norm, dests)
        what = f"{case.name} b={b} norm={norm} flags={flags:#x} {'+'.join(dests)} [{gc.instantiation(la)} variant {la.variant}, {la.blocks} blocks]"
        idx = gc.indices(b, 17 + seed + b)
        got = self.fused(case, idx, norm, flags, dests, what)
        gc.check_outputs(got, gc.expected(case, idx, norm, flags, dests, self.d), case, what)
        return la


_RINGS = {}


def _ring(dev, case):
    key = (case.dtype, case.O, case.A)
    if key not in _RINGS:
        _RINGS[key] = _Ring(dev, gc.CASE_BY_NAME[f"{gc.DT[case.dtype]}_{case.O}_{'obs' if case.A < 0 else case.A}"])
    return _RINGS[key]


def _plain_gather(dev, ring, case, b):
    """one pqlk_replay_gather of b rows into guarded outputs, checked against the host rows"""
    from pql_amd import _lib as L
    idx = gc.indices(b, 3)
    want = gc.expected_plain(case, idx, ring.d)
    bufs = {k: Guarded(dev, w.shape, POISON, off=SLACK) for k, w in want.items()}
    gi = Guarded(dev, (b,), gc.TRIPWIRE, init=idx, off=SLACK, dtype=torch.int64)
    p = lambda k: bufs[k].ptr if k in bufs else None      # noqa: E731
    _launched(L.lib.pqlk_replay_gather(C.byref(ring.desc), gi.ptr, b, p("obs"), p("act"), p("rew"), p("nobs"), p("done"), L.stream(dev)),
              f"plain gather {case.name} b={b}")
    for k, g in bufs.items():
        assert g.intact(), f"{case.name}: slack around {k} was written"
    gc.check_outputs({k: g.t.cpu().numpy() for k, g in bufs.items()}, want, case, f"{case.name} plain gather b={b}")


# --------------------------------------------------------------------------- insert and plain gather
@pytest.mark.parametrize("name", [c.name for c in gc.CASES if not c.extra])
def test_insert_writes_the_record_layout_and_the_plain_gather_returns_the_rows(dev, name):
    """The raw records after a wrapped two-segment insert equal the layout built on the CPU, pad words (and pad halves) zero,
    nothing written around the ring; pqlk_replay_gather returns the host rows, out-of-range indices reading row 0."""
    case = gc.CASE_BY_NAME[name]
    t0 = time.perf_counter()
    ring = _ring(dev, case)
    assert ring.case.strided == case.strided
    gc.check_records(ring.words(), gc.expected_records(case.dtype, ring.d), f"{name} records")
    assert ring.records.intact(), "slack around the records was written"
    for g in ring.src.values():
        assert g.intact()
    _plain_gather(dev, ring, case, 37)
    print(f"GATHER {name} insert+plain {time.perf_counter() - t0:.2f}s")


@pytest.mark.parametrize("name", gc.PLAIN_PAST_CAP)
def test_plain_gather_past_its_block_cap(dev, name):
    """8192 blocks x 4 waves and three more rows of a multi-chunk record: every wave's second trip"""
    case = gc.CASE_BY_NAME[name]
    _plain_gather(dev, _ring(dev, case), case, gc.PLAIN_MAX_BLOCKS * 4 + 3)


# --------------------------------------------------------------------------- the fused gather
@pytest.mark.parametrize("name", [c.name for c in gc.CASES])
def test_fused_gather_base_sweep(dev, name):
    """With statistics and clamp, and without statistics: one row; one fewer and one more than a block's rows per trip; for the
    lean kernels, at one wave per CU, the smallest batch that sends a wave on a ragged second trip."""
    case = gc.CASE_BY_NAME[name]
    t0 = time.perf_counter()
    ring = _ring(dev, case)
    runs = 0
    for norm in ((True, False) if gc.has_stats(case) else (False,)):
        for b, flags in gc.base_batches(case):
            la = ring.run(case, b, norm, flags | (gc.CLAMP5 if norm else 0))
            assert tuple(la[:4]) == (case.template, norm, case.shape, case.variant)
            runs += 1
    print(f"GATHER {name} {case.template}{case.shape} variant {case.variant}: {runs} launches {time.perf_counter() - t0:.2f}s")


@pytest.mark.parametrize("name", gc.PAST_CAP)
def test_generic_gather_past_its_block_cap(dev, name):
    """2048 blocks x 4 waves x R rows and three more: every wave's second trip, most of them past the last row"""
    case = gc.CASE_BY_NAME[name]
    t0 = time.perf_counter()
    b = gc.past_cap_rows(case)
    la = _ring(dev, case).run(case, b, True, gc.CLAMP5)
    assert la.blocks == gc.GENERIC_MAX_BLOCKS and la.shape == case.shape and b == la.blocks * la.rows_blk + 3
    print(f"GATHER {name} past the cap: {b} rows {time.perf_counter() - t0:.2f}s")


@pytest.mark.parametrize("template", list(gc.REPRESENTATIVES))
def test_fused_gather_one_factor_at_a_time(dev, template):
    """On one representative per template: clamp off, PADS_ZERO, non-temporal loads, non-temporal stores, every rows-in-flight
    override, every destination subset the learners use (with and without PADS_ZERO)."""
    case = gc.CASE_BY_NAME[gc.REPRESENTATIVES[template]]
    t0 = time.perf_counter()
    ring = _ring(dev, case)
    runs = gc.factor_runs(case)
    for k, (what, flags, norm, dests) in enumerate(runs):
        la = ring.run(case, gc.factor_batch(case, flags), norm, flags, dests, seed=100 + k)
        assert la.template == template, what
    print(f"GATHER {template} on {case.name}: {len(runs)} factor launches {time.perf_counter() - t0:.2f}s")
