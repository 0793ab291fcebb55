"""pqlk_rollout_step, pqlk_nstep_push_emit and pqlk_rms_merge against the CPU models of tests/rollout_cases.py, at the edges
the tables there name: one env, one env on each side of a wave and of a 1024-env scan chunk, windows of 1, 7 and 100 slots
(some larger than N), steps where exactly win, win + 1 or win - 1 (wrapping) envs finish, all four (done, truncated) pairs in
one step, both copy paths of every field, the three copy loops past the 512-block cap; every window length of the n-step
assembler up to 16 through the raw C entry (n = 1 and calls that emit nothing included), from a count past 2^31; the statistics
merge over several blocks and past 2^24 samples.  The models, the tables and the checks are proved without a GPU in
tests/test_rollout_cases_cpu.py.

Everything is bit for bit; there are no tolerances.  Every written buffer has poison in front of it and behind it that must
come back intact (the poison behind a ring stands in for the kernel's discard slot), every input has slack of 1e6 (bytes: 1)
around it and must come back unchanged, and the state of a case is compared after every launch."""
import ctypes as C
import time

import numpy as np
import pytest
import torch

import rollout_cases as rc
from guarded import Guarded
from reduction_cases import IN_BIG, SLACK, T
from support import dev  # noqa: F401

pytestmark = pytest.mark.gpu

POISON = rc.POISON
PTR_FILL = 12345           # slack around the two window pointers
COUNTS = {"rollout-step launches": 0, "n-step calls": 0, "n-step launches": 0, "merge traces": 0, "merge launches": 0}


@pytest.fixture(scope="module", autouse=True)
def _launch_counts(dev):  # noqa: F811
    t0 = time.perf_counter()
    yield
    print(f"\n[rollout kernels] {', '.join(f'{v} {k}' for k, v in COUNTS.items())}; {time.perf_counter() - t0:.2f} s in all")


def _launched(rcode, what):
    from pql_amd import _lib as L
    if rcode < 0:      # a HIP error: nothing more may be started on this device
        pytest.exit(f"{what}: HIP error {rcode}", returncode=3)
    L.check(rcode)
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"{what}: {e}", returncode=3)


def _inputs(dev, arrays):
    """{name: Guarded} of read-only inputs: slack of IN_BIG (bytes: 1, which reads as done and as truncated) around them"""
    out = {}
    for k, a in arrays.items():
        if a is None:
            out[k] = None
        elif a.dtype == np.uint8:
            out[k] = Guarded(dev, a.shape, 1, init=a, off=SLACK, dtype=torch.uint8)
        else:
            out[k] = Guarded(dev, a.shape, IN_BIG, init=a, off=SLACK)
    return out


def _unchanged(bufs, arrays, what):
    for k, g in bufs.items():
        if g is not None:
            assert g.intact() and np.array_equal(g.t.cpu().numpy(), arrays[k]), f"{what}: input {k} or its slack changed"


# --------------------------------------------------------------------------- pqlk_rollout_step
@pytest.mark.parametrize("name", [c.name for c in rc.ROLLOUT_CASES])
def test_rollout_step_equals_the_model_after_every_launch(dev, name):
    """Slabs (with the untouched columns of other t), accumulators, both rings slot by slot (`ring[(ptr + i) % win] == deque[i]`)
    with the slot behind them, and both pointers, after every step of the case's script."""
    from pql_amd import _lib as L
    case = rc.ROLLOUT_BY_NAME[name]
    N, O, A, win, H = case.N, case.O, case.A, case.win, case.H
    t0 = time.perf_counter()
    model = rc.RolloutModel(case)
    G = lambda shape, **kw: Guarded(dev, shape, POISON, off=SLACK, **kw)      # noqa: E731
    slabs = {k: G((N, H, w)) for k, w in zip(rc.SLABS, (O, A, 1, O, 1))}
    cur = {k: G((N,), init=np.zeros(N, dtype=np.float32)) for k in ("cur_ret", "cur_len")}
    rings = {k: G((win,), init=np.zeros(win, dtype=np.float32)) for k in ("ring_ret", "ring_len")}      # exactly win floats
    ptrs = {k: Guarded(dev, (1,), PTR_FILL, init=np.array([p], dtype=np.int64), off=SLACK, dtype=torch.int64)
            for k, p in (("ptr_ret", model.ptr_ret), ("ptr_len", model.ptr_len))}
    written = {**slabs, **cur, **rings, **ptrs}
    launch = rc.rollout_launch(N, O, A)
    for i, step in enumerate(case.steps):
        what = f"{name} step {i} {step} [{launch.copy_blocks} copy blocks, trips {launch.trips_obs}/{launch.trips_act}/{launch.trips_rd}]"
        arrays = rc.rollout_inputs(case, i)
        inp = _inputs(dev, arrays)
        _launched(L.lib.pqlk_rollout_step(
            N, O, A, H, step.t, inp["obs"].ptr, inp["act"].ptr, inp["nobs"].ptr, inp["rew"].ptr, inp["done"].ptr,
            inp["trunc"].ptr if inp["trunc"] is not None else None, *[slabs[k].ptr for k in rc.SLABS], cur["cur_ret"].ptr,
            cur["cur_len"].ptr, rings["ring_ret"].ptr, rings["ring_len"].ptr, ptrs["ptr_ret"].ptr, ptrs["ptr_len"].ptr, win,
            L.stream(dev)), what)
        COUNTS["rollout-step launches"] += 1
        model.step(step.t, **arrays)
        got = {k: g.t.cpu().numpy() for k, g in {**slabs, **cur}.items()}
        for k, g in rings.items():       # the ring and the first float behind it: the slot at index win
            got[k] = g.full[g.off: g.off + win + 1].cpu().numpy()
        for k, g in ptrs.items():
            got[k] = int(g.t.item())
        rc.check_rollout(got, model.expected(), what)
        for k, g in written.items():
            assert g.intact(), f"{what}: slack around {k} was written"
        _unchanged(inp, arrays, what)
    print(f"\n[rollout step] {name}: N={N} O={O} A={A} win={win} H={H}, {len(case.steps)} launches, {time.perf_counter() - t0:.2f} s")


# --------------------------------------------------------------------------- pqlk_nstep_push_emit
@pytest.mark.parametrize("name", [c.name for c in rc.NSTEP_CASES])
def test_nstep_push_emit_equals_the_model_after_every_call(dev, name):
    """The raw C entry: a call that emits nothing (outputs NULL), two calls of one step, one of 2 n + 1 steps.  After each the
    row count, the emitted rows (outputs of exactly that many rows) and the whole window, pad words included, equal the model."""
    from pql_amd import _lib as L
    case = rc.NSTEP_BY_NAME[name]
    N, n, O, A = case.N, case.n, case.O, case.A
    t0 = time.perf_counter()
    model = rc.nstep_model(case)
    lay = model.L
    assert lay.ld == int(L.lib.pqlk_replay_rec_ld(O, A))
    window = Guarded(dev, (N, n, lay.ld), POISON, init=np.zeros((N, n, lay.ld), dtype=np.float32), off=SLACK)
    gp = (C.c_float * n)(*[float(g) for g in model.g])
    count, emitting = case.count0, 0
    for k, Tn in enumerate(rc.nstep_calls(n)):
        what = f"{name} call {k}: T={Tn} from count {count}"
        arrays = rc.nstep_inputs(case, k)
        inp = _inputs(dev, arrays)
        want, want_rows = model.call(**arrays)
        outs = {f: Guarded(dev, w.shape, POISON, off=SLACK) for f, w in want.items()} if want_rows else {}
        rows = C.c_int64(-1)
        _launched(L.lib.pqlk_nstep_push_emit(
            window.ptr, N, n, O, A, count, Tn, inp["obs"].ptr, inp["act"].ptr, inp["rew"].ptr, inp["nobs"].ptr, inp["done"].ptr, gp,
            *[outs[f].ptr if outs else None for f in rc.OUTS], C.byref(rows), L.stream(dev)), what)
        COUNTS["n-step calls"] += 1
        COUNTS["n-step launches"] += Tn
        emitting += want_rows > 0
        got = {f: g.t.cpu().numpy() for f, g in outs.items()} if outs else want
        rc.check_nstep(got, rows.value, window.t.cpu().numpy(), want, want_rows, model.window, lay, what)
        for f, g in {**outs, "window": window}.items():
            assert g.intact(), f"{what}: slack around {f} was written"
        _unchanged(inp, arrays, what)
        count += Tn
    assert emitting >= 1 and count == model.count
    print(f"\n[n-step] {name}: n={n} N={N} O={O} A={A} gamma={case.gamma}, {len(rc.nstep_calls(n))} calls ({emitting} emitting), "
          f"{time.perf_counter() - t0:.2f} s")


# --------------------------------------------------------------------------- pqlk_rms_merge
@pytest.mark.parametrize("cols", rc.RMS_COLS)
def test_rms_merge_equals_the_float32_expression_on_both_traces(dev, cols):
    """Five merges from count = 1e-4 and five from past 2^24 samples, where float(count) rounds, on one to three blocks."""
    from pql_amd import _lib as L
    t0 = time.perf_counter()
    for trace, count in enumerate(rc.RMS_STARTS):
        mean, var = rc.rms_start(cols, trace)
        for step, n in enumerate(rc.RMS_BATCHES):
            what = f"cols={cols} trace {trace} merge {step}: count={count!r} batch={n}"
            bm, bv = rc.rms_batch(cols, trace, step)
            arrays = dict(mean=mean, var=var, bm=bm, bv=bv)
            inp = _inputs(dev, arrays)
            out = {k: Guarded(dev, (cols,), POISON, off=SLACK) for k in ("mean", "var")}
            _launched(L.lib.pqlk_rms_merge(inp["mean"].ptr, inp["var"].ptr, inp["bm"].ptr, inp["bv"].ptr, float(count), float(n),
                                           float(count + n), cols, out["mean"].ptr, out["var"].ptr, L.stream(dev)), what)
            COUNTS["merge launches"] += 1
            mean, var, count = rc.rms_merge_ref(mean, var, bm, bv, count, n)
            for k, w in (("mean", mean), ("var", var)):
                g = out[k].t.cpu().numpy()
                bad = np.flatnonzero(rc.bits(g) != rc.bits(w))
                assert not len(bad), f"{what}: {k}: {len(bad)} columns differ, first {bad[0]}: got {g[bad[0]]!r}, want {w[bad[0]]!r}"
                assert out[k].intact(), f"{what}: slack around {k}_out was written"
            _unchanged(inp, arrays, what)
        COUNTS["merge traces"] += 1
    print(f"\n[rms merge] cols={cols}: 2 traces of {len(rc.RMS_BATCHES)} merges, {time.perf_counter() - t0:.2f} s")
