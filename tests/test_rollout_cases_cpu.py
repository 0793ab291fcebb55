"""tests/rollout_cases.py means what tests/test_rollout_kernels_gpu.py assumes: the three CPU models agree with independent
statements of the same laws (Tracker, the oracle's NStepRef, torch's own CPU row sum and expressions), the case tables reach the
edges they name (grid-stride second trips by the launch mirror, every scripted pattern, every (done, truncated) pair, every
window situation), the checks reject the wrong outputs they are there to catch, and the C entries refuse what they say they
refuse.  No GPU needed."""
import ctypes as C
from functools import lru_cache

import numpy as np
import pytest
import torch

import rollout_cases as rc
from reduction_cases import T

F32 = np.float32
E_SHAPE, E_UNSUPPORTED = 2, 5


@lru_cache(maxsize=None)
def _rollout_trace(name):
    """the model after every step of a case: [(inputs, expected outputs)] and the model"""
    case = rc.ROLLOUT_BY_NAME[name]
    m, out = rc.RolloutModel(case), []
    for i, step in enumerate(case.steps):
        inp = rc.rollout_inputs(case, i)
        m.step(step.t, **inp)
        out.append((inp, m.expected()))
    return out, m


@lru_cache(maxsize=None)
def _nstep_trace(name):
    """[(inputs, outputs, rows, window after the call)] of a case's calls and the model"""
    case = rc.NSTEP_BY_NAME[name]
    m, out = rc.nstep_model(case), []
    for k in range(len(rc.nstep_calls(case.n))):
        inp = rc.nstep_inputs(case, k)
        outs, rows = m.call(**inp)
        out.append((inp, outs, rows, m.window.copy()))
    return out, m


SMALL = [c.name for c in rc.ROLLOUT_CASES if not c.past_cap]


def _find_step(pred):
    """(case, step index, trace) of the first step of a small case that pred(case, step, log entry) accepts"""
    for name in SMALL:
        case = rc.ROLLOUT_BY_NAME[name]
        trace, m = _rollout_trace(name)
        for i, step in enumerate(case.steps):
            if pred(case, step, m.log[i]):
                return case, i, trace
    raise AssertionError("no such step in the tables")


# --------------------------------------------------------------------------- the models against independent statements
@pytest.mark.parametrize("name", SMALL)
def test_rollout_model_windows_are_the_trackers(name):
    """The model's deques against pql_amd.utils.common.Tracker fed the finished envs' values from a restatement in torch."""
    from pql_amd.utils.common import Tracker
    case = rc.ROLLOUT_BY_NAME[name]
    trace, _ = _rollout_trace(name)
    tr_ret, tr_len = Tracker(case.win), Tracker(case.win)
    cur_ret, cur_len = torch.zeros(case.N), torch.zeros(case.N)
    p_ret, p_len = 0, case.ptr_len0
    for (inp, want) in trace:
        cur_ret += T(inp["rew"]); cur_len += 1
        idx = torch.where(T(inp["done"]) != 0)[0]
        tr_ret.update(cur_ret[idx]); tr_len.update(cur_len[idx])
        cur_ret[idx] = 0; cur_len[idx] = 0
        p_ret, p_len = (p_ret + len(idx)) % case.win, (p_len + len(idx)) % case.win
        assert (want["ptr_ret"], want["ptr_len"]) == (p_ret, p_len)
        for ring, p, tr in ((want["ring_ret"], p_ret, tr_ret), (want["ring_len"], p_len, tr_len)):
            assert [ring[(p + i) % case.win] for i in range(case.win)] == [F32(v) for v in tr.moving_average]
            assert ring[case.win] == rc.POISON32
        assert np.array_equal(want["cur_ret"], cur_ret.numpy()) and np.array_equal(want["cur_len"], cur_len.numpy())


@pytest.mark.parametrize("name", [c.name for c in rc.NSTEP_CASES if c.count0 == 0 and c.n >= 2])
def test_nstep_fifo_model_is_the_oracles(name):
    """Every call of a case in one slab through oracle.pql_ref_cpu.NStepRef (which takes any n >= 2; n = 1 is a pass-through
    there): the same rows in the same order, bit for bit."""
    from oracle.pql_ref_cpu import NStepRef
    case = rc.NSTEP_BY_NAME[name]
    trace, _ = _nstep_trace(name)
    ref = NStepRef(case.O, case.A, case.N, case.n, case.gamma)
    slab = {k: T(np.concatenate([inp[k] for inp, *_ in trace], axis=1)) for k in ("obs", "act", "rew", "nobs", "done")}
    want = ref.add(slab["obs"], slab["act"], slab["rew"], slab["nobs"], slab["done"])
    assert np.array_equal(rc.gamma_pow(case.gamma, case.n), ref.gamma_pow.numpy())
    for k, w in zip(rc.OUTS, want):
        got = np.concatenate([outs[k] for _, outs, _, _ in trace])
        w = w.numpy().reshape(got.shape)
        assert np.array_equal(rc.bits(got), rc.bits(np.ascontiguousarray(w))), (name, k)
    assert sum(rows for *_, rows, _ in trace) == len(want[0])


def test_nstep_n1_is_the_pass_through():
    """n = 1: the rows are the inputs, time-major"""
    trace, _ = _nstep_trace("n1")
    for inp, outs, rows, _ in trace:
        N, Tn = inp["rew"].shape
        assert rows == N * Tn
        for k, f in zip(rc.OUTS, ("obs", "act", "rew", "nobs", "done")):
            assert np.array_equal(outs[k], np.swapaxes(inp[f], 0, 1).reshape(outs[k].shape))


@pytest.mark.parametrize("name", [c.name for c in rc.NSTEP_CASES])
def test_reward_sum_law_against_torch_and_float64(name):
    """n <= 5: the four-lane sum is torch's own CPU `(rew * gamma_pow * keep).sum(1)` on the case data.  n >= 6: it is a law of
    its own (test_four_lane_law_is_torchs_row_sum_up_to_n_5_only), held to the float64 sum within (n + 1) 2^-24 sum_j |r_j g_j|:
    one rounding of each product and fewer than n roundings of partial sums, each at most 2^-24 of a magnitude that
    sum_j |r_j g_j| (1 + 2^-24)^n bounds.  The sum runs over the kept terms; a masked term is an exact zero."""
    case = rc.NSTEP_BY_NAME[name]
    _, m = _nstep_trace(name)
    assert m.windows
    for rew_w, done_w in m.windows:
        terms, keep, _, _ = rc.reward_terms(rew_w, done_w, m.g)
        R = rc.reward_sum(terms)
        if case.n <= 5:
            want = (T(rew_w) * T(m.g) * T(keep)).sum(1).numpy()
            assert np.array_equal(rc.bits(R), rc.bits(want)), name
        else:
            exact = rew_w.astype(np.float64) * m.g.astype(np.float64)[None, :] * keep
            bound = (case.n + 1) * 2.0 ** -24 * np.abs(exact).sum(axis=1)
            assert (np.abs(R.astype(np.float64) - exact.sum(axis=1)) <= bound).all(), name


def test_four_lane_law_is_torchs_row_sum_up_to_n_5_only():
    """On 20000 rows per n: the four-lane order equals torch's CPU `.sum(1)` for n = 2..5, and from n = 5 on it is not left to
    right.  For n = 6..16 the same rows differ from torch's `.sum(1)` somewhere at every n (DESIGN.md records it); that half
    is a statement about torch's vectorised CPU kernels, not about this project, so it is not asserted: the kernel is held to
    the four-lane law for every n, and torch is its reference only where the two coincide."""
    import detdata as dd
    for n in range(2, 17):
        terms = dd.uniform((20000, n), 900 + n, -1, 1)
        lanes = rc.reward_sum(terms)
        if n <= 5:
            assert np.array_equal(lanes, T(terms).sum(1).numpy()), n
        assert np.array_equal(lanes, rc.reward_sum(terms, "ltr")) == (n <= 4), n


@pytest.mark.parametrize("cols", rc.RMS_COLS)
def test_rms_merge_expression_is_torchs(cols):
    """The float32 restatement against the reference's torch expression on the CPU with the same Python scalars, on both traces."""
    for trace, count in enumerate(rc.RMS_STARTS):
        mean, var = rc.rms_start(cols, trace)
        mean_t, var_t, count_t = T(mean), T(var), count
        for step, n in enumerate(rc.RMS_BATCHES):
            bm, bv = rc.rms_batch(cols, trace, step)
            mean, var, count = rc.rms_merge_ref(mean, var, bm, bv, count, n)
            delta = T(bm) - mean_t
            tot = count_t + n
            m2 = var_t * count_t + T(bv) * n + delta ** 2 * count_t * n / tot
            mean_t = mean_t + delta * n / tot
            var_t = m2 / tot
            count_t = tot
            assert count == count_t
            assert np.array_equal(rc.bits(mean), rc.bits(mean_t.numpy())) and np.array_equal(rc.bits(var), rc.bits(var_t.numpy())), (cols, trace, step)


def test_second_rms_trace_is_where_the_count_rounds():
    """from the start of the second trace on float(count) is not the count: the claim "rounded where torch rounds" is in play"""
    count = rc.RMS_STARTS[1]
    assert count > 2 ** 24
    rounded = []
    for n in rc.RMS_BATCHES:
        rounded.append(float(F32(count)) != count or float(F32(count + n)) != count + n)
        count += n
    assert all(rounded)
    count = rc.RMS_STARTS[0]
    for n in rc.RMS_BATCHES:       # the first trace stays where only the 1e-4 is lost
        count += n
        assert abs(float(F32(count)) - count) < 2e-4
    assert count < 2 ** 24


# --------------------------------------------------------------------------- the tables are what they claim
def test_launch_mirror_and_the_cases_past_the_copy_cap():
    la = rc.rollout_launch
    assert la(4096, 88, 16).copy_blocks == 192                          # the largest case of the older test stays under the cap
    assert la(1, 1, 1).copy_blocks == 1 and la(1, 1, 1).threads == 1024
    assert la(2056, 1024, 257).copy_blocks == rc.COPY_MAX_BLOCKS
    claimed = set()
    for case in rc.ROLLOUT_CASES:
        launch = la(case.N, case.O, case.A)
        for loop in case.past_cap:
            assert launch.copy_blocks == rc.COPY_MAX_BLOCKS or loop == "rd"
            assert rc.PAST_CAP_TRIPS[loop](launch) >= 2, (case.name, loop, launch)
            claimed.add(loop)
            # "one done pattern with many finished envs"
            _, m = _rollout_trace(case.name)
            assert max(total for _, total in m.log) > case.N // 5
        if not case.past_cap:
            assert max(launch.trips_obs, launch.trips_act, launch.trips_rd) == 1, case.name
    assert claimed == {"obs16", "act_scalar", "rd"}
    assert la(400000, 1, 1).chunks == 391 and la(400000, 1, 1).threads < 400000


def test_every_scripted_pattern_geometry_window_width_and_horizon_occurs():
    cases = rc.ROLLOUT_CASES
    scan = [c for c in cases if c.name.startswith("scan_")]
    assert [c.N for c in scan] == [1, 63, 64, 65, 1023, 1024, 1025, 2049] and all((c.O, c.A) == (8, 4) for c in scan)
    assert {c.win for c in scan} == {1, 7, 100} and any(c.win > c.N for c in scan)
    assert {(c.O, c.A) for c in cases} >= {(8, 4), (8, 3), (7, 4), (5, 3), (1, 1)}
    assert {c.H for c in cases} >= {1, 3}
    seen = set()
    for c in cases:
        seen |= {s.pattern for s in c.steps}
        assert all(0 <= s.t < c.H for s in c.steps)
        assert {s.t for s in c.steps} == set(range(c.H)), c.name               # every t of the horizon
        assert {s.trunc is None for s in c.steps} == {True, False} or len(c.steps) < 2, c.name
        assert c.ptr_len0 == 3 % c.win
    assert seen == set(rc.PATTERNS)
    # the patterns are what their names say, at the N where they are run
    for c in cases:
        _, m = _rollout_trace(c.name)
        for i, s in enumerate(c.steps):
            done = rc.rollout_inputs(c, i)["done"] != 0
            ptr, total = m.log[i]
            assert total == done.sum()
            want = {"none": 0, "first": 1, "last": 1, "wave": 2, "chunk": 2, "all": c.N, "win": c.win, "win+1": c.win + 1,
                    "wrap": c.win - 1}.get(s.pattern)
            assert want is None or total == want, (c.name, s)
            if s.pattern == "wave":
                assert list(np.flatnonzero(done)) == [63, 64]
            if s.pattern == "chunk":
                assert list(np.flatnonzero(done)) == [1023, 1024]
            if s.pattern == "first":
                assert done[0]
            if s.pattern == "last":
                assert done[c.N - 1]
            if s.pattern == "lastchunk":
                assert np.flatnonzero(done).min() == (c.N - 1) // 1024 * 1024 >= 1024 and total == c.N - (c.N - 1) // 1024 * 1024
            if s.pattern == "wrap":                                            # the appended run passes the end of the ring
                assert 0 < total < c.win and ptr + total > c.win, (c.name, s, ptr)
    # a step with total == win and one with total == win + 1 at every window length that N allows, N = 1 included in "all"
    for win in (1, 7, 100):
        pats = {s.pattern for c in scan if c.win == win for s in c.steps}
        assert {"win", "win+1"} <= pats, win
    assert any(c.N == 1 and {"none", "all"} <= {s.pattern for s in c.steps} for c in scan)


def test_every_done_truncated_pair_occurs_in_one_step():
    n_mixed = 0
    for c in rc.ROLLOUT_CASES:
        for i, s in enumerate(c.steps):
            inp = rc.rollout_inputs(c, i)
            assert (inp["trunc"] is None) == (s.trunc is None)
            if s.pattern != "mixed4":
                continue
            n_mixed += 1
            pairs = set(zip((inp["done"] != 0).tolist(), (inp["trunc"] != 0).tolist()))
            assert pairs == {(False, False), (False, True), (True, False), (True, True)}, c.name
            # done & truncated: out of done', into the windows
            _, want = _rollout_trace(c.name)[0][i]
            both = (inp["done"] != 0) & (inp["trunc"] != 0)
            assert both.any() and (want["s_done"][both, s.t, 0] == 0).all() and (want["cur_len"][both] == 0).all()
            assert set(np.unique(inp["done"])) > {0, 1} and set(np.unique(inp["trunc"])) > {0, 1}    # other non-zero bytes
    assert n_mixed >= len([c for c in rc.ROLLOUT_CASES if c.N >= 4])


def test_nstep_table_covers_the_lists_and_every_window_situation():
    cs = rc.NSTEP_CASES
    assert {c.n for c in cs} >= {1, 2, 5, 6, 8, 13, 16} and max(c.n for c in cs) == rc.MAX_NSTEP
    assert {c.N for c in cs} >= {1, 3, 4, 5, 257}
    assert {(c.O, c.A) for c in cs} >= {(1, 1), (63, 3), (64, 64), (65, 70), (130, 5)}
    assert {c.gamma for c in cs} == {0.99, 1.0}
    assert [c.count0 for c in cs if c.count0] == [2 ** 31 + 5]
    silent_first, emitting_second = 0, 0
    seen = {}
    for c in cs:
        calls = rc.nstep_calls(c.n)
        assert calls[-3:] == [1, 1, 2 * c.n + 1] and (len(calls) == 4) == (c.n >= 3) and (c.n < 3 or calls[0] == c.n - 2)
        trace, m = _nstep_trace(c.name)
        rows = [r for *_, r, _ in trace]
        first = max(c.n - 1 - c.count0, 0)
        count = c.count0
        for Tn, r in zip(calls, rows):                       # the host's count of emitted rows
            assert r == max(Tn - max(c.n - 1 - count, 0), 0) * c.N
            count += Tn
        silent_first += c.n >= 3 and rows[0] == 0 and first > 0
        emitting_second += rows[-3] > 0
        for inp, *_ in trace:
            assert set(np.unique(inp["done"])) <= {0.0, 1.0}
        for k in rc.SITUATIONS:
            seen[k] = seen.get(k, 0) + m.seen[k]
        if c.n >= 2 and c.count0 == 0:                       # env 0 of the last call alone brings every situation
            assert all(m.seen[k] > 0 for k in rc.SITUATIONS), (c.name, m.seen)
    assert silent_first >= 5 and emitting_second >= 2
    assert all(seen[k] > 0 for k in rc.SITUATIONS), seen
    # "two dones, where the first one counts": somewhere the first and the last done of a window are different steps
    _, m = _nstep_trace("n6")
    assert any(((d != 0).sum(1) >= 2).any() for _, d in m.windows)


# --------------------------------------------------------------------------- the checks fail on wrong outputs
def _rejected(want, what, **changed):
    got = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in want.items()}
    got.update(changed)
    rc.check_rollout({k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in want.items()}, want, what)   # the untouched copy passes
    with pytest.raises(AssertionError):
        rc.check_rollout(got, want, what)


def test_ring_values_one_slot_off_are_rejected_where_the_sorted_comparison_accepts():
    case, i, trace = _find_step(lambda c, s, log: s.pattern == "win" and c.win == 7)
    want = trace[i][1]
    ring = want["ring_ret"].copy()
    ring[:case.win] = np.roll(ring[:case.win], 1)
    assert len(set(want["ring_ret"][:case.win].tolist())) == case.win
    assert sorted(ring[:case.win].tolist()) == sorted(want["ring_ret"][:case.win].tolist())      # the old comparison
    _rejected(want, "one slot off", ring_ret=ring)


def test_swapped_neighbours_are_rejected():
    case, i, trace = _find_step(lambda c, s, log: s.pattern == "all" and c.win == 100 and c.N >= 100)
    want = trace[i][1]
    ring = want["ring_len"].copy()
    j = next(j for j in range(case.win - 1) if ring[j] != ring[j + 1])
    ring[[j, j + 1]] = ring[[j + 1, j]]
    _rejected(want, "swapped", ring_len=ring)
    ring = want["ring_ret"].copy()
    ring[[10, 11]] = ring[[11, 10]]
    assert ring[10] != ring[11]
    _rejected(want, "swapped", ring_ret=ring)


def test_pointer_advanced_by_min_total_win_is_rejected():
    case, i, trace = _find_step(lambda c, s, log: s.pattern == "win+1" and c.win == 7)
    want = trace[i][1]
    before = trace[i - 1][1]
    _rejected(want, "pointer", ptr_ret=(before["ptr_ret"] + case.win) % case.win)
    _rejected(want, "pointer", ptr_len=(before["ptr_len"] + case.win) % case.win)


def test_done_without_the_truncation_mask_is_rejected():
    case, i, trace = _find_step(lambda c, s, log: s.pattern == "mixed4")
    inp, want = trace[i]
    s_done = want["s_done"].copy()
    s_done[:, case.steps[i].t, 0] = (inp["done"] != 0).astype(F32)
    _rejected(want, "no mask", s_done=s_done)


def test_accumulator_not_reset_is_rejected():
    case, i, trace = _find_step(lambda c, s, log: s.pattern == "last" and c.N > 1 and log[0] >= 0)
    inp, want = trace[i]
    before = trace[i - 1][1]
    for k, add in (("cur_ret", inp["rew"]), ("cur_len", F32(1))):
        a = want[k].copy()
        a[case.N - 1] = (before[k] + add)[case.N - 1]
        assert a[case.N - 1] != 0
        _rejected(want, "no reset", **{k: a})


def test_write_into_the_slot_behind_the_ring_is_rejected():
    case, i, trace = _find_step(lambda c, s, log: s.pattern == "win+1")
    want = trace[i][1]
    for k in ("ring_ret", "ring_len"):
        ring = want[k].copy()
        ring[case.win] = ring[0]
        _rejected(want, "discard slot", **{k: ring})


def test_written_column_of_another_t_is_rejected():
    case, i, trace = _find_step(lambda c, s, log: c.H == 3)
    want = trace[i][1]
    assert i == 0 and (want["s_obs"][:, 1:] == rc.POISON32).all() and (want["s_rew"][:, 1:] == rc.POISON32).all()
    s_obs = want["s_obs"].copy()
    s_obs[0, 1, 0] = 0.0
    _rejected(want, "other column", s_obs=s_obs)


def _nstep_rejected(name, k, outs=None, window=None):
    case = rc.NSTEP_BY_NAME[name]
    trace, m = _nstep_trace(name)
    _, want_outs, rows, want_window = trace[k]
    rc.check_nstep(want_outs, rows, want_window, want_outs, rows, want_window, m.L, name)
    with pytest.raises(AssertionError):
        rc.check_nstep(want_outs if outs is None else outs, rows, want_window if window is None else window, want_outs, rows,
                       want_window, m.L, name)


def _wrong_model_outs(name, **kw):
    """the outputs of every call of a case under a wrong law"""
    case = rc.NSTEP_BY_NAME[name]
    m = rc.nstep_model(case, **kw)
    return [m.call(**rc.nstep_inputs(case, k))[0] for k in range(len(rc.nstep_calls(case.n)))]


def test_left_to_right_reward_sum_at_n_7_is_rejected():
    outs = _wrong_model_outs("n7_count_2p31", order="ltr")
    trace, _ = _nstep_trace("n7_count_2p31")
    k = len(outs) - 1
    assert (outs[k]["o_rew"] != trace[k][1]["o_rew"]).any() and all(np.array_equal(outs[k][f], trace[k][1][f]) for f in rc.OUTS if f != "o_rew")
    _nstep_rejected("n7_count_2p31", k, outs=outs[k])


def test_next_obs_of_the_last_done_is_rejected():
    outs = _wrong_model_outs("n6", pick="last")
    trace, _ = _nstep_trace("n6")
    k = len(outs) - 1
    assert (outs[k]["o_nobs"] != trace[k][1]["o_nobs"]).any() and np.array_equal(outs[k]["o_rew"], trace[k][1]["o_rew"])
    _nstep_rejected("n6", k, outs=outs[k])


def test_non_zero_pad_word_in_the_window_is_rejected():
    for name in ("n6", "n2"):
        trace, m = _nstep_trace(name)
        L = m.L
        pads = [c for c in range(L.ld) if not (c < L.O or L.off_nobs <= c < L.off_nobs + L.O or L.off_act <= c < L.off_act + L.A
                                               or c in (L.off_rd, L.off_rd + 1))]
        assert pads and (trace[-1][3][:, :, pads] == 0).all()
        for c in (pads[0], pads[-1]):
            w = trace[-1][3].copy()
            w[0, 1, c] = 1e-30
            _nstep_rejected(name, len(trace) - 1, window=w)


def test_env_major_rows_are_rejected():
    trace, _ = _nstep_trace("n6")
    case = rc.NSTEP_BY_NAME["n6"]
    k = len(trace) - 1
    want = trace[k][1]
    steps = trace[k][2] // case.N
    assert steps >= 2 and case.N >= 2
    outs = {f: v.copy() for f, v in want.items()}
    env_major = lambda v: np.swapaxes(v.reshape((steps, case.N) + v.shape[1:]), 0, 1).reshape(v.shape)      # noqa: E731
    outs["o_obs"] = env_major(want["o_obs"])
    _nstep_rejected("n6", k, outs=outs)
    # one row alone: row 1 (step 0, env 1) holds what belongs to (step 1, env 0)
    outs = {f: v.copy() for f, v in want.items()}
    outs["o_act"][1] = want["o_act"][case.N]
    _nstep_rejected("n6", k, outs=outs)


def test_wrong_row_count_is_rejected():
    trace, m = _nstep_trace("n6")
    _, outs, rows, window = trace[0]
    assert rows == 0
    with pytest.raises(AssertionError):
        rc.check_nstep(outs, -1, window, outs, rows, window, m.L, "rows")


# --------------------------------------------------------------------------- refusals of the C entries (no launch is made)
def test_c_entries_refuse_what_they_say():
    """0x1000 stands in for a device pointer: argument validation never dereferences it.  (NULL pointers, n = 0, t = horizon at
    a horizon of four and the alignment rule of pqlk_rollout_step are pinned in tests/test_host_cpu.py.)"""
    from pql_amd import _lib as L
    lib, P = L.lib, C.c_void_p(0x1000)
    gp = (C.c_float * 17)(*([1.0] * 17))
    rows = C.c_int64(-1)
    nstep = lambda n: lib.pqlk_nstep_push_emit(P, 4, n, 8, 2, 0, 1, P, P, P, P, P, gp, P, P, P, P, P, C.byref(rows), None)   # noqa: E731
    assert nstep(0) == E_UNSUPPORTED and nstep(17) == E_UNSUPPORTED and nstep(-1) == E_UNSUPPORTED
    assert rows.value == -1
    roll = lambda horizon, t, win: lib.pqlk_rollout_step(16, 8, 2, horizon, t, P, P, P, P, P, None, P, P, P, P, P, P, P, P, P, P, P,   # noqa: E731
                                                          win, None)
    assert roll(1, 1, 100) == E_SHAPE and roll(3, 3, 100) == E_SHAPE and roll(3, -1, 100) == E_SHAPE     # t >= horizon, t < 0
    assert roll(3, 0, 0) == E_SHAPE and roll(3, 0, -1) == E_SHAPE                                        # win_len
    merge = lambda cols, total: lib.pqlk_rms_merge(P, P, P, P, 1.0, 1.0, total, cols, P, P, None)        # noqa: E731
    assert merge(0, 2.0) == E_SHAPE and merge(-1, 2.0) == E_SHAPE and merge(8, 0.0) == E_SHAPE
