"""Cases, CPU models and checks for the actor-side kernels: pqlk_rollout_step and pqlk_rms_merge (pql_amd/csrc/rollout.hip) and
pqlk_nstep_push_emit (pql_amd/csrc/nstep.hip).

Plain numpy and the standard library: no torch device, no library.  tests/test_rollout_cases_cpu.py proves the models against
independent statements (Tracker, the oracle's NStepRef, torch's CPU row sum and expressions), proves that the tables reach what
they say they reach, and shows the checks failing on wrong outputs; tests/test_rollout_kernels_gpu.py runs the kernels.

The laws, all compared bit for bit:
  rollout step   r = cur_ret + rew, l = cur_len + 1 (float32); finished = done != 0; the two windows are `deque(maxlen=win)`
                 extended with r[finished], l[finished] in env order; the finished envs' accumulators become 0;
                 ptr' = (ptr + finished.sum()) % win; ring[(ptr' + i) % win] == deque[i]; slab column t = obs, act, rew, nobs and
                 done & ~truncated as 0.0 / 1.0; the other columns, and the slot behind each ring, are untouched.
  n-step         rows of the last n steps, oldest first: any = any(done_j != 0), first = first index of the largest done_j;
                 R = four partial sums over j mod 4 of (r_j * g_j) * keep_j, then ((A0 + A1) + A2) + A3, keep_j = not any or
                 j <= first, g_j = gamma ** j in double rounded once; obs, act of the oldest step; next_obs of step `first` if
                 any, else of the newest; done = 1 if any else the newest done.  Rows are time-major blocks of N.  The window
                 holds the record of step s in slot s % n of its env, in the ring's record layout, pad words 0.0.
  rms merge      Chan's merge as k_rms_merge states it, the three Python scalars rounded to float32 before use."""
from collections import Counter, deque, namedtuple

import numpy as np

import detdata as dd
from gather_cases import POISON as POISON32, bits, rec_layout

F32 = np.float32
# What every output holds before a call, and the slack around it: gather_cases' -777.25.  (reduction_cases' 5.0 is an episode
# length here: a stray write of a five-step episode into the slot behind the length window would not show.)
POISON = float(POISON32)

# --------------------------------------------------------------------------- host launch arithmetic of pqlk_rollout_step
COPY_MAX_BLOCKS = 512      # cap of the copy grid (blocks 1 .. copy_blocks; block 0 keeps the books)
BLOCK = 1024               # threads per block, and envs per chunk of block 0's scan
RolloutLaunch = namedtuple("RolloutLaunch", "copy_blocks threads trips_obs trips_act trips_rd vec_obs vec_act chunks")


def copy_items(n, w):
    """loop length of copy_rows: 16-byte lanes when the width is a multiple of four floats, else floats"""
    return n * (w >> 2) if w % 4 == 0 else n * w


def rollout_launch(n, O, A):
    """the copy grid and the trips the longest-running thread of each of its three loops takes"""
    copy_blocks = (n * (2 * O + A) // 4 + 1023) // 1024
    copy_blocks = min(max(copy_blocks, 1), COPY_MAX_BLOCKS)
    threads = BLOCK * copy_blocks
    trips = lambda items: (items + threads - 1) // threads      # noqa: E731
    return RolloutLaunch(copy_blocks, threads, trips(copy_items(n, O)), trips(copy_items(n, A)), trips(n), O % 4 == 0, A % 4 == 0,
                         (n + BLOCK - 1) // BLOCK)


# --------------------------------------------------------------------------- the rollout-step cases
PATTERNS = ("none", "first", "last", "wave", "chunk", "lastchunk", "wrap", "win", "win+1", "all", "mixed4", "random")


def spread(N, k):
    """k distinct envs in env order, env 0 among them"""
    return (np.arange(k, dtype=np.int64) * N) // k


def applicable(name, N, win):
    return {"wave": N >= 65, "chunk": N >= 1025, "lastchunk": N > BLOCK, "wrap": win >= 3 and N >= win - 1, "win": N >= win,
            "win+1": N >= win + 1, "mixed4": N >= 4}.get(name, True)


def done_pattern(name, N, win, seed):
    """the finished envs of one scripted step, as booleans"""
    d = np.zeros(N, dtype=bool)
    if name == "first":
        d[0] = True
    elif name == "last":
        d[N - 1] = True
    elif name == "wave":                       # one env on each side of the first wave boundary
        d[[63, 64]] = True
    elif name == "chunk":                      # one env on each side of the first 1024-env chunk boundary
        d[[1023, 1024]] = True
    elif name == "lastchunk":                  # every env of the last chunk and nobody else
        d[(N - 1) // BLOCK * BLOCK:] = True
    elif name == "all":
        d[:] = True
    elif name in ("win", "win+1", "wrap"):     # exactly win, win + 1, win - 1 envs
        d[spread(N, win + {"win": 0, "win+1": 1, "wrap": -1}[name])] = True
    elif name == "mixed4":                     # with truncated = bit 1 of the env index: all four (done, truncated) pairs
        d = np.arange(N) % 2 == 1
    elif name == "random":
        d = dd.bernoulli((N,), seed, 0.3) > 0
    else:
        assert name == "none", name
    return d


Step = namedtuple("Step", "t pattern trunc")       # trunc: None (NULL pointer), "hash" (three envs in ten), "mixed4"
RolloutCase = namedtuple("RolloutCase", "name cid N O A win H ptr_len0 steps past_cap")


def _seed(cid, i):
    return 100000 * (cid + 1) + 100 * i


def _script(cid, N, win, H, patterns):
    """The steps of one case: the applicable patterns in order, t cycling through the horizon, every other step without a
    truncation vector.  In front of "wrap" as many "first" steps as it takes to bring the return window's pointer to 2 or more, so
    that the win - 1 appended values run past the end of the ring."""
    steps, ptr = [], 0

    def add(p):
        nonlocal ptr
        i = len(steps)
        steps.append(Step(i % H, p, "mixed4" if p == "mixed4" else (None if i % 2 == 0 else "hash")))
        ptr = (ptr + int(done_pattern(p, N, win, _seed(cid, i)).sum())) % win

    for p in patterns:
        if not applicable(p, N, win):
            continue
        while p == "wrap" and ptr < 2:
            add("first")
        add(p)
    return tuple(steps)


def _rollout_cases():
    out = []

    def case(name, N, O, A, win, H, patterns, past_cap=()):
        cid = len(out)
        # the two windows have pointers of their own: the length window starts at another slot than the return window
        out.append(RolloutCase(name, cid, N, O, A, win, H, 3 % win, _script(cid, N, win, H, patterns), tuple(past_cap)))

    # scan geometry: one env, one env on each side of a wave and of a 1024-env chunk, three chunks; win 1, 7, 100, two of them
    # larger than N; a horizon of one where t = 0 is the only column, else every t of three
    for N, win in zip((1, 63, 64, 65, 1023, 1024, 1025, 2049), (7, 100, 1, 7, 100, 1, 7, 100)):
        case(f"scan_{N}", N, 8, 4, win, 1 if N in (1, 64) else 3, PATTERNS + ("none",))
    # both copy paths for each field, and their mixtures
    for O, A in ((8, 3), (7, 4), (5, 3), (1, 1)):
        case(f"width_{O}_{A}", 130, O, A, 7, 3, ("random", "mixed4", "all"))
    # past the cap of the copy grid, shapes from rollout_launch: 2056 * 1024 / 4 and 2056 * 257 are both above 512 * 1024 ...
    case("cap_copy", 2056, 1024, 257, 100, 2, ("random", "all", "mixed4"), ("obs16", "act_scalar"))
    # ... and 400000 envs are more than the 293 * 1024 threads their three columns get; block 0 scans 391 chunks
    case("cap_rd", 400000, 1, 1, 100, 2, ("random", "lastchunk", "mixed4"), ("rd",))
    return out


ROLLOUT_CASES = _rollout_cases()
ROLLOUT_BY_NAME = {c.name: c for c in ROLLOUT_CASES}
assert len(ROLLOUT_BY_NAME) == len(ROLLOUT_CASES)
PAST_CAP_TRIPS = {"obs16": lambda la: la.trips_obs if la.vec_obs else 0, "act_scalar": lambda la: 0 if la.vec_act else la.trips_act,
                  "rd": lambda la: la.trips_rd}


def rollout_inputs(case, i):
    """the inputs of step i: obs, act, nobs (N, .), rew (N), done and trunc as bytes (trunc None = a NULL pointer).  The mixed4
    step marks some finished envs with 255 and some truncated ones with 2: any non-zero byte counts."""
    N, O, A = case.N, case.O, case.A
    s, step = _seed(case.cid, i), case.steps[i]
    done = done_pattern(step.pattern, N, case.win, s).astype(np.uint8)
    trunc = None
    if step.trunc == "hash":
        trunc = (dd.bernoulli((N,), s + 5, 0.3) > 0).astype(np.uint8)
    elif step.trunc == "mixed4":
        e = np.arange(N)
        trunc = ((e >> 1) & 1).astype(np.uint8)
        done[e % 8 == 3] = 255
        trunc[e % 8 == 6] = 2
    return dict(obs=dd.uniform((N, O), s + 1, -2, 2), act=dd.uniform((N, A), s + 2, -1, 1), nobs=dd.uniform((N, O), s + 3, -2, 2),
                rew=dd.uniform((N,), s + 4, -1, 1), done=done, trunc=trunc)


SLABS = ("s_obs", "s_act", "s_rew", "s_nobs", "s_done")


def ring_of(dq, ptr, win):
    """the ring a deque stands for, by slot: ring[(ptr + i) % win] == deque[i]; the slot at index win keeps its poison"""
    ring = np.full(win + 1, POISON32, dtype=F32)
    assert len(dq) == win
    for i, v in enumerate(dq):
        ring[(ptr + i) % win] = F32(v)
    return ring


class RolloutModel:
    """One state under pqlk_rollout_step calls (pql_actor.py:104-114, :129-135 and common.py:195-202 of the reference)."""

    def __init__(self, case):
        N, win = case.N, case.win
        self.case = case
        self.slabs = {k: np.full((N, case.H, w), POISON32, dtype=F32) for k, w in zip(SLABS, (case.O, case.A, 1, case.O, 1))}
        self.cur_ret, self.cur_len = np.zeros(N, dtype=F32), np.zeros(N, dtype=F32)
        self.dq_ret, self.dq_len = deque([0.0] * win, maxlen=win), deque([0.0] * win, maxlen=win)
        self.ptr_ret, self.ptr_len = 0, case.ptr_len0
        self.log = []              # (pointer of the return window before the step, finished envs) per step

    def step(self, t, obs, act, nobs, rew, done, trunc):
        win = self.case.win
        r = (self.cur_ret + rew).astype(F32)
        l = (self.cur_len + F32(1)).astype(F32)
        fin = done != 0
        self.dq_ret.extend(r[fin].tolist())
        self.dq_len.extend(l[fin].tolist())
        self.cur_ret, self.cur_len = np.where(fin, F32(0), r), np.where(fin, F32(0), l)
        total = int(fin.sum())
        self.log.append((self.ptr_ret, total))
        self.ptr_ret, self.ptr_len = (self.ptr_ret + total) % win, (self.ptr_len + total) % win
        s = self.slabs
        s["s_obs"][:, t], s["s_act"][:, t], s["s_rew"][:, t, 0], s["s_nobs"][:, t] = obs, act, rew, nobs
        s["s_done"][:, t, 0] = (fin & ~(trunc != 0) if trunc is not None else fin).astype(F32)

    def expected(self):
        """every output after the steps so far; ring_ret / ring_len are win + 1 floats, the last one the untouched slot behind"""
        win = self.case.win
        out = {k: v.copy() for k, v in self.slabs.items()}
        out.update(cur_ret=self.cur_ret.copy(), cur_len=self.cur_len.copy(), ring_ret=ring_of(self.dq_ret, self.ptr_ret, win),
                   ring_len=ring_of(self.dq_len, self.ptr_len, win), ptr_ret=self.ptr_ret, ptr_len=self.ptr_len)
        return out


def _first_difference(g, w):
    bad = np.argwhere(bits(g) != bits(w))
    if not len(bad):
        return None
    at = tuple(int(v) for v in bad[0])
    return len(bad), at, g[at], w[at]


def check_rollout(got, want, what):
    """every output of a rollout step equals the model bit for bit: slabs with their untouched columns, accumulators, the two
    rings slot by slot with the slot behind them, the two pointers"""
    assert set(got) == set(want), (what, sorted(got), sorted(want))
    for k in ("ptr_ret", "ptr_len"):
        assert int(got[k]) == want[k], f"{what}: {k} is {int(got[k])}, want {want[k]}"
    for k, w in want.items():
        if k.startswith("ptr_"):
            continue
        g = np.asarray(got[k])
        assert g.shape == w.shape and g.dtype == F32, (what, k, g.shape, w.shape, g.dtype)
        d = _first_difference(g, w)
        if d:
            where = "the slot behind the ring" if k.startswith("ring_") and d[1][0] == len(w) - 1 else f"index {d[1]}"
            raise AssertionError(f"{what}: {k}: {d[0]} elements differ, first at {where}: got {d[2]!r}, want {d[3]!r}")


# --------------------------------------------------------------------------- the n-step assembler
MAX_NSTEP = 16
OUTS = ("o_obs", "o_act", "o_rew", "o_nobs", "o_done")
SITUATIONS = ("none", "oldest", "newest_only", "two")


def gamma_pow(gamma, n):
    """gamma ** j in Python double, rounded once to float32"""
    return np.array([float(gamma) ** j for j in range(n)], dtype=np.float64).astype(F32)


def reward_terms(rew_w, done_w, g):
    """(r_j * g_j) * keep_j in float32 and keep, any, first of the (rows, n) windows, oldest step first"""
    n = rew_w.shape[1]
    anyd = (done_w != 0).any(axis=1)
    first = (done_w == done_w.max(axis=1, keepdims=True)).argmax(axis=1)       # first index of the largest entry
    keep = np.where(anyd[:, None], np.arange(n)[None, :] <= first[:, None], True).astype(F32)
    terms = ((rew_w * g[None, :]).astype(F32) * keep).astype(F32)
    return terms, keep, anyd, first


def reward_sum(terms, order="lanes4"):
    """lanes4: four partial sums over j mod 4, then ((A0 + A1) + A2) + A3 -- the kernel's law for every n up to 16.
    ltr: plain left to right (what the law is NOT from n = 5 on)."""
    n = terms.shape[1]
    if order == "ltr":
        R = terms[:, 0]
        for j in range(1, n):
            R = (R + terms[:, j]).astype(F32)
        return R
    assert order == "lanes4"
    lanes = [None] * 4
    for j in range(n):
        lanes[j % 4] = terms[:, j] if lanes[j % 4] is None else (lanes[j % 4] + terms[:, j]).astype(F32)
    R = lanes[0]
    for a in lanes[1:]:
        if a is not None:
            R = (R + a).astype(F32)
    return R


def situations(done_w):
    """which of the window situations each (row of) done window is in"""
    nz = done_w != 0
    return {"none": ~nz.any(axis=1), "oldest": nz[:, 0], "newest_only": nz[:, -1] & ~nz[:, :-1].any(axis=1), "two": nz.sum(axis=1) >= 2}


def emit_rows(w, g, order="lanes4", pick="first"):
    """The emitted rows of the windows w = (obs, act, rew, nobs, done), each (N, n, .) with the oldest step first.
    pick="last" takes next_obs at the LAST done (a wrong law, for the CPU test)."""
    obs_w, act_w, rew_w, nobs_w, done_w = w
    N, n = rew_w.shape
    terms, _, anyd, first = reward_terms(rew_w, done_w, g)
    sel = first
    if pick == "last":
        sel = n - 1 - (done_w[:, ::-1] != 0).argmax(axis=1)
    sel = np.where(anyd, sel, n - 1)
    return {"o_obs": obs_w[:, 0].copy(), "o_act": act_w[:, 0].copy(), "o_rew": reward_sum(terms, order),
            "o_nobs": nobs_w[np.arange(N), sel].copy(), "o_done": np.where(anyd, F32(1), done_w[:, -1]).astype(F32)}


class NStepModel:
    """pqlk_nstep_push_emit in two independent halves: a FIFO of the last n steps for the emitted rows, and the window by slot.
    A model that starts at count > 0 starts, like the kernel on a zeroed window, with min(count, n - 1) all-zero steps behind it."""

    def __init__(self, N, n, O, A, gamma, count=0, order="lanes4", pick="first"):
        self.N, self.n, self.O, self.A, self.count = N, n, O, A, count
        self.g, self.order, self.pick = gamma_pow(gamma, n), order, pick
        self.L = rec_layout(O, A)
        self.window = np.zeros((N, n, self.L.ld), dtype=F32)
        zero = tuple(np.zeros((N,) + s, dtype=F32) for s in ((O,), (A,), (), (O,), ()))
        self.fifo = [zero] * min(count, n - 1)
        self.seen = Counter()      # window situations over everything emitted
        self.windows = []          # (rew, done) windows of every emitting step, for the CPU test

    def call(self, obs, act, rew, nobs, done):
        """(N, T, .) slabs in; the five outputs of `rows` rows, time-major"""
        T = rew.shape[1]
        L, n = self.L, self.n
        blocks = []
        for t in range(T):
            step = (obs[:, t], act[:, t], rew[:, t], nobs[:, t], done[:, t])
            # the slot model: step s goes to slot s % n of its env, pad words zero
            rec = np.zeros((self.N, L.ld), dtype=F32)
            rec[:, :self.O], rec[:, L.off_nobs: L.off_nobs + self.O] = step[0], step[3]
            rec[:, L.off_act: L.off_act + self.A], rec[:, L.off_rd], rec[:, L.off_rd + 1] = step[1], step[2], step[4]
            self.window[:, (self.count + t) % n] = rec
            # the FIFO model
            self.fifo = (self.fifo + [step])[-n:]
            if len(self.fifo) == n:
                w = tuple(np.stack([s[k] for s in self.fifo], axis=1) for k in range(5))
                blocks.append(emit_rows(w, self.g, self.order, self.pick))
                self.windows.append((w[2], w[4]))
                for k, v in situations(w[4]).items():
                    self.seen[k] += int(v.sum())
        self.count += T
        shapes = {"o_obs": (0, self.O), "o_act": (0, self.A), "o_rew": (0,), "o_nobs": (0, self.O), "o_done": (0,)}
        outs = {k: (np.concatenate([b[k] for b in blocks]) if blocks else np.zeros(shapes[k], dtype=F32)) for k in OUTS}
        return outs, len(blocks) * self.N


NStepCase = namedtuple("NStepCase", "name n N O A gamma count0")
# every n, N, width and gamma of the issue at least once; the calls of a case are nstep_calls(n)
NSTEP_CASES = [
    NStepCase("n1", 1, 5, 63, 3, 0.99, 0), NStepCase("n2", 2, 4, 1, 1, 1.0, 0), NStepCase("n5", 5, 257, 64, 64, 0.99, 0),
    NStepCase("n6", 6, 3, 65, 70, 0.99, 0), NStepCase("n8", 8, 1, 130, 5, 1.0, 0), NStepCase("n13", 13, 257, 1, 1, 0.99, 0),
    NStepCase("n16", 16, 5, 65, 70, 0.99, 0),
    NStepCase("n7_count_2p31", 7, 5, 63, 3, 0.99, 2 ** 31 + 5),     # a zeroed window far into a run: every call emits
]
NSTEP_BY_NAME = {c.name: c for c in NSTEP_CASES}


def nstep_calls(n):
    """T of the calls of one case: n - 2 steps (emits nothing from count 0), one step, one step, then 2 n + 1"""
    return ([n - 2] if n >= 3 else []) + [1, 1, 2 * n + 1]


def nstep_inputs(case, k):
    """the (N, T, .) slabs of call k.  done is 0.0 / 1.0, three in ten; in the last call env 0 is scripted: done at t = 0, 1 and 2 n
    only, so that (n >= 2) the window emitted at t = 1 holds two dones, the one at t = n its done in the oldest slot, those from
    t = n + 1 to 2 n - 1 none, and the last one a done in the newest slot only."""
    calls = nstep_calls(case.n)
    T, N, O, A = calls[k], case.N, case.O, case.A
    s = 7000 * case.n + 100 * k + N
    done = dd.bernoulli((N, T), s + 5, 0.3)
    if k == len(calls) - 1:
        done[0, :] = 0.0
        done[0, [0, 1, 2 * case.n]] = 1.0
    return dict(obs=dd.uniform((N, T, O), s + 1, -2, 2), act=dd.uniform((N, T, A), s + 2, -1, 1), rew=dd.uniform((N, T), s + 3, -1, 1),
                nobs=dd.uniform((N, T, O), s + 4, -2, 2), done=done)


def nstep_model(case, **kw):
    return NStepModel(case.N, case.n, case.O, case.A, case.gamma, case.count0, **kw)


def check_nstep(got_outs, got_rows, got_window, want_outs, want_rows, want_window, L, what):
    """the row count, the emitted rows and the whole window (pad words included) equal the model bit for bit"""
    assert int(got_rows) == want_rows, f"{what}: rows_out is {int(got_rows)}, want {want_rows}"
    assert set(got_outs) == set(want_outs), (what, sorted(got_outs), sorted(want_outs))
    for k, w in want_outs.items():
        g = np.asarray(got_outs[k])
        assert g.shape == w.shape and g.dtype == F32, (what, k, g.shape, w.shape, g.dtype)
        d = _first_difference(g, w)
        if d:
            raise AssertionError(f"{what}: {k}: {d[0]} elements differ, first at {d[1]} (row = emitting step * N + env): "
                                 f"got {d[2]!r}, want {d[3]!r}")
    g = np.asarray(got_window)
    assert g.shape == want_window.shape and g.dtype == F32, (what, g.shape, want_window.shape)
    d = _first_difference(g, want_window)
    if d:
        c = d[1][2]
        field = ("obs" if c < L.O else "next_obs" if L.off_nobs <= c < L.off_nobs + L.O else "act" if L.off_act <= c < L.off_act + L.A
                 else "reward" if c == L.off_rd else "done" if c == L.off_rd + 1 else "pad word")
        raise AssertionError(f"{what}: window: {d[0]} words differ, first at (env, slot, word) {d[1]} ({field}): got {d[2]!r}, want {d[3]!r}")


# --------------------------------------------------------------------------- the statistics merge
RMS_COLS = (1, 255, 256, 257, 600)                 # one block of 256 threads, its last thread, and a second and third block
RMS_BATCHES = (131072, 4096, 1, 4096, 4096)
RMS_STARTS = (1e-4, 2 ** 24 + 4096 * 3 + 1e-4)     # the second: past 2^24 samples, where float(count) rounds


def rms_merge_ref(mean, var, bm, bv, count, batch_count):
    """RunningMeanStd.update_from_moments (torch_util.py:91-103 of the reference) as k_rms_merge states it: count, batch_count and
    their double sum each rounded to float32, then float32 operations in the kernel's order.  Returns mean', var', count'."""
    tot = count + batch_count
    c, b, t = F32(count), F32(batch_count), F32(tot)
    delta = (bm - mean).astype(F32)
    m2 = ((var * c).astype(F32) + (bv * b).astype(F32)).astype(F32) + ((((delta * delta).astype(F32) * c).astype(F32) * b).astype(F32) / t).astype(F32)
    return (mean + ((delta * b).astype(F32) / t).astype(F32)).astype(F32), (m2.astype(F32) / t).astype(F32), tot


def rms_start(cols, trace):
    if trace == 0:
        return np.zeros(cols, dtype=F32), np.ones(cols, dtype=F32)
    return dd.uniform((cols,), 640 + cols, -1, 1), dd.uniform((cols,), 641 + cols, 0.1, 3.0)


def rms_batch(cols, trace, step):
    s = 650 + 20 * trace + 2 * step + 1000 * cols
    return dd.uniform((cols,), s, -1, 1), dd.uniform((cols,), s + 1, 0.1, 3.0)
