"""Cases, CPU reference and checks for the replay ring kernels of pql_amd/csrc/replay.hip: insert, plain gather and the fused
gather (sample + normalise + clamp + concat), whose ten kernel templates and 58 instantiations are all chosen on the host.

Plain numpy plus detdata: no torch device, no library.  tests/test_gather_cases_cpu.py proves the layout mirror against the
library, the dispatch mirror against a literal list of the instantiations, and that the checks fail on wrong outputs;
tests/test_gather_kernels_gpu.py runs the kernels.

The record law, from host copies of the inserted rows (never from reading the ring back):
    src    = idx if 0 <= idx < capacity else 0
    x_sa   = [norm(obs[src]) | act[src] | pad]            obs-only ring: [norm(obs[src]) | 0 ...]
    xn_sa  = [norm(next_obs[src]) | untouched | pad]
    xn_obs = [norm(next_obs[src]) | pad]                  obs-only ring: [norm(obs[src]) | pad]
    rew    = rew[src],  done = 1.0 if done[src] != 0 else 0.0
    norm(x) = (x - mean) / sqrt(var + eps) in float32 (eps rounded to float32 first), then the +-5 clamp when bit 0 is set
    pad = 0, or untouched under PADS_ZERO;  an fp16 ring holds x.astype(float16).astype(float32) in its two observation fields.
Everything is compared bit for bit.  The clamped cases hold no NaN: the kernels' fminf(fmaxf(.)) turns a NaN into -5 where
torch.clamp keeps it, and nothing here asserts that either way."""
from collections import namedtuple
from functools import lru_cache

import numpy as np

import detdata as dd

F32, F16 = 0, 1                                              # PQLK_OBS_F32 / PQLK_OBS_F16
DT = {F32: "f32", F16: "f16"}
CLAMP5, PADS_ZERO, NT_LOADS, NT_STORES = 1, 2, 4, 8          # PQLK_GATHER_* (include/pqlk.h)
GATHER_MAX_OBS = 1024      # widest observation the kernels normalise
MAX_CHUNKS = 1024          # 16-B chunks of the largest record the fused gather takes
GENERIC_MAX_BLOCKS = 2048  # block cap of the generic kernels
DESTS = ("x_sa", "xn_sa", "xn_obs", "rew", "done")

POISON = np.float32(-777.25)   # what every destination holds before a call: "untouched" means these bits
GUARD_ROWS = 2                 # rows of poison behind row b - 1 of every destination
EPS = 1e-4
CAP, START = 211, 150          # ring rows; the fill starts at START and wraps: two segments, every row written
TRIPWIRE = 3                   # ring row whose index fills the slack around the index vector


def ROWS_IN_FLIGHT(r):
    return (r & 15) << 8


def WAVES_PER_CU(w):
    return (w & 63) << 12


def ld(cols):
    """pqlk_ld"""
    return (max(cols, 1) + 31) // 32 * 32


# --------------------------------------------------------------------------- record layouts (pqlk_common.h), offsets in 4-byte words
Layout = namedtuple("Layout", "O A dtype field off_nobs off_act off_rd used ld")


def rec_layout(O, A):
    o4 = (O + 3) & ~3
    if A < 0:
        off_nobs = off_act = off_rd = used = o4
    else:
        off_nobs, off_act, off_rd = o4, 2 * o4, 2 * o4 + ((A + 3) & ~3)
        used = off_rd + 4
    return Layout(O, A, F32, o4, off_nobs, off_act, off_rd, used, (used + 31) & ~31)


def rec_layout_h(O, A):
    oh = ((O + 7) & ~7) >> 1
    if A < 0:
        off_nobs = off_act = off_rd = used = oh
    else:
        off_nobs, off_act, off_rd = oh, 2 * oh, 2 * oh + ((A + 3) & ~3)
        used = off_rd + 4
    return Layout(O, A, F16, oh, off_nobs, off_act, off_rd, used, (used + 31) & ~31)


def layout(O, A, dtype):
    return rec_layout(O, A) if dtype == F32 else rec_layout_h(O, A)


# --------------------------------------------------------------------------- host dispatch of pqlk_replay_gather_fused
# template: the kernel's name without "k_replay_gather_"; shape: R of a lean kernel, (R, CH) of a generic one; variant: the
# argument the launch fixes at run time -- halves (fast), lgp (obs), ring kind (generic).  blocks and rows_blk (rows one block
# takes per trip) are the launch geometry.  Every destination is taken to be 16-byte aligned.
Launch = namedtuple("Launch", "template norm shape variant blocks rows_blk")
TRANSITION, OBS_ONLY = "transition", "obs-only"


def gather_launch(O, A, dtype, ld_sa, ld_o, flags, b, destinations, norm=True):
    L = layout(O, A, dtype)
    nchunk = L.used >> 2
    assert b > 0 and nchunk <= MAX_CHUNKS and (not norm or O <= GATHER_MAX_OBS) and (A >= 0 or "xn_sa" not in destinations)
    write_pads = not (flags & PADS_ZERO)
    tune_R, tune_wpc = (flags >> 8) & 15, (flags >> 12) & 63
    x_sa, xn_obs = "x_sa" in destinations, "xn_obs" in destinations
    narrow = dtype == F16 and (L.used >> 1) <= 64
    suffix = "" if dtype == F32 else ("_h8" if narrow else "_f16")
    fast = A >= 0 and nchunk <= 128 and (not write_pads or (ld_sa - O - A <= 64 and (not xn_obs or ld_o - O <= 64)))
    if fast:
        R = tune_R if tune_R in (1, 2, 4, 8) else 2
        halves = 2 if nchunk > 64 else 1
        rows_blk = 4 // halves * R
        blocks = min((b + rows_blk - 1) // rows_blk, 256 * (tune_wpc or 12) // 4)
        return Launch("fast" + suffix, norm, R, halves, blocks, rows_blk)
    if A < 0 and nchunk <= 64 and (x_sa or xn_obs):
        nlane = (L.used >> 1) if narrow else nchunk
        lgp = 0
        while (1 << lgp) < nlane:
            lgp += 1
        G = 64 >> lgp
        groups = (b + G - 1) // G
        R = 4 if groups >= 4 * 4096 else (2 if groups >= 2 * 4096 else 1)
        if tune_R in (1, 2, 4):
            R = tune_R
        blocks = min((groups + 4 * R - 1) // (4 * R), 256 * (tune_wpc or 16) // 4)
        return Launch("obs" + suffix, norm, R, lgp, blocks, 4 * R * G)
    R, CH = (4, 1) if nchunk <= 64 else ((2, 2) if nchunk <= 128 else ((1, 4) if nchunk <= 256 else (1, 16)))
    blocks = min((b + 4 * R - 1) // (4 * R), GENERIC_MAX_BLOCKS)
    return Launch("fused" + ("" if dtype == F32 else "_f16"), norm, (R, CH), TRANSITION if A >= 0 else OBS_ONLY, blocks, 4 * R)


def gather_path(O, A, dtype, ld_sa, ld_o, flags, b, destinations, norm=True):
    """(template, NORM, R or (R, CH), runtime variant) of one call"""
    return tuple(gather_launch(O, A, dtype, ld_sa, ld_o, flags, b, destinations, norm)[:4])


def instantiation(launch):
    shape = ", ".join(str(s) for s in launch.shape) if isinstance(launch.shape, tuple) else str(launch.shape)
    return f"k_replay_gather_{launch.template}<{'true' if launch.norm else 'false'}, {shape}>"


# --------------------------------------------------------------------------- the case table
# (storage, O, A, columns added to pqlk_ld, template, R | (R, CH), variant): what a call with default flags and a small batch
# reaches.  The O are the smallest on each side of every chunk-count seam of the dispatch above.
T_, O_ = TRANSITION, OBS_ONLY
_TABLE = [
    # fp32 transitions, A = 4: 64 | 65, 128 | 129, 256 | 257 chunks, and exactly 1024 (O = 2045 is refused)
    (F32, 124, 4, 0, "fast", 2, 1), (F32, 125, 4, 0, "fast", 2, 2), (F32, 252, 4, 0, "fast", 2, 2), (F32, 253, 4, 0, "fused", (1, 4), T_),
    (F32, 508, 4, 0, "fused", (1, 4), T_), (F32, 509, 4, 0, "fused", (1, 16), T_), (F32, 2044, 4, 0, "fused", (1, 16), T_),
    # A = 8
    (F32, 120, 8, 0, "fast", 2, 1), (F32, 121, 8, 0, "fast", 2, 2), (F32, 248, 8, 0, "fast", 2, 2), (F32, 249, 8, 0, "fused", (1, 4), T_),
    (F32, 504, 8, 0, "fused", (1, 4), T_), (F32, 505, 8, 0, "fused", (1, 16), T_),
    # fp32 obs-only
    (F32, 256, -1, 0, "obs", 1, 6), (F32, 257, -1, 0, "fused", (2, 2), O_), (F32, 512, -1, 0, "fused", (2, 2), O_),
    (F32, 513, -1, 0, "fused", (1, 4), O_), (F32, 1024, -1, 0, "fused", (1, 4), O_), (F32, 1025, -1, 0, "fused", (1, 16), O_),
    # O = GATHER_MAX_OBS with statistics
    (F32, 1024, 4, 0, "fused", (1, 16), T_),
    # lgp 0..6
    (F32, 1, -1, 0, "obs", 1, 0), (F32, 5, -1, 0, "obs", 1, 1), (F32, 9, -1, 0, "obs", 1, 2), (F32, 17, -1, 0, "obs", 1, 3),
    (F32, 33, -1, 0, "obs", 1, 4), (F32, 65, -1, 0, "obs", 1, 5), (F32, 129, -1, 0, "obs", 1, 6),
    # ragged fields: O % 4 != 0; O aligned but (O + A) % 4 != 0
    (F32, 1, 1, 0, "fast", 2, 1), (F32, 5, 3, 0, "fast", 2, 1), (F32, 8, 2, 0, "fast", 2, 1),
    # destinations 96 columns wider than pqlk_ld: the generic kernel's small shapes on transition rings
    (F32, 8, 2, 96, "fused", (4, 1), T_), (F32, 5, 3, 96, "fused", (4, 1), T_), (F32, 125, 4, 96, "fused", (2, 2), T_),
    # pqlk_ld + 32: still the fast kernel, at its pad bound
    (F32, 5, 3, 32, "fast", 2, 1), (F32, 124, 4, 32, "fast", 2, 1), (F32, 125, 4, 32, "fast", 2, 2),
    # fp16 transitions, A = 4: the narrow seam at 512 B (120 | 121), then 64 | 65, 128 | 129, 256 | 257 chunks
    (F16, 120, 4, 0, "fast_h8", 2, 1), (F16, 121, 4, 0, "fast_f16", 2, 1), (F16, 248, 4, 0, "fast_f16", 2, 1), (F16, 249, 4, 0, "fast_f16", 2, 2),
    (F16, 504, 4, 0, "fast_f16", 2, 2), (F16, 505, 4, 0, "fused_f16", (1, 4), T_), (F16, 1016, 4, 0, "fused_f16", (1, 4), T_),
    (F16, 1017, 4, 0, "fused_f16", (1, 16), T_),
    # A = 8
    (F16, 240, 8, 0, "fast_f16", 2, 1), (F16, 241, 8, 0, "fast_f16", 2, 2), (F16, 496, 8, 0, "fast_f16", 2, 2),
    (F16, 497, 8, 0, "fused_f16", (1, 4), T_), (F16, 1008, 8, 0, "fused_f16", (1, 4), T_), (F16, 1009, 8, 0, "fused_f16", (1, 16), T_),
    # fp16 obs-only: the narrow seam (256 | 257), then 64 | 65, 128 | 129, 256 | 257 chunks
    (F16, 256, -1, 0, "obs_h8", 1, 6), (F16, 257, -1, 0, "obs_f16", 1, 6), (F16, 512, -1, 0, "obs_f16", 1, 6),
    (F16, 513, -1, 0, "fused_f16", (2, 2), O_), (F16, 1024, -1, 0, "fused_f16", (2, 2), O_), (F16, 1025, -1, 0, "fused_f16", (1, 4), O_),
    (F16, 2048, -1, 0, "fused_f16", (1, 4), O_), (F16, 2049, -1, 0, "fused_f16", (1, 16), O_),
    (F16, 1024, 4, 0, "fused_f16", (1, 16), T_),
    # lgp 1..6 of the 8-B-chunk kernel
    (F16, 1, -1, 0, "obs_h8", 1, 1), (F16, 5, -1, 0, "obs_h8", 1, 1), (F16, 9, -1, 0, "obs_h8", 1, 2), (F16, 17, -1, 0, "obs_h8", 1, 3),
    (F16, 33, -1, 0, "obs_h8", 1, 4), (F16, 65, -1, 0, "obs_h8", 1, 5), (F16, 129, -1, 0, "obs_h8", 1, 6),
    (F16, 1, 1, 0, "fast_h8", 2, 1), (F16, 5, 3, 0, "fast_h8", 2, 1), (F16, 8, 2, 0, "fast_h8", 2, 1),
    (F16, 117, 3, 0, "fast_h8", 2, 1),     # exactly 512 B in use, O % 4 = 1, O odd: every kind of store of the 8-B-chunk kernel
    (F16, 8, 2, 96, "fused_f16", (4, 1), T_), (F16, 5, 3, 96, "fused_f16", (4, 1), T_), (F16, 249, 4, 96, "fused_f16", (2, 2), T_),
    (F16, 5, 3, 32, "fast_h8", 2, 1), (F16, 120, 4, 32, "fast_h8", 2, 1), (F16, 248, 4, 32, "fast_f16", 2, 1), (F16, 249, 4, 32, "fast_f16", 2, 2),
]

Case = namedtuple("Case", "name dtype O A extra template shape variant strided")


def _case(row):
    dtype, O, A, extra, template, shape, variant = row
    name = f"{DT[dtype]}_{O}_{'obs' if A < 0 else A}" + (f"_w{extra}" if extra else "")
    # one case per format inserts from source arrays whose strides are larger than their widths
    return Case(name, dtype, O, A, extra, template, shape, variant, (O, A, extra) == (5, 3, 0))


CASES = [_case(r) for r in _TABLE]
CASE_BY_NAME = {c.name: c for c in CASES}
assert len(CASE_BY_NAME) == len(CASES)

# one representative per template for the one-factor-at-a-time runs
REPRESENTATIVES = {"fast": "f32_125_4", "obs": "f32_33_obs", "fused": "f32_253_4", "fast_h8": "f16_117_3", "fast_f16": "f16_249_4",
                   "obs_h8": "f16_33_obs", "obs_f16": "f16_257_obs", "fused_f16": "f16_505_4"}
LEAN_R = {"fast": (1, 2, 4, 8), "obs": (1, 2, 4)}      # rows in flight the flag word can ask for
# the generic kernels past their block cap: 2048 * 4 * R + 3 rows
PAST_CAP = ["f32_8_2_w96", "f32_125_4_w96", "f32_253_4", "f32_509_4", "f16_8_2_w96", "f16_249_4_w96", "f16_505_4", "f16_1017_4"]


PLAIN_MAX_BLOCKS = 8192    # block cap of pqlk_replay_gather, one wave per row
PLAIN_PAST_CAP = ["f32_125_4", "f16_249_4"]


def has_stats(case):
    return case.O <= GATHER_MAX_OBS


def lds(case):
    """(ld_sa, ld_o) of the case's destinations"""
    return ld(case.O + max(case.A, 0)) + case.extra, ld(case.O) + case.extra


def all_dests(case):
    return DESTS if case.A >= 0 else ("x_sa", "xn_obs")


def dest_subsets(case):
    if case.A < 0:
        return [("x_sa", "xn_obs"), ("x_sa",), ("xn_obs",)]
    return [DESTS, ("x_sa",), ("xn_sa", "rew", "done"), ("xn_obs",), ("x_sa", "xn_sa", "rew", "done")]


def lean(case):
    return not case.template.startswith("fused")


def kind(template):
    return "fast" if template.startswith("fast") else ("obs" if template.startswith("obs") else "fused")


def launch_of(case, b=1, flags=0, norm=None, destinations=None):
    ld_sa, ld_o = lds(case)
    norm = has_stats(case) if norm is None else norm
    return gather_launch(case.O, case.A, case.dtype, ld_sa, ld_o, flags, b, all_dests(case) if destinations is None else destinations, norm)


def base_batches(case):
    """[(b, flags)] of the base sweep: one row; one fewer and one more than the rows a block takes per trip; for the lean
    kernels, with one wave per CU (64 blocks), the smallest b that gives some wave a second trip, which is then ragged."""
    rows_blk = launch_of(case).rows_blk
    out = [(b, 0) for b in sorted({1, rows_blk - 1, rows_blk + 1}) if b >= 1]
    if lean(case):
        b = 64 * rows_blk + 1
        la = launch_of(case, b, WAVES_PER_CU(1))
        assert la.blocks == 64 and la.rows_blk == rows_blk and la.shape == case.shape
        out.append((b, WAVES_PER_CU(1)))
    return out


def factor_runs(case):
    """[(what, flags, norm, destinations)] on a representative: one factor at a time away from statistics + clamp + every destination"""
    runs = [("clamp off", 0, True, None), ("pads_zero", CLAMP5 | PADS_ZERO, True, None), ("nt_loads", CLAMP5 | NT_LOADS, True, None),
            ("nt_stores", CLAMP5 | NT_STORES, True, None), ("nt_loads+stores, no statistics", NT_LOADS | NT_STORES, False, None)]
    for R in LEAN_R.get(kind(case.template), ()):
        for norm in (True, False):
            runs.append((f"R={R} norm={norm}", (CLAMP5 if norm else 0) | ROWS_IN_FLIGHT(R) | WAVES_PER_CU(1), norm, None))
    for d in dest_subsets(case)[1:]:
        runs.append(("destinations " + "+".join(d), CLAMP5, True, d))
        runs.append(("destinations " + "+".join(d) + " pads_zero", CLAMP5 | PADS_ZERO, True, d))
    return runs


def factor_batch(case, flags):
    """rows of a factor run: two full blocks and a ragged third, at least 37; a rows-in-flight override runs at one wave per CU
    (64 blocks) with one row more than the grid takes in a trip, so that its second, ragged trip runs at that R"""
    rows_blk = launch_of(case, 1, flags).rows_blk
    return 64 * rows_blk + 1 if (flags >> 12) & 63 else max(37, 2 * rows_blk + 1)


def reached():
    """{instantiation: set of runtime variants} over everything tests/test_gather_kernels_gpu.py launches"""
    out = {}

    def add(la):
        out.setdefault(instantiation(la), set()).add(la.variant)

    for c in CASES:
        for norm in ((True, False) if has_stats(c) else (False,)):
            for b, flags in base_batches(c):
                add(launch_of(c, b, flags, norm))
    for name in REPRESENTATIVES.values():
        c = CASE_BY_NAME[name]
        for _, flags, norm, dests in factor_runs(c):
            add(launch_of(c, factor_batch(c, flags), flags, norm, dests))
    for name in PAST_CAP:
        c = CASE_BY_NAME[name]
        add(launch_of(c, past_cap_rows(c), 0, True))
    return out


def past_cap_rows(case):
    return GENERIC_MAX_BLOCKS * 4 * case.shape[0] + 3


# --------------------------------------------------------------------------- data
def q16(x):
    return x.astype(np.float16).astype(np.float32)


def normalize(x, mean, var, clamp):
    sd = np.sqrt(var.astype(np.float32) + np.float32(EPS), dtype=np.float32)
    y = ((x.astype(np.float32) - mean.astype(np.float32)) / sd).astype(np.float32)
    return np.clip(y, np.float32(-5), np.float32(5)) if clamp else y


class Data:
    """The host rows of one (O, A): CAP source rows, inserted from ring row START on and wrapping, so that ring row j holds source
    row (j - START) mod CAP.  Every array below is in ring order."""

    def __init__(self, O, A):
        s = 1000 * O + 10 * (A + 1)
        perm = (np.arange(CAP) - START) % CAP
        self.O, self.A, self.perm = O, A, perm
        self.src = {"obs": dd.uniform((CAP, O), s + 1, -8, 8)}
        if A >= 0:
            done = dd.bernoulli((CAP, 1), s + 5, 0.3)
            done[::7, 0] = 2.5            # non-canonical truth values: stored as 1.0
            done[3::11, 0] = -0.0         # and a negative zero: stored as +0.0
            self.src.update(nobs=dd.uniform((CAP, O), s + 2, -8, 8), act=dd.uniform((CAP, A), s + 3, -2, 2),
                            rew=dd.uniform((CAP, 1), s + 4, -1, 1), done=done)
        self.head = CAP - START           # source rows [0, head) -> ring rows [START, CAP); the rest -> [0, CAP - head)
        # the first draw of the statistics under which the clamp binds on 5 % to 50 % of the elements (a ring of one or two columns
        # may draw a variance so large that nothing reaches +-5)
        for k in range(32):
            self._cache = {}
            self.mean = dd.uniform((O,), s + 6 + 100 * k, -0.5, 0.5)
            self.var = dd.uniform((O,), s + 7 + 100 * k, 0.25, 4.0)
            if 0.05 <= self.clamped_share(F32) <= 0.50:
                break

    def ring(self, field, dtype=F32):
        """the rows the ring holds, as the gathers return them"""
        key = (field, dtype if field in ("obs", "nobs") else F32)
        if key not in self._cache:
            a = self.src[field][self.perm]
            if field in ("obs", "nobs") and dtype == F16:
                a = q16(a)
            if field == "done":
                a = (a != 0).astype(np.float32)
            self._cache[key] = a
        return self._cache[key]

    def normed(self, field, dtype, norm, clamp):
        if not norm:
            return self.ring(field, dtype)
        key = (field, dtype, "n", bool(clamp))
        if key not in self._cache:
            self._cache[key] = normalize(self.ring(field, dtype), self.mean, self.var, clamp)
        return self._cache[key]

    def clamped_share(self, dtype):
        """share of the normalised elements that lie outside +-5"""
        ys = [self.normed(f, dtype, True, False) for f in (("obs", "nobs") if self.A >= 0 else ("obs",))]
        return float(np.mean(np.concatenate([np.abs(y).reshape(-1) > 5 for y in ys])))


@lru_cache(maxsize=None)
def data(O, A):
    return Data(O, A)


def expected_records(dtype, d):
    """raw 32-bit words (CAP, rec_ld) of the ring after the fill, pad words and pad halves zero"""
    L = layout(d.O, d.A, dtype)
    O, A = d.O, d.A
    fields = [("obs", 0)] + ([("nobs", L.off_nobs)] if A >= 0 else [])
    if dtype == F32:
        w = np.zeros((CAP, L.ld), dtype=np.uint32)
        for f, off in fields:
            w[:, off: off + O] = d.src[f][d.perm].view(np.uint32)
    else:
        h = np.zeros((CAP, 2 * L.ld), dtype=np.uint16)
        for f, off in fields:
            h[:, 2 * off: 2 * off + O] = d.src[f][d.perm].astype(np.float16).view(np.uint16)
        w = h.view(np.uint32)            # little endian: the even column is the low half of its word
    if A >= 0:
        w[:, L.off_act: L.off_act + A] = d.ring("act").view(np.uint32)
        w[:, L.off_rd] = d.ring("rew").view(np.uint32)[:, 0]
        w[:, L.off_rd + 1] = d.ring("done").view(np.uint32)[:, 0]
    return w


_SPECIAL = (CAP + 5, 0, -1, None, None, CAP, CAP - 1)       # None, None: a duplicate pair


def indices(b, seed):
    """b sample indices; with b >= 7 they hold 0, CAP - 1 (in the last row), a duplicate, -1, CAP and CAP + 5, spread over the
    vector (a shorter vector takes CAP - 1, -1, 0, CAP, CAP + 5, a pair, as far as it goes)"""
    idx = dd.integers((b,), seed, CAP)
    if b < 7:
        idx[:] = np.array([CAP - 1, -1, 0, CAP, CAP + 5, 9, 9], dtype=np.int64)[:b]
        return idx
    pos = [int(p) for p in np.linspace(0, b - 1, 7)]
    for p, v in zip(pos, _SPECIAL):
        idx[p] = idx[pos[3]] if v is None else v
    return idx


def sources(idx):
    return np.where((idx >= 0) & (idx < CAP), idx, 0)


def expected(case, idx, norm, flags, destinations=None, d=None):
    """{destination: the whole buffer after the call}, GUARD_ROWS of poison behind the b rows, POISON where nothing is written"""
    d = data(case.O, case.A) if d is None else d
    O, A, b = case.O, case.A, len(idx)
    ld_sa, ld_o = lds(case)
    dests = all_dests(case) if destinations is None else destinations
    src = sources(idx)
    clamp, pads = bool(flags & CLAMP5), not (flags & PADS_ZERO)
    n_obs = d.normed("obs", case.dtype, norm, clamp)[src]
    n_next = d.normed("nobs", case.dtype, norm, clamp)[src] if A >= 0 else n_obs
    out = {}
    for name in dests:
        cols = {"x_sa": ld_sa, "xn_sa": ld_sa, "xn_obs": ld_o}.get(name)
        t = np.full((b + GUARD_ROWS,) + ((cols,) if cols else ()), POISON, dtype=np.float32)
        if name == "x_sa":
            t[:b, :O] = n_obs
            if A >= 0:
                t[:b, O: O + A] = d.ring("act")[src]
            if pads:
                t[:b, O + max(A, 0):] = 0
        elif name == "xn_sa":
            t[:b, :O] = n_next
            if pads:
                t[:b, O + A:] = 0
        elif name == "xn_obs":
            t[:b, :O] = n_next
            if pads:
                t[:b, O:] = 0
        else:
            t[:b] = d.ring(name)[src, 0]
        out[name] = t
    return out


def expected_plain(case, idx, d=None):
    """the five contiguous outputs of pqlk_replay_gather, GUARD_ROWS of poison behind them"""
    d = data(case.O, case.A) if d is None else d
    src, b = sources(idx), len(idx)
    out = {}
    for name, f in (("obs", "obs"),) + ((("act", "act"), ("rew", "rew"), ("nobs", "nobs"), ("done", "done")) if case.A >= 0 else ()):
        a = d.ring(f, case.dtype)[src]
        t = np.full((b + GUARD_ROWS, a.shape[1]), POISON, dtype=np.float32)
        t[:b] = a
        out[name] = t
    return out


# --------------------------------------------------------------------------- checks
def bits(a):
    a = np.ascontiguousarray(a)
    assert a.dtype == np.float32
    return a.view(np.uint32)


def _region(case, name, r, c, b):
    if r >= b:
        return "guard row"
    if name in ("rew", "done"):
        return name
    if c < case.O:
        return "observation column"
    if name == "x_sa" and c < case.O + max(case.A, 0):
        return "action column"
    if name == "xn_sa" and c < case.O + case.A:
        return "untouched action column"
    return "pad column"


def check_outputs(got, want, case, what):
    """every destination equals the reference bit for bit: data, pads, untouched columns and guard rows"""
    assert set(got) == set(want), (what, sorted(got), sorted(want))
    for name in want:
        g, w = np.asarray(got[name]), want[name]
        assert g.shape == w.shape and g.dtype == np.float32, (what, name, g.shape, w.shape, g.dtype)
        bad = np.argwhere(bits(g) != bits(w))
        if len(bad):
            r, c = int(bad[0][0]), (int(bad[0][1]) if g.ndim == 2 else 0)
            gv, wv = (g[r, c], w[r, c]) if g.ndim == 2 else (g[r], w[r])
            raise AssertionError(f"{what}: {name}: {len(bad)} elements differ, first at row {r} col {c} "
                                 f"({_region(case, name, r, c, len(w) - GUARD_ROWS)}): got {gv!r}, want {wv!r}")


def check_records(got_words, want_words, what):
    got_words = np.asarray(got_words)
    assert got_words.shape == want_words.shape and got_words.dtype == np.uint32, (what, got_words.shape, want_words.shape)
    bad = np.argwhere(got_words != want_words)
    if len(bad):
        r, c = (int(v) for v in bad[0])
        raise AssertionError(f"{what}: {len(bad)} record words differ, first at ring row {r} word {c}: "
                             f"got {got_words[r, c]:#010x}, want {want_words[r, c]:#010x}")
