"""Half-precision observation storage of the replay rings on the GPU (PQLK_OBS_F16, `reserve_space=True`, `algo.replay_obs_dtype`).

The law every test here pins: an fp16 ring fed x behaves bit for bit like the fp32 ring fed q(x) = x.to(float16).to(float32).  The
fp32 path is itself pinned to the reference by the existing tests, so it is the yardstick throughout.  Floats are compared through
their int32 bit views; where inputs hold NaN the NaN positions must agree and everything else must be bit-equal (payloads are not
pinned).  Run with `pytest -m gpu`."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import detdata as dd
from learner_harness import _fill, _sd, make_cfg
from resume_cases import PQL, PQL_KEYS, child, same
from support import dev  # noqa: F401

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (O, A); A = -1: the P-learner's obs-only ring.  O not a multiple of 4 or 8, records above 1 KiB ((600, 7): 2.4 KiB in fp16), and
# (300, 6): a 1.25-KiB fp16 record, the two-waves-per-row shape of the fast kernel, which none of the others reaches in fp16;
# (520, 4): 132 fp16 chunks, the four-chunks-per-lane instantiation of the generic kernel; (400, -1): an obs-only record above the
# 512 B that the 8-B-chunk kernels serve, so the 16-B-chunk obs kernel (which (211, 20) and (108, 21) reach for transition rings)
SHAPES = [(8, 2), (88, 16), (211, 20), (108, 21), (3, 1), (13, 5), (600, 7), (300, 6), (520, 4), (3, -1), (13, -1), (88, -1), (211, -1), (400, -1),
          (600, -1)]
SENTINEL = -777.25
CLAMP5, PADS_ZERO, NT_LOADS = 1, 2, 4


def q(x):
    """The quantisation, by torch on the CPU."""
    return x.cpu().to(torch.float16).to(torch.float32)


def bits(t):
    return t.contiguous().view(torch.int32)


def assert_same_bits(a, b, what=""):
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    assert a.shape == b.shape and a.dtype == b.dtype, (what, a.shape, b.shape, a.dtype, b.dtype)
    na, nb = torch.isnan(a), torch.isnan(b)
    assert torch.equal(na, nb), f"{what}: NaN positions differ ({int(na.sum())} vs {int(nb.sum())})"
    ia = torch.where(na, torch.zeros_like(bits(a)), bits(a))
    ib = torch.where(nb, torch.zeros_like(bits(b)), bits(b))
    bad = (ia != ib).nonzero()
    assert bad.numel() == 0, f"{what}: {bad.shape[0]} elements differ, first at {bad[0].tolist()}: {a[tuple(bad[0])]!r} vs {b[tuple(bad[0])]!r}"


_SPECIALS = {}


def specials():
    """Every value the rounding can go wrong at, as one fp32 vector (computed once): all 65 536 fp16 bit patterns widened; the fp32
    midpoint of every adjacent finite fp16 pair and that midpoint -+ 1 fp32 ulp (ties to even), both signs -- which contains 2^-25
    (half the smallest subnormal) and its two neighbours; the largest-finite / infinity boundary; fp32 values below every fp16
    subnormal; +-0, +-inf and NaN come with the bit patterns."""
    if "v" not in _SPECIALS:
        allh = torch.arange(-32768, 32768, dtype=torch.int32).to(torch.int16).view(torch.float16).to(torch.float32)
        fin = torch.arange(0, 0x7C00, dtype=torch.int32).to(torch.int16).view(torch.float16).to(torch.float32)   # +0 .. 65504, ascending
        mid = (fin[:-1].double() + fin[1:].double()) / 2
        mid = mid.to(torch.float32)
        assert torch.equal(mid.double() * 2, fin[:-1].double() + fin[1:].double())    # exact: 12 significant bits
        mb = mid.view(torch.int32)
        mids = torch.cat([mid, (mb - 1).view(torch.float32), (mb + 1).view(torch.float32)])
        tiny = torch.tensor([2.0 ** -25], dtype=torch.float32)
        edge = torch.cat([torch.tensor([65519.996, 65520.0, 65504.0, 65519.0, 65535.0, 65536.0, 1e6, 3.4e38, 1e-8, 1e-30, 1.4e-45],
                                       dtype=torch.float32), tiny, (tiny.view(torch.int32) - 1).view(torch.float32),
                          (tiny.view(torch.int32) + 1).view(torch.float32)])
        rnd = torch.from_numpy(dd.uniform((4096,), 4242, -3, 3))
        v = torch.cat([allh, mids, -mids, edge, -edge, rnd])
        assert float(torch.tensor(65519.996, dtype=torch.float32)) < 65520.0 and torch.isinf(q(torch.tensor([65520.0]))).all()
        assert q(torch.tensor([65519.996]))[0] == 65504.0 and q(tiny)[0] == 0.0 and q((tiny.view(torch.int32) + 1).view(torch.float32))[0] > 0
        _SPECIALS["v"] = v
    return _SPECIALS["v"]


def make_ring(cap, O, A, dev, dtype):
    from pql_amd.replay.simple_replay import RecordRing, ReplayBuffer
    if A < 0:
        return None, RecordRing(cap, O, -1, dev, obs_dtype=dtype)
    rb = ReplayBuffer(cap, (O,), A, dev, obs_dtype=dtype)
    return rb, rb.ring


def expected_records(ring, obs, act=None, rew=None, nobs=None, done=None):
    """The raw fp16 records of these rows as int16 halves (m, 2 * rec_ld), built on the CPU from the header's layout."""
    m, O, A = obs.shape[0], ring.O, ring.A
    h = torch.zeros((m, 2 * ring.rec_ld), dtype=torch.int16)
    h[:, :O] = obs.to(torch.float16).view(torch.int16)
    if A >= 0:
        h[:, 2 * ring.off_nobs: 2 * ring.off_nobs + O] = nobs.to(torch.float16).view(torch.int16)
        w = h.view(torch.int32)
        w[:, ring.off_act: ring.off_act + A] = bits(act)
        w[:, ring.off_rd] = bits(rew)[:, 0]
        w[:, ring.off_rd + 1] = bits((done != 0).to(torch.float32))[:, 0]
    return h


@pytest.mark.parametrize("O,A", SHAPES)
def test_insert_quantises_as_torch_does_and_the_plain_gather_widens_exactly(dev, O, A):
    """Insert (a wrapped, two-segment one) then read back: the raw records equal the layout of include/pqlk.h filled with torch's
    x.to(float16) -- pad halves and words zero, actions / reward exact, done canonical -- rows beside the two segments keep their
    bits, and the plain gather returns x.to(float16).to(float32)."""
    from pql_amd import _lib as L
    from pql_amd.replay.simple_replay import ring_plan
    v = specials()
    m = (v.numel() + O - 1) // O
    pad = m * O - v.numel()
    obs = torch.cat([v, v[:pad]]).reshape(m, O)
    nobs = torch.cat([v, v[:pad]]).roll(12345).reshape(m, O)
    act = rew = done = None
    if A >= 0:
        act = torch.from_numpy(dd.uniform((m, A), 7, -2, 2))
        act.view(-1)[:8] = torch.tensor([0.0, -0.0, float("inf"), -float("inf"), 1e-40, -1e-45, 65519.996, 2.0 ** -25])   # stay fp32
        rew = torch.from_numpy(dd.uniform((m, 1), 8, -0.05, 0.05))
        done = torch.from_numpy(dd.bernoulli((m, 1), 9, 0.3))
        done[:4, 0] = torch.tensor([2.5, -0.0, 0.0, 1.0])
    cap, start = m + 7, m // 3 + 11     # 7 rows stay untouched between the wrapped tail and the head
    rb, ring = make_ring(cap, O, A, dev, torch.float16)
    assert ring.rec_ld == L.lib.pqlk_replay_rec_ld_ex(O, A, L.OBS_F16) and ring.records.dtype == torch.float32
    assert ring.records.shape == (cap, ring.rec_ld) and ring.desc.obs_dtype == L.OBS_F16
    ring.records.fill_(SENTINEL)
    to = lambda t: None if t is None else t.to(dev)   # noqa: E731
    if rb is not None:
        rb.next_p = start
        rb.add_to_buffer((to(obs), to(act), to(rew), to(nobs), to(done)))
        assert rb.if_full and rb.cur_capacity == cap and rb.next_p == start + m - cap
    else:
        segs, p, full, cur = ring_plan(start, False, cap, m)
        assert len(segs) == 2 and full and cur == cap
        ring.insert_segments(segs, to(obs))
    head = cap - start                                   # source rows [0, head) -> [start, cap); the LAST m - head rows -> [0, m - head)
    rows = torch.cat([torch.arange(start, cap), torch.arange(0, m - head)])
    raw = ring.records.cpu()
    got = raw[rows].view(torch.int16)
    want = expected_records(ring, obs, act, rew, nobs, done)
    gh, wh = got.view(torch.float16), want.view(torch.float16)
    # observation halves: NaN where torch's are NaN, every other half -- data, pad halves, and the fp32 words seen as halves -- equal
    obs_cols = torch.zeros(2 * ring.rec_ld, dtype=torch.bool)
    obs_cols[:O] = True
    if A >= 0:
        obs_cols[2 * ring.off_nobs: 2 * ring.off_nobs + O] = True
    nan = torch.isnan(wh) & obs_cols
    assert torch.equal(torch.isnan(gh) & obs_cols, nan)
    assert torch.equal(torch.where(nan, torch.zeros_like(got), got), torch.where(nan, torch.zeros_like(want), want))
    untouched = raw[m - head: start]
    assert untouched.shape[0] == 7 and bool((untouched == SENTINEL).all())
    # reference-named views and the plain gather
    idx = torch.cat([rows, torch.tensor([0, cap - 1, 5, 5])]).to(dev)
    src = torch.cat([torch.arange(m), torch.tensor([head, head - 1, int((rows == 5).nonzero()), int((rows == 5).nonzero())])])
    if rb is not None:
        assert rb.buf_obs.dtype == torch.float16 and rb.buf_obs.shape == (cap, O) and rb.buf_next_obs.shape == (cap, O)
        o, a, r, no, d = rb.sample_batch(idx.shape[0], device=dev, indices=idx)
        assert all(t.dtype == torch.float32 for t in (o, a, r, no, d))
        assert_same_bits(o, q(obs)[src], "obs")
        assert_same_bits(no, q(nobs)[src], "next_obs")
        assert_same_bits(o, rb.buf_obs[idx].to(torch.float32), "obs vs buf_obs")
        assert_same_bits(no, rb.buf_next_obs[idx].to(torch.float32), "next_obs vs buf_next_obs")
        assert torch.equal(bits(a.cpu()), bits(act[src])) and torch.equal(bits(r.cpu()), bits(rew[src]))
        assert torch.equal(d.cpu(), (done[src] != 0).to(torch.float32))
    else:
        out = torch.full((idx.shape[0], O), SENTINEL, device=dev)
        L.check(L.lib.pqlk_replay_gather(C.byref(ring.desc), L.ptr(idx), idx.shape[0], L.ptr(out), None, None, None, None, L.stream(dev)))
        assert_same_bits(out, q(obs)[src], "obs")
        assert_same_bits(out, ring.obs_view()[idx].to(torch.float32), "obs vs view")


def _rows(O, A, n, seed):
    """Random rows with the specials sprinkled in (NaN, infinities, ties, subnormals, values that overflow fp16)."""
    obs = torch.from_numpy(dd.uniform((n, O), seed, -3, 3))
    nobs = torch.from_numpy(dd.uniform((n, O), seed + 1, -3, 3))
    sp = torch.tensor([float("nan"), float("inf"), -float("inf"), 65519.996, 65520.0, -1e6, 2.0 ** -25, 6e-8, -0.0, 1.00048828125, 3e-5])
    for t, s in ((obs, seed + 2), (nobs, seed + 3)):
        pos = torch.from_numpy(dd.integers((64,), s, n * O)).long()
        t.view(-1)[pos] = sp.repeat(6)[:64]
    if A < 0:
        return obs, None, None, None, None
    return (obs, torch.from_numpy(dd.uniform((n, A), seed + 4, -1, 1)), torch.from_numpy(dd.uniform((n, 1), seed + 5, -0.05, 0.05)), nobs,
            torch.from_numpy(dd.bernoulli((n, 1), seed + 6, 0.1)))


def _indices(b, cap, seed, dev):
    idx = torch.from_numpy(dd.integers((b,), seed, cap)).long()
    idx[-1] = cap - 1
    if b >= 5:
        idx[0], idx[2], idx[3] = 0, idx[1], cap + 5      # row 0, a duplicate, one index >= capacity (both rings map it to row 0)
    return idx.to(dev)


@pytest.mark.parametrize("O,A", SHAPES)
def test_fused_gather_of_an_fp16_ring_equals_the_fp32_ring_fed_the_quantised_rows(dev, O, A):
    """x_sa, xn_sa, xn_obs, rew and done of the fused gather: fp16 ring fed x == fp32 ring fed q(x), bit for bit, with and without
    statistics, clamp on / off, PADS_ZERO on / off (tiles pre-filled with a sentinel: the untouched action columns of xn_sa and the
    pad columns are compared too), non-temporal loads on / off, b in {1, 5, 257, 4 x 300 as one K-batch launch}; once more with a
    destination so wide that the call leaves the lean kernels for the generic one."""
    from pql_amd import _lib as L
    cap, n = 3000, 2900
    data = _rows(O, A, n, 100 + O)
    rings = {}
    for name, dtype in (("h", torch.float16), ("f", torch.float32)):
        rb, ring = make_ring(cap, O, A, dev, dtype)
        feed = [None if t is None else t.clone() for t in data]
        if name == "f":
            feed[0] = q(feed[0])
            if A >= 0:
                feed[3] = q(feed[3])
        feed = [None if t is None else t.to(dev) for t in feed]
        if rb is not None:
            rb.next_p = cap - 500                                             # the fill wraps
            rb.add_to_buffer(tuple(feed))
        else:
            from pql_amd.replay.simple_replay import ring_plan
            ring.insert_segments(ring_plan(cap - 500, False, cap, n)[0], feed[0])
        rings[name] = ring
    assert rings["h"].rec_ld <= rings["f"].rec_ld
    mean = torch.from_numpy(dd.uniform((O,), 6, -0.5, 0.5)).to(dev)
    var = torch.from_numpy(dd.uniform((O,), 7, 0.5, 2.0)).to(dev)
    Aw = max(A, 0)
    checked = 0
    for b in (1, 5, 257, 4 * 300):
        idx = _indices(b, cap, 31 + b, dev)
        for wide in (False, True):
            ld_sa = L.ld(O + (Aw if A >= 0 else 16)) + (96 if wide else 0)
            ld_o = L.ld(O) + (96 if wide else 0)
            for norm in (True, False):
                for clamp in ((CLAMP5, 0) if norm else (0,)):
                    for pz in ((0,) if wide else (0, PADS_ZERO)):
                        for nt in (0, NT_LOADS):
                            outs = {}
                            for name, ring in rings.items():
                                f = dict(dtype=torch.float32, device=dev)
                                x_sa, xn_obs = torch.full((b, ld_sa), SENTINEL, **f), torch.full((b, ld_o), SENTINEL, **f)
                                xn_sa = torch.full((b, ld_sa), SENTINEL, **f) if A >= 0 else None
                                rew = torch.full((b,), SENTINEL, **f) if A >= 0 else None
                                done = torch.full((b,), SENTINEL, **f) if A >= 0 else None
                                L.check(L.lib.pqlk_replay_gather_fused(
                                    C.byref(ring.desc), L.ptr(idx), b, L.ptr(mean) if norm else None, L.ptr(var) if norm else None, 1e-4,
                                    clamp | pz | nt, L.ptr(x_sa), ld_sa, L.ptr(xn_sa), L.ptr(xn_obs), ld_o, L.ptr(rew), L.ptr(done),
                                    L.stream(dev)))
                                outs[name] = [t for t in (x_sa, xn_sa, xn_obs, rew, done) if t is not None]
                            what = f"b={b} wide={wide} norm={norm} clamp={clamp} pads_zero={pz} nt={nt}"
                            for k, (h, f32) in enumerate(zip(outs["h"], outs["f"])):
                                assert_same_bits(h, f32, f"{what} output {k}")
                            checked += 1
                            if b == 257 and norm and not wide:     # the fp32 side is not vacuous: data columns written, sentinels kept
                                x_sa = outs["h"][0].cpu()
                                assert not bool((x_sa[:, :O + Aw] == SENTINEL).any())
                                if pz:
                                    assert bool((x_sa[:, O + Aw:] == SENTINEL).all())
                                elif A >= 0:
                                    assert bool((x_sa[:, O + Aw:] == 0).all()) and bool((outs["h"][1].cpu()[:, O:O + Aw] == SENTINEL).all())
    assert checked == 4 * (12 + 6)
    # without statistics the tile holds q(x) itself
    idx = _indices(257, cap, 9, dev)
    x_sa = torch.zeros((257, L.ld(O + Aw + (16 if A < 0 else 0))), device=dev)
    L.check(L.lib.pqlk_replay_gather_fused(C.byref(rings["h"].desc), L.ptr(idx), 257, None, None, 1e-4, 0, L.ptr(x_sa), x_sa.shape[1], None,
                                           None, 0, None, None, L.stream(dev)))
    src = torch.where(idx >= cap, torch.zeros_like(idx), idx).cpu()
    ring_row = (torch.arange(n) + cap - 500) % cap                           # source row r lives in ring row (cap - 500 + r) mod cap
    inv = torch.full((cap,), -1, dtype=torch.long)
    inv[ring_row] = torch.arange(n)
    keep = inv[src] >= 0                                                       # (rows never written hold zeros)
    assert_same_bits(x_sa.cpu()[keep][:, :O], q(data[0])[inv[src][keep]], "identity gather")


def test_unknown_obs_dtype_is_a_shape_error(dev):
    from pql_amd import _lib as L
    rec = torch.zeros((4, 32), device=dev)
    idx = torch.zeros(2, dtype=torch.int64, device=dev)
    out = [torch.zeros((2, 32), device=dev) for _ in range(5)]
    for code in (2, -1, 7):
        d = L.PqlReplayDesc(rec.data_ptr(), 4, 8, 2, 32, code)
        assert L.lib.pqlk_replay_insert(C.byref(d), 0, 2, *[x for t in out for x in (L.ptr(t), 32)], L.stream(dev)) == 2   # PQLK_E_SHAPE
        assert L.lib.pqlk_replay_gather(C.byref(d), L.ptr(idx), 2, *[L.ptr(t) for t in out], L.stream(dev)) == 2
        assert L.lib.pqlk_replay_gather_fused(C.byref(d), L.ptr(idx), 2, None, None, 1e-4, 0, L.ptr(out[0]), 32, L.ptr(out[1]), L.ptr(out[2]),
                                              32, L.ptr(out[3]), L.ptr(out[4]), L.stream(dev)) == 2
    torch.cuda.synchronize()
    assert float(rec.abs().sum()) == 0


def test_reference_named_surface(dev):
    """`ReplayBuffer(reserve_space=True)`, `create_buffer(reserve_space=True)`: the reference's switch (simple_replay.py:9,15,91,94)."""
    from pql_amd.replay.simple_replay import ReplayBuffer, create_buffer
    O, A, cap = 88, 16, 1000
    rb = ReplayBuffer(cap, (O,), A, device=dev, reserve_space=True)
    assert rb.records.dtype == torch.float32 and rb.records.numel() * 4 == cap * 512
    assert ReplayBuffer(cap, (O,), A, device=dev).records.numel() * 4 == cap * 896
    assert ReplayBuffer(cap, (O,), A, device=dev, obs_dtype=torch.float16).ring.half and rb.ring.obs_dtype == torch.float16
    assert not ReplayBuffer(cap, (O,), A, device=dev, obs_dtype="float32").ring.half
    obs, act, rew, nobs, done = _rows(O, A, 700, 5)
    rb.add_to_buffer(tuple(t.to(dev) for t in (obs, act, rew, nobs, done)))
    assert (rb.next_p, rb.cur_capacity, rb.if_full) == (700, 700, False)
    assert rb.buf_obs.dtype == rb.buf_next_obs.dtype == torch.float16 and rb.buf_obs.shape == rb.buf_next_obs.shape == (cap, O)
    assert rb.buf_action.dtype == rb.buf_reward.dtype == torch.float32 and rb.buf_done.dtype == torch.bool
    assert rb.buf_action.shape == (cap, A) and rb.buf_reward.shape == (cap, 1) and rb.buf_done.shape == (cap, 1)
    assert_same_bits(rb.buf_obs[:700].to(torch.float32), q(obs), "buf_obs")
    assert_same_bits(rb.buf_next_obs[:700].to(torch.float32), q(nobs), "buf_next_obs")
    assert torch.equal(bits(rb.buf_action[:700].cpu()), bits(act)) and torch.equal(bits(rb.buf_reward[:700].cpu()), bits(rew))
    assert torch.equal(rb.buf_done[:700].cpu(), done != 0)
    torch.manual_seed(3)
    o, a, r, no, d = rb.sample_batch(300, device=dev)
    torch.manual_seed(3)
    idx = rb.draw_indices(300)
    assert all(t.dtype == torch.float32 and t.device == dev for t in (o, a, r, no, d))
    assert_same_bits(o, rb.buf_obs[idx].to(torch.float32), "sample obs")
    assert_same_bits(no, rb.buf_next_obs[idx].to(torch.float32), "sample next_obs")
    assert torch.equal(a, rb.buf_action[idx]) and torch.equal(r, rb.buf_reward[idx]) and torch.equal(d, rb.buf_done[idx].float())
    bufs = create_buffer(50, (O,), A, device=dev, reserve_space=True)
    assert [t.dtype for t in bufs] == [torch.float16, torch.float32, torch.float16, torch.float32, torch.bool]
    assert [tuple(t.shape) for t in bufs] == [(50, O), (50, A), (50, O), (50, 1), (50, 1)] and all(t.device == dev for t in bufs)
    assert [t.dtype for t in create_buffer(50, (O,), A, device=dev)] == [torch.float32] * 4 + [torch.bool]
    with pytest.raises(NotImplementedError):
        ReplayBuffer(cap, (O,), A, device=dev, left_agent=True)
    with pytest.raises(NotImplementedError):
        ReplayBuffer(cap, (O,), A, device=dev, left_agent=True, reserve_space=True)
    with pytest.raises(ValueError):
        ReplayBuffer(cap, (O,), A, device=dev, obs_dtype=torch.bfloat16)
    # the ring header of a checkpoint names the format; one written before the key existed means float32
    st = rb.training_state()
    assert st["ring"]["obs_dtype"] == "float16"
    f32 = ReplayBuffer(cap, (O,), A, device=dev)
    with pytest.raises(ValueError, match="obs_dtype=float32 but the checkpoint holds obs_dtype=float16"):
        f32.load_training_state(st)
    with pytest.raises(ValueError, match="obs_dtype=float16 but the checkpoint holds obs_dtype=float32"):
        rb.load_training_state(f32.training_state())
    old = f32.training_state()
    del old["ring"]["obs_dtype"]
    f32.load_training_state(old)
    with pytest.raises(ValueError, match="obs_dtype"):
        rb.load_training_state(old)
    rb.load_training_state(st)


# ------------------------------------------------------------------------------------------------ learners
def _qdata(data, dtype):
    """The rows as fed: x to the fp16 ring, q(x) to the fp32 ring."""
    data = list(data)
    if dtype == "float32":
        data[0], data[3] = q(data[0]), q(data[3])
    return tuple(data)


def _pql_run(dev, dtype, distl, graph):
    from pql_amd.algo.pql_p_learner import PQLPLearner
    from pql_amd.algo.pql_v_learner import PQLVLearner
    O, A, B = 8, 2, 256
    cfg = make_cfg(distl, B=B, memory=3000, graph=graph)
    cfg.algo.rng = "auto"
    cfg.algo.replay_obs_dtype = dtype
    v, p = PQLVLearner((O,), A, cfg), PQLPLearner((O,), A, cfg)
    assert v.memory.ring.half == p.ring.half == (dtype == "float16")
    v.critic.load_state_dict(_sd(dd.doubleq_state(O, A, 51 if distl else 1, 31 if distl else 21)))
    v.critic_target.arena.data.copy_(v.critic.arena.data)
    p.actor.load_state_dict(_sd(dd.mlp_state(O, A, 11)))
    v.use_private_rng(1234); p.use_private_rng(4321)
    norm = (torch.from_numpy(dd.uniform((O,), 6, -0.5, 0.5)).to(dev), torch.from_numpy(dd.uniform((O,), 7, 0.5, 2.0)).to(dev), 1e-4)
    Kv, Kp = v._depth, p._depth
    for it in range(2):                                                        # two hand-offs, fresh rows at each
        data = tuple(t.to(dev) for t in _qdata(_fill(O, A, 700, 50 + 10 * it), dtype))
        critic, _, _ = v.update(p.actor, data, norm, 0)
        p.update(critic, data[0], norm, 0)
        if graph:
            v.learn_many(Kv); p.learn_many(Kp)
        else:
            for _ in range(Kv):
                v.learn()
            for _ in range(Kp):
                p.learn()
    torch.cuda.synchronize()
    assert v.update_count == 2 * Kv and p.update_count == 2 * Kp and v.memory.cur_capacity == 1400 == p.cur_capacity
    out = {"critic": v.critic.arena.data, "critic_target": v.critic_target.arena.data, "v.m": v.opt.m, "v.v": v.opt.v, "v.step": v.opt.step,
           "v.loss": v.loss_ring, "actor": p.actor.arena.data, "p.m": p.opt.m, "p.v": p.opt.v, "p.step": p.opt.step, "p.loss": p.loss_ring}
    out = {k: t.detach().clone().cpu() for k, t in out.items()}
    out["offsets"] = torch.tensor([v.gen.get_offset(), p.gen.get_offset()])
    return out


@pytest.mark.parametrize("distl,graph", [(False, False), (False, True), (True, True)])
def test_pql_learners_on_fp16_rings_equal_fp32_rings_fed_the_quantised_rows(dev, distl, graph):
    """PQLVLearner + PQLPLearner (algo.replay_obs_dtype=float16, rings filled through `update`: add_to_buffer / the P-learner's insert)
    over two hand-offs -- 2 K V steps and the matching P steps, one `update()` with fresh rows in between: arenas, targets, Adam state,
    loss rings and generator offsets equal those of the fp32 rings fed q(x).  Eager, as whole-run graphs, and with the C51 critic."""
    h, f = _pql_run(dev, "float16", distl, graph), _pql_run(dev, "float32", distl, graph)
    for k in h:
        assert torch.equal(h[k], f[k]) if h[k].dtype != torch.float32 else torch.equal(bits(h[k]), bits(f[k])), k
    assert float(h["v.loss"].abs().sum()) > 0 and float(h["p.loss"].abs().sum()) > 0 and torch.isfinite(h["critic"]).all()


def _baseline_run(dev, algo, dtype):
    import importlib
    from pql_amd.envs.synthetic import create_task_env
    from pql_amd.replay.simple_replay import ReplayBuffer
    from pql_amd.utils.cfg import load_cfg
    O, A = 8, 2
    cfg = load_cfg([f"algo={algo}_algo", "task.name=Toy", "num_envs=64", "algo.batch_size=64", "algo.memory_size=400", "device=cuda:0",
                    "sim_device=cuda:0", "algo.update_times=3", f"algo.replay_obs_dtype={dtype}"])
    cls = getattr(importlib.import_module(f"pql_amd.algo.{algo}"), {"ddpg": "AgentDDPG", "sac": "AgentSAC", "crossq": "AgentCrossQ"}[algo])
    torch.manual_seed(11)
    agent = cls(create_task_env(cfg), cfg)
    assert agent.replay_obs_dtype == (torch.float16 if dtype == "float16" else torch.float32)
    agent.obs_rms.mean = torch.from_numpy(dd.uniform((O,), 801, -0.5, 0.5)).to(dev)
    agent.obs_rms.var = torch.from_numpy(dd.uniform((O,), 802, 0.5, 2.0)).to(dev)
    memory = ReplayBuffer(400, (O,), A, device=dev, obs_dtype=agent.replay_obs_dtype)
    memory.add_to_buffer(tuple(t.to(dev) for t in _qdata(_fill(O, A, 300, 810), dtype)))
    before = {k: t.detach().clone().cpu() for k, t in agent._state_tensors().items()}
    torch.manual_seed(12)
    info = agent.update_net(memory)
    torch.cuda.synchronize()
    return before, {k: t.detach().clone().cpu() for k, t in agent._state_tensors().items()}, info


@pytest.mark.parametrize("algo", ["ddpg", "sac", "crossq"])
def test_baseline_agents_on_an_fp16_ring_equal_the_fp32_ring_fed_the_quantised_rows(dev, algo):
    """update_net (3 steps) of DDPG, SAC and CrossQ from a pre-filled buffer built from `algo.replay_obs_dtype`."""
    (h0, h, hi), (f0, f, fi) = _baseline_run(dev, algo, "float16"), _baseline_run(dev, algo, "float32")
    assert h0.keys() == f0.keys() and h.keys() == f.keys()
    for k in h0:
        assert torch.equal(h0[k], f0[k]), f"initial {k}: the two agents do not start from the same state"
    changed = 0
    for k in h:
        assert torch.equal(bits(h[k].reshape(-1)), bits(f[k].reshape(-1))) if h[k].dtype == torch.float32 else torch.equal(h[k], f[k]), k
        changed += int(not torch.equal(h[k], h0[k]))
    assert changed >= 4 and np.isfinite(hi["train/critic_loss"]) and hi["train/critic_loss"] == fi["train/critic_loss"]
    with pytest.raises(ValueError, match="algo.replay_obs_dtype"):
        from pql_amd.replay.simple_replay import cfg_obs_dtype
        from pql_amd.utils.cfg import load_cfg
        cfg_obs_dtype(load_cfg([f"algo={algo}_algo", "algo.replay_obs_dtype=bfloat16"]).algo)


# ------------------------------------------------------------------------------------------------ entry points
PM_SMALL = ["task=pointmass", "num_envs=64", "algo.batch_size=256", "algo.memory_size=20000", "algo.num_gpus=1", "algo.hidden_layers=[128, 128]",
            "algo.distl=False", "algo.graph=True"]
H16, F32 = "algo.replay_obs_dtype=float16", "algo.replay_obs_dtype=float32"


_CK16 = {}


def _half_way_fp16(tmp_path):
    """B1: the float16 run stopped at 3000 steps with a checkpoint (made once, used by both tests below)."""
    if "b1" not in _CK16:
        ck = tmp_path / "ck16"
        _CK16["b1"] = child(PQL, PM_SMALL + [H16, "max_step=3000", f"checkpoint.dir={ck}"], tmp_path)
        _CK16["ck"] = ck
    return _CK16["ck"], _CK16["b1"]


def test_train_pql_on_fp16_rings_runs_and_resumes_bit_exact(tmp_path):
    """scripts/train_pql.py task=pointmass algo.replay_obs_dtype=float16 at the small shape (fresh child processes, the helpers of
    tests/test_resume_gpu.py): A runs to max_step with finite losses; B1 stops half way with a checkpoint, B2 resumes it and ends with
    A's bits (scalar critic, graph mode)."""
    import math
    a = child(PQL, PM_SMALL + [H16, "max_step=6000"], tmp_path)
    assert a["resumed_from"] is None and a["rollout_iterations"] == 62 and a["global_steps"] > 6000
    assert math.isfinite(a["critic_loss"]) and math.isfinite(a["actor_loss"]) and a["critic_updates"] == 8 * 62
    ck, b1 = _half_way_fp16(tmp_path)
    assert b1["rollout_iterations"] == 15 and b1["critic_sha"] != a["critic_sha"]
    b2 = child(PQL, PM_SMALL + [H16, "max_step=6000", f"resume={ck}"], tmp_path)
    assert b2["resumed_from"]["global_steps"] == b1["global_steps"]
    same(a, b2, PQL_KEYS)


def test_a_checkpoint_of_the_other_format_is_refused_by_name(tmp_path):
    """A float16 checkpoint under algo.replay_obs_dtype=float32, and a float32 one under float16: ValueError naming obs_dtype."""
    ck, b1 = _half_way_fp16(tmp_path)
    r = child(PQL, PM_SMALL + [F32, "max_step=6000", f"resume={ck}"], tmp_path, check=False)
    assert r.returncode != 0 and "ValueError" in r.stderr and "obs_dtype" in r.stderr and "float16" in r.stderr, r.stderr[-2000:]
    ck32 = tmp_path / "ck32"
    c1 = child(PQL, PM_SMALL + ["max_step=3000", f"checkpoint.dir={ck32}"], tmp_path)      # the default: float32
    assert c1["replay_sha"] != b1["replay_sha"]
    r = child(PQL, PM_SMALL + [H16, "max_step=6000", f"resume={ck32}"], tmp_path, check=False)
    assert r.returncode != 0 and "ValueError" in r.stderr and "obs_dtype" in r.stderr and "float32" in r.stderr, r.stderr[-2000:]


# ------------------------------------------------------------------------------------------------ it still learns
LEARN_ITERS = 1000
# profiles/pointmass_learning_fp16.json (tools/learn_pointmass.py --override algo.replay_obs_dtype=float16, seeds 0-4): DDPG small
# f = 0.9684 0.9614 0.9634 0.9741 0.9500; the rule of DESIGN section 10 f7: half of the lowest of the five
F_MIN_FP16 = 0.5 * 0.9500


def test_ddpg_learns_pointmass_on_fp16_rings():
    """DDPG on PointMass small (obs 8, act 2, 64 envs, batch 256, hidden [128, 128], 1000 iterations, seed 0) with
    algo.replay_obs_dtype=float16 closes at least F_MIN_FP16 = 0.5 x 0.9500 = 0.475 of the gap between the zero action and the PD
    controller, as test_ddpg_learns_pointmass does with fp32 rings (f_min 0.473).  Source of the value:
    profiles/pointmass_learning_fp16.json, DDPG small, seeds 0-4: f = 0.9684, 0.9614, 0.9634, 0.9741, 0.9500; half of the lowest
    (the half covers seed-to-seed and box-to-box spread; the yardsticks depend on no learner kernel).  DESIGN section 10 f8."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("learn_pointmass_fp16", os.path.join(ROOT, "tools", "learn_pointmass.py"))
    lp = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(lp)
    r = lp.run("ddpg", "small", 0, LEARN_ITERS, extra=(H16,))
    print(f"pointmass ddpg fp16 rings seed 0, {LEARN_ITERS} iterations: R={r['R']:.3f} R_zero={r['R_zero']:.3f} R_pd={r['R_pd']:.3f} "
          f"f={r['f']:.4f} wall={r['wall_s']}s")
    assert r["R_pd"] > r["R_zero"]
    assert r["f"] >= F_MIN_FP16, r
