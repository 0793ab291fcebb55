"""The scalar twin critic's TD step, kernel by kernel, against a float64 reference on exactly summable data:
pqlk_mlp_backward_td (k_skinny_bwd<1, CH, true> at CH = 1 / 2 / 4 and 16 / 32 / 64 rows per block), pqlk_mlp_forward_td +
pqlk_mlp_backward_td_tail (the TD part of fused_head under k_mlp_fwd_fused<1, 2> / <2, 2> / <1, 4>, one and two chunks of its quad
loop), pqlk_mlp_backward_layers with the TD inputs, the squared-norm partials of pqlk_mlp_backward_norm and of the TD entries, and
pqlk_adamw_polyak_fused with prenorm > 0 and the loss fold.  Cases, inputs, mirror and references: tests/backward_cases.py (the
TD family), proved without a GPU in tests/test_backward_cases_cpu.py.

For B a power of two 2.0f / B is exact and every gradient element has ONE right value: the arena is compared with `==`.  For any
other B dL/dQ is rounded once (dy = float32(2) / float32(B) * dq) and the TD paths must leave the bits pqlk_mlp_backward leaves
when fed that dy -- everywhere for pqlk_mlp_backward_td (the documented contract), in the hidden layers for the forward path, whose
head sums run in other groups and are held to (B + 8) 2^-24 sum_b |dy_b h_bk| of the float64 sum.  The loss partials are sums of
unscaled dq^2: exact at every B.  Workspaces, gradients and partials start as NaN; every buffer is guarded."""
import ctypes as C

import numpy as np
import pytest
import torch

import backward_cases as bc
import reduction_cases as rc
from backward_job import Guarded, _returned, _sync_or_stop
from support import dev  # noqa: F401

pytestmark = pytest.mark.gpu

T = rc.T
F32, F64 = np.float32, np.float64
POISON, SLACK, IN_ONE = bc.POISON, bc.SLACK, bc.IN_ONE
NAN = float("nan")
PART_ROOM = 2048          # floats of room in loss_part and sumsq_part (include/pqlk.h)
STEP0 = 5                 # the device step counter before a call that must move it by exactly 1


def _same(a, b):
    """Bit equality of two device tensors, NaN payloads included."""
    return bool((a.view(torch.int32) == b.view(torch.int32)).all())


class TdJob:
    """One TD case on the device.  Inputs (guarded in front and behind with 1.0): arena, x, the target stash, rew, done, and on
    path "bwd" the online stash.  Outputs (NaN, poison behind): ws, grads, loss_part, sumsq_part, and on path "fwd" the stash."""

    def __init__(self, dev, name=None, problem=None):
        from pql_amd import _lib as L
        self.p = p = problem if problem is not None else bc.td_problem(name)
        self.dev, self.case, self.name = dev, p.case, p.case.name
        c = self.case
        self.desc = L.mlp_desc(c.dims, 2)
        self.arena = Guarded(dev, (bc.net_stride(c.dims) * 2,), IN_ONE, bc.td_arena(p), off=SLACK)
        self.x = Guarded(dev, (c.B, c.ldx), IN_ONE, np.array(p.x), off=SLACK)
        self.acts_t = Guarded(dev, (bc.acts_floats(c.dims, 2, c.B),), IN_ONE, bc.td_target_stash(p), off=SLACK)
        self.rew = Guarded(dev, (c.B,), IN_ONE, p.rew.astype(F32), off=SLACK)
        self.done = Guarded(dev, (c.B,), IN_ONE, p.done.astype(F32), off=SLACK)
        self.dy = Guarded(dev, (2, c.B, 32), IN_ONE, np.array(p.dy), off=SLACK)
        self.inputs = [self.arena, self.x, self.acts_t, self.rew, self.done, self.dy]
        self.acts = None
        if p.tc.path == "bwd":
            self.acts = Guarded(dev, (self.acts_t.n,), IN_ONE, bc.td_stash(p), off=SLACK)
            self.inputs.append(self.acts)
        self.gamma_n = bc.GAMMA_N
        self.ws_floats = int(L.lib.pqlk_mlp_bwd_ws_floats(C.byref(self.desc), c.B, c.splits))
        assert self.ws_floats == bc.bwd_ws_floats(c.dims, 2, c.B, c.splits)
        self.ws = Guarded(dev, (self.ws_floats,), POISON, body=NAN)
        self.norm_parts = int(L.lib.pqlk_mlp_norm_parts(C.byref(self.desc)))
        assert self.norm_parts == bc.norm_parts(c.dims, 2) <= PART_ROOM
        self.step = Guarded(dev, (1,), 77, init=np.array([STEP0], dtype=np.int32), dtype=torch.int32)
        self.packed = None
        self.fresh_outputs()
        self.seal()

    def seal(self):
        self.before = [g.full.clone() for g in self.inputs]

    def fresh_outputs(self):
        self.grads = Guarded(self.dev, (self.arena.n,), POISON, body=NAN)
        self.loss = Guarded(self.dev, (PART_ROOM,), POISON, body=NAN)
        self.sumsq = Guarded(self.dev, (PART_ROOM,), POISON, body=NAN)

    def fresh_stash(self):
        return Guarded(self.dev, (self.acts_t.n,), POISON, body=NAN)

    def pack(self):
        from pql_amd import _lib as L
        n = int(L.lib.pqlk_mlp_packed_floats(C.byref(self.desc)))
        assert n > 0
        self.packed = Guarded(self.dev, (n,), IN_ONE, body=NAN, off=SLACK)
        assert _returned(L.lib.pqlk_mlp_pack(C.byref(self.desc), L.ptr(self.arena.t), L.ptr(self.packed.t), L.stream(self.dev)), "pqlk_mlp_pack") == 0
        _sync_or_stop(f"pqlk_mlp_pack on {self.name}")
        assert self.packed.intact() and not bool(torch.isnan(self.packed.t).any())
        self.inputs.append(self.packed)
        self.seal()

    # ---- the entry points
    def _done(self, rcode, what):
        _returned(rcode, f"{what} on {self.name}")
        _sync_or_stop(f"{what} on {self.name}")
        return rcode

    def _norm_args(self, norm):
        from pql_amd import _lib as L
        return (L.ptr(self.sumsq.t), L.ptr(self.step.t)) if norm else (None, None)

    def backward_td(self, norm=False):
        from pql_amd import _lib as L
        c = self.case
        return self._done(L.lib.pqlk_mlp_backward_td(
            C.byref(self.desc), L.ptr(self.arena.t), L.ptr(self.x.t), c.ldx, c.B, L.ptr(self.acts.t), L.ptr(self.acts_t.t), L.ptr(self.rew.t),
            L.ptr(self.done.t), self.gamma_n, L.ptr(self.loss.t), L.ptr(self.grads.t), c.splits, L.ptr(self.ws.t), self.ws_floats,
            *self._norm_args(norm), L.stream(self.dev)), "pqlk_mlp_backward_td")

    def backward(self, acts, norm=False):
        """pqlk_mlp_backward (norm: pqlk_mlp_backward_norm) fed the host's dy."""
        from pql_amd import _lib as L
        c = self.case
        head = (C.byref(self.desc), L.ptr(self.arena.t), L.ptr(self.x.t), c.ldx, c.B, L.ptr(acts.t), L.ptr(self.dy.t), L.ptr(self.grads.t),
                c.splits, None, 0, 0, 0, None, 0, L.ptr(self.ws.t), self.ws_floats)
        if norm:
            return self._done(L.lib.pqlk_mlp_backward_norm(*head, *self._norm_args(True), L.stream(self.dev)), "pqlk_mlp_backward_norm")
        return self._done(L.lib.pqlk_mlp_backward(*head, L.stream(self.dev)), "pqlk_mlp_backward")

    def layers(self, hi, lo):
        from pql_amd import _lib as L
        c = self.case
        return self._done(L.lib.pqlk_mlp_backward_layers(
            C.byref(self.desc), L.ptr(self.arena.t), L.ptr(self.x.t), c.ldx, c.B, L.ptr(self.acts.t), None, L.ptr(self.acts_t.t),
            L.ptr(self.rew.t), L.ptr(self.done.t), self.gamma_n, L.ptr(self.loss.t), L.ptr(self.grads.t), c.splits, L.ptr(self.ws.t),
            self.ws_floats, hi, lo, L.stream(self.dev)), f"pqlk_mlp_backward_layers({hi}, {lo})")

    def forward(self, acts):
        from pql_amd import _lib as L
        c = self.case
        return self._done(L.lib.pqlk_mlp_forward(C.byref(self.desc), L.ptr(self.arena.t), L.ptr(self.packed.t), 1, L.ptr(self.x.t), c.ldx, c.B,
                                                 L.ACT_NONE, None, 0.0, 0.0, L.ptr(acts.t), None, 0, L.stream(self.dev)), "pqlk_mlp_forward")

    def forward_td(self, acts):
        from pql_amd import _lib as L
        c = self.case
        return self._done(L.lib.pqlk_mlp_forward_td(
            C.byref(self.desc), L.ptr(self.arena.t), L.ptr(self.packed.t), L.ptr(self.x.t), c.ldx, c.B, L.ptr(acts.t), L.ptr(self.acts_t.t),
            L.ptr(self.rew.t), L.ptr(self.done.t), self.gamma_n, L.ptr(self.loss.t), L.ptr(self.ws.t), self.ws_floats, c.splits,
            L.stream(self.dev)), "pqlk_mlp_forward_td")

    def tail(self, acts, norm=False):
        from pql_amd import _lib as L
        c = self.case
        return self._done(L.lib.pqlk_mlp_backward_td_tail(
            C.byref(self.desc), L.ptr(self.arena.t), L.ptr(self.x.t), c.ldx, c.B, L.ptr(acts.t), L.ptr(self.grads.t), c.splits,
            L.ptr(self.ws.t), self.ws_floats, *self._norm_args(norm), L.stream(self.dev)), "pqlk_mlp_backward_td_tail")

    # ---- the checks
    def assert_guards(self, what, *more):
        for g in (self.ws, self.grads, self.loss, self.sumsq, self.step) + more:
            assert g.intact(), f"{what}: slack behind a written buffer was written"
        for g, b in zip(self.inputs, self.before):
            assert _same(g.full, b), f"{what}: an input buffer or its slack was written"

    def check_loss(self, parts_fn, what):
        """loss_part[0, parts) == the float64 sum of dq^2 of each (row block, net); nothing is written behind that range."""
        from pql_amd import _lib as L
        want = bc.td_loss_parts(self.name)
        assert int(parts_fn(C.byref(self.desc), self.case.B)) == len(want), what
        got = self.loss.host()
        bad = np.argwhere(~(got[: len(want)].astype(F64) == want))
        assert bad.size == 0, f"{what}: {len(bad)} loss partials differ, first at {int(bad[0][0])}: {got[bad[0][0]]} != {want[bad[0][0]]}"
        assert np.isnan(got[len(want):]).all(), f"{what}: loss_part written behind its {len(want)} partials"
        return got

    def check_sumsq(self, want, what):
        """The float64 sum of sumsq_part[0, pqlk_mlp_norm_parts) == sum g^2; nothing is written behind that range."""
        got = self.sumsq.host()
        assert not np.isnan(got[: self.norm_parts]).any(), f"{what}: a squared-norm partial was not written"
        assert np.isnan(got[self.norm_parts:]).all(), f"{what}: sumsq_part written behind its {self.norm_parts} partials"
        total = float(got[: self.norm_parts].astype(F64).sum())
        assert total == want, f"{what}: the squared-norm partials sum to {total}, sum g^2 is {want}"

    def step_value(self):
        return int(self.step.t.cpu()[0])


def _hidden_and_head(dims):
    """Arena index masks: (hidden layers, head) over both nets."""
    head = np.zeros(bc.net_stride(dims) * 2, dtype=bool)
    for net in range(2):
        a, b = bc.head_range(dims, net)
        head[a:b] = True
    return ~head, head


# ------------------------------------------------------------------------------------------------ pqlk_mlp_backward_td
@pytest.mark.parametrize("name", bc.TD_BWD_NAMES)
def test_backward_td_case(dev, name):
    """One pqlk_mlp_backward_td over a NaN workspace: the whole arena carries the bits pqlk_mlp_backward leaves when fed dy =
    2 / B dq (every B) and, for B a power of two, equals the float64 reference; each loss partial equals its block's sum of dq^2
    and nothing is written behind them; a second call over the dirty workspace leaves the same bits; with sumsq_part and step_dev
    the gradient bits are the same and the step counter has moved by exactly 1."""
    from pql_amd import _lib as L
    job = TdJob(dev, name)
    tc = job.p.tc
    assert job.backward_td() == 0
    grads1 = job.grads.host()
    loss1 = job.check_loss(L.lib.pqlk_td_head_loss_parts, name)
    job.assert_guards(name)
    assert not np.isnan(grads1).any(), f"{name}: the arena holds NaN"
    if bc.is_pow2(tc.B):
        bc.check_grads(grads1, job.case, ref=bc.td_reference(name), what=name)
    assert bool(torch.isnan(job.sumsq.t).all()) and job.step_value() == STEP0, f"{name}: sumsq_part / step_dev touched without being given"
    # ---- the documented contract: the bits of pqlk_mlp_backward fed dy
    job.fresh_outputs()
    job.ws.t.fill_(NAN)
    assert job.backward(job.acts) == 0
    plain = job.grads.host()
    assert bc.bits_equal(grads1, plain), f"{name}: not the gradient of pqlk_mlp_backward fed 2 / B dq"
    # ---- again, over the workspace the calls left
    job.fresh_outputs()
    assert job.backward_td() == 0
    assert bc.bits_equal(job.grads.host(), grads1), f"{name}: the second call leaves other gradient bits"
    assert bc.bits_equal(job.check_loss(L.lib.pqlk_td_head_loss_parts, f"{name} second call"), loss1)
    # ---- with the squared-norm partials and the step increment
    job.fresh_outputs()
    assert job.backward_td(norm=True) == 0
    assert bc.bits_equal(job.grads.host(), grads1), f"{name}: sumsq_part changes the gradient bits"
    assert bc.bits_equal(job.check_loss(L.lib.pqlk_td_head_loss_parts, f"{name} with sumsq_part"), loss1)
    assert job.step_value() == STEP0 + 1, f"{name}: step_dev moved by {job.step_value() - STEP0}"
    got = job.sumsq.host()
    assert not np.isnan(got[: job.norm_parts]).any() and np.isnan(got[job.norm_parts:]).all()
    job.assert_guards(f"{name} with sumsq_part")
    print(f"TDPATH {name} k_skinny_bwd<1, CH, true> (CH, rows)={bc.td_instance(tc)} loss_parts={len(loss1[~np.isnan(loss1)])} "
          f"exact_arena={bc.is_pow2(tc.B)}")


@pytest.mark.parametrize("name", bc.TD_LAYERS_NAMES)
def test_backward_layers_with_td_leave_the_single_call_bits(dev, name):
    """pqlk_mlp_backward_layers given the four TD inputs, in the learner's buckets and in one bucket per layer: together the calls
    leave the arena bits and the loss_part bits of one pqlk_mlp_backward_td call."""
    from pql_amd import _lib as L
    from pql_amd.utils.dp import layer_buckets
    job = TdJob(dev, name)
    assert job.backward_td() == 0
    single, loss = job.grads.host(), job.check_loss(L.lib.pqlk_td_head_loss_parts, name)
    n_layers = len(job.case.dims) - 1
    for buckets in (layer_buckets(n_layers), [(l, l) for l in range(n_layers - 1, -1, -1)]):
        job.fresh_outputs()
        job.ws.t.fill_(NAN)
        for hi, lo in buckets:
            assert job.layers(hi, lo) == 0
        assert bc.bits_equal(job.grads.host(), single), (name, buckets)
        assert bc.bits_equal(job.check_loss(L.lib.pqlk_td_head_loss_parts, f"{name} buckets {buckets}"), loss), (name, buckets)
        job.assert_guards(f"{name} buckets {buckets}")


# ------------------------------------------------------------------------------------------------ pqlk_mlp_forward_td + _tail
def _check_forward_td_stash(job, got, ref, what):
    """Every block but the last hidden layer's carries the forward's bits (pads zero); the last hidden block is left unwritten."""
    dims, B = job.case.dims, job.case.B
    lo, _ = bc.act_offset(dims, 2, B, 0, len(dims) - 3)
    hi, _ = bc.act_offset(dims, 2, B, 0, len(dims) - 2)
    assert bc.bits_equal(got[:lo], ref[:lo]), f"{what}: a hidden block below the last differs from pqlk_mlp_forward's"
    assert bc.bits_equal(got[hi:], ref[hi:]), f"{what}: the Q block differs from pqlk_mlp_forward's"
    assert np.isnan(got[lo:hi]).all(), f"{what}: the last hidden layer's block was written"


@pytest.mark.parametrize("name", bc.TD_FWD_NAMES)
def test_forward_td_case(dev, name):
    """pqlk_mlp_forward(packed, stash_all = 1, NONE) on the exactly evaluable network leaves exactly the float64 activations and Q;
    pqlk_mlp_forward_td leaves the same bits in every block but the last hidden layer's, which stays NaN, and one exact loss
    partial per (row tile, net); after pqlk_mlp_backward_td_tail the arena equals the float64 reference for B a power of two; at
    every B the hidden layers carry the bits of pqlk_mlp_backward fed dy = 2 / B dq and the head's dW / db lie within
    (B + 8) 2^-24 sum_b |dy_b h_bk| of their float64 sums.  A second round over the dirty buffers leaves the same bits."""
    from pql_amd import _lib as L
    job = TdJob(dev, name)
    tc, case = job.p.tc, job.case
    job.pack()
    # ---- the plain forward: the premise of the exact reference, and the bits the TD forward must repeat
    acts_ref = job.fresh_stash()
    assert job.forward(acts_ref) == 0
    stash = acts_ref.host()
    want = bc.td_stash(job.p)
    bad = np.argwhere(~(stash == want))
    assert bad.size == 0, f"{name}: the forward's stash differs from the exact network at {int(bad[0][0])}: {stash[bad[0][0]]} != {want[bad[0][0]]}"
    # ---- the TD forward
    acts = job.fresh_stash()
    assert job.forward_td(acts) == 0
    _check_forward_td_stash(job, acts.host(), stash, name)
    loss1 = job.check_loss(L.lib.pqlk_td_forward_loss_parts, name)
    assert bool(torch.isnan(job.grads.t).all())
    job.assert_guards(name, acts, acts_ref)
    # ---- the tail
    assert job.tail(acts) == 0
    grads1 = job.grads.host()
    assert not np.isnan(grads1).any(), f"{name}: the arena holds NaN"
    ref = bc.td_reference(name)
    if bc.is_pow2(tc.B):
        bc.check_grads(grads1, case, ref=ref, what=name)
    job.assert_guards(f"{name} tail", acts, acts_ref)
    # ---- against pqlk_mlp_backward on the forward's full stash, fed the host's dy
    ws_td = job.ws
    job.ws = Guarded(dev, (job.ws_floats,), POISON, body=NAN)
    job.fresh_outputs()
    assert job.backward(acts_ref) == 0
    plain = job.grads.host()
    hidden, head = _hidden_and_head(case.dims)
    assert bc.bits_equal(grads1[hidden], plain[hidden]), f"{name}: hidden-layer gradients are not those of pqlk_mlp_backward fed 2 / B dq"
    bound = bc.head_sum_bound(job.p, ref)[head]
    err = np.abs(grads1[head].astype(F64) - ref["grads"][head])
    ratio = float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0
    print(f"TDPATH {name} k_mlp_fwd_fused<R, TM> (R, TM)={bc.td_instance(tc)} loss_parts={len(bc.td_loss_parts(name))} "
          f"exact_arena={bc.is_pow2(tc.B)} head_err_over_bound={ratio:.3g}")
    assert np.all(err <= bound), f"{name}: the head's sums leave the bound, worst ratio {ratio}"
    job.assert_guards(f"{name} plain backward", acts, acts_ref)
    # ---- a second round over the dirty stash and workspace, now with the squared-norm partials
    job.ws = ws_td
    job.fresh_outputs()
    assert job.forward_td(acts) == 0
    _check_forward_td_stash(job, acts.host(), stash, f"{name} second round")
    assert bc.bits_equal(job.check_loss(L.lib.pqlk_td_forward_loss_parts, f"{name} second round"), loss1)
    assert job.tail(acts, norm=True) == 0
    assert bc.bits_equal(job.grads.host(), grads1), f"{name}: the second round leaves other gradient bits"
    assert job.step_value() == STEP0 + 1, f"{name}: step_dev moved by {job.step_value() - STEP0}"
    got = job.sumsq.host()
    assert not np.isnan(got[: job.norm_parts]).any() and np.isnan(got[job.norm_parts:]).all()
    job.assert_guards(f"{name} second round", acts, acts_ref)


def test_forward_td_is_refused_one_step_past_its_eligibility_edge(dev):
    """[8, 288, 32, 1] (256 + 4 free LDS columns beside the last hidden layer) is taken -- the cases above; [8, 256, 32, 1] (228)
    returns PQLK_E_UNSUPPORTED from pqlk_mlp_forward_td and from pqlk_mlp_backward_td_tail, and no output byte changes."""
    from pql_amd import _lib as L
    B = 33
    tc = bc.TdCase("refused", list(bc.TD_REFUSED), B, 1, "fwd", "std")
    case = bc.td_as_case(tc)
    W, bias, x = bc.exact_network(case)
    _, H, q = bc.exact_forward(case, W, bias, x)
    z = np.zeros((2, B))
    p = bc.SimpleNamespace(tc=tc, case=case, W=W, bias=bias, H=H, x=x, q=q, qt=z, rew=z[0], done=z[0], dq=z, dy=np.zeros((2, B, 32), dtype=F32))
    job = TdJob(dev, problem=p)
    job.pack()
    d = C.byref(job.desc)
    assert int(L.lib.pqlk_td_forward_loss_parts(d, B)) == 0 and int(L.lib.pqlk_td_forward_loss_parts(C.byref(L.mlp_desc(bc.TD_TAKEN, 2)), B)) == 4
    acts = job.fresh_stash()
    outs = [acts, job.ws, job.grads, job.loss, job.sumsq, job.step]
    before = [g.full.clone() for g in outs]
    assert job.forward_td(acts) == L.E_UNSUPPORTED
    assert job.tail(acts) == L.E_UNSUPPORTED
    assert job.tail(acts, norm=True) == L.E_UNSUPPORTED
    for g, b in zip(outs, before):
        assert _same(g.full, b), "a refused call wrote an output"
    job.assert_guards("refused", acts)
    # the plain forward still takes the layout: the refusal is the TD path's alone
    assert job.forward(acts) == 0
    assert np.array_equal(acts.host(), bc.td_stash(p))


# ------------------------------------------------------------------------------------------------ the squared-norm partials
@pytest.mark.parametrize("name", bc.TD_NORM_BWD_NAMES)
def test_sumsq_partials_of_the_backward_count_every_element_once(dev, name):
    """Integer gradients with sum g^2 <= 2^24: the float64 sum of sumsq_part[0, pqlk_mlp_norm_parts) equals sum g^2 out of
    pqlk_mlp_backward_norm (fused head: main blocks + head fold blocks) and out of pqlk_mlp_backward_td.  On the head-only case
    everything but the head's dW / db is zero: a head counted twice or not at all fails outright."""
    job = TdJob(dev, name)
    ref = bc.td_reference(name)
    assert bc.head_is_fused(job.case.dims) and job.norm_parts > bc.cdiv(bc.net_stride(job.case.dims) * 2 // 4, 256)
    for entry in ("pqlk_mlp_backward_norm", "pqlk_mlp_backward_td"):
        what = f"{name} {entry}"
        job.fresh_outputs()
        job.ws.t.fill_(NAN)
        before = job.step_value()
        assert (job.backward(job.acts, norm=True) if entry == "pqlk_mlp_backward_norm" else job.backward_td(norm=True)) == 0
        bc.check_grads(job.grads.host(), job.case, ref=ref, what=what)
        job.check_sumsq(ref["sumsq"], what)
        assert job.step_value() == before + 1, what
        job.assert_guards(what)


@pytest.mark.parametrize("name", bc.TD_NORM_FWD_NAMES)
def test_sumsq_partials_of_the_td_tail_count_every_element_once(dev, name):
    job = TdJob(dev, name)
    ref = bc.td_reference(name)
    job.pack()
    acts = job.fresh_stash()
    assert job.forward_td(acts) == 0
    assert job.tail(acts, norm=True) == 0
    bc.check_grads(job.grads.host(), job.case, ref=ref, what=name)
    job.check_sumsq(ref["sumsq"], name)
    assert job.step_value() == STEP0 + 1
    job.assert_guards(name, acts)


def test_sumsq_partials_with_a_head_that_is_not_fused(dev):
    """pqlk_mlp_backward_norm with 16 outputs on K = 512 (k_skinny_dw + k_skinny_dx: the head goes through the slabs and the main
    blocks of the reduction count it): integer gradients, the partials sum to sum g^2 exactly."""
    from pql_amd import _lib as L
    case = bc.norm_plain_case()
    want = bc.norm_plain_reference(case)
    desc = L.mlp_desc(case.dims, 2)
    parts = int(L.lib.pqlk_mlp_norm_parts(C.byref(desc)))
    assert parts == bc.norm_parts(case.dims, 2) and not bc.head_is_fused(case.dims)
    arena = Guarded(dev, (bc.net_stride(case.dims) * 2,), IN_ONE, bc.arena(case), off=SLACK)
    acts = Guarded(dev, (bc.acts_floats(case.dims, 2, case.B),), IN_ONE, bc.norm_plain_stash(case), off=SLACK)
    x = Guarded(dev, (case.B, case.ldx), IN_ONE, bc.x_input(case), off=SLACK)
    dy = Guarded(dev, (2, case.B, bc.ld(case.dims[-1])), IN_ONE, bc.dy_input(case), off=SLACK)
    ws_floats = int(L.lib.pqlk_mlp_bwd_ws_floats(C.byref(desc), case.B, case.splits))
    ws = Guarded(dev, (ws_floats,), POISON, body=NAN)
    grads = Guarded(dev, (arena.n,), POISON, body=NAN)
    sumsq = Guarded(dev, (PART_ROOM,), POISON, body=NAN)
    step = Guarded(dev, (1,), 77, init=np.array([STEP0], dtype=np.int32), dtype=torch.int32)
    rcode = L.lib.pqlk_mlp_backward_norm(C.byref(desc), L.ptr(arena.t), L.ptr(x.t), case.ldx, case.B, L.ptr(acts.t), L.ptr(dy.t), L.ptr(grads.t),
                                         case.splits, None, 0, 0, 0, None, 0, L.ptr(ws.t), ws_floats, L.ptr(sumsq.t), L.ptr(step.t), L.stream(dev))
    assert _returned(rcode, "pqlk_mlp_backward_norm") == 0
    _sync_or_stop("pqlk_mlp_backward_norm on a non-fused head")
    g = grads.host()
    assert np.array_equal(g.astype(F64), want)
    got = sumsq.host()
    assert not np.isnan(got[:parts]).any() and np.isnan(got[parts:]).all()
    assert float(got[:parts].astype(F64).sum()) == float((want * want).sum())
    assert int(step.t.cpu()[0]) == STEP0 + 1
    for b in (ws, grads, sumsq, step, arena, acts, x, dy):
        assert b.intact()


# ------------------------------------------------------------------------------------------------ pqlk_adamw_polyak_fused
RING_LEN = 4
HYPER = dict(lr=5e-4, b1=0.9, b2=0.999, eps=1e-8, wd=1e-2, tau=0.05)
MAX_NORM = 0.5


class _Opt:
    """p, m, v, target, the step counter at 0, gnorm, scratch, the loss ring (poison): one optimiser state on the device."""

    def __init__(self, dev, n):
        self.p = Guarded(dev, (n,), POISON, bc.dd.uniform((n,), 901, -1.0, 1.0))
        self.m = Guarded(dev, (n,), POISON, bc.dd.uniform((n,), 902, -0.5, 0.5))
        self.v = Guarded(dev, (n,), POISON, bc.dd.uniform((n,), 903, 0.0, 1.0))
        self.target = Guarded(dev, (n,), POISON, bc.dd.uniform((n,), 904, -1.0, 1.0))
        self.step = Guarded(dev, (1,), 77, init=np.array([0], dtype=np.int32), dtype=torch.int32)
        self.gnorm = Guarded(dev, (1,), POISON, body=NAN)
        self.scratch = Guarded(dev, (PART_ROOM,), POISON, body=NAN)
        self.ring = Guarded(dev, (RING_LEN,), POISON, body=POISON)

    def state(self):
        return [g.host() for g in (self.p, self.m, self.v, self.target, self.gnorm)]

    def intact(self):
        return all(g.intact() for g in (self.p, self.m, self.v, self.target, self.step, self.gnorm, self.scratch, self.ring))


@pytest.mark.parametrize("route", ["norm", "td", "fwd"])
def test_fused_optimiser_on_exact_partials_leaves_the_stand_alone_bits(dev, route):
    """The squared-norm partials are exact sums of integers, so pqlk_mlp_backward_norm / pqlk_mlp_backward_td /
    pqlk_mlp_backward_td_tail (each with sumsq_part and step_dev) followed by pqlk_adamw_polyak_fused(prenorm =
    pqlk_mlp_norm_parts) leave p, m, v, target and gnorm bit for bit as pqlk_mlp_backward + pqlk_clip_adamw_polyak on the same
    gradient do, the step counter ends at 1, and with loss_part given loss_ring[(t - 1) % ring_len] == fl(S * scale), S the exact
    sum of dq^2 and scale = 1 / B a power of two, every other ring slot untouched."""
    from pql_amd import _lib as L
    name = bc.TD_NORM_FWD_NAMES[0] if route == "fwd" else bc.TD_NORM_BWD_NAMES[0]
    job = TdJob(dev, name)
    n, B = job.arena.n, job.case.B
    h = HYPER
    stream = L.stream(dev)
    # ---- the stand-alone pair on the same gradient
    acts = job.acts
    if route == "fwd":
        job.pack()
        acts = job.fresh_stash()
        assert job.forward(acts) == 0
    assert job.backward(acts) == 0
    bc.check_grads(job.grads.host(), job.case, ref=bc.td_reference(name), what=name)
    alone = _Opt(dev, n)
    rcode = L.lib.pqlk_clip_adamw_polyak(L.ptr(alone.p.t), L.ptr(job.grads.t), L.ptr(alone.m.t), L.ptr(alone.v.t), L.ptr(alone.target.t), n, 1.0,
                                         MAX_NORM, h["lr"], h["b1"], h["b2"], h["eps"], h["wd"], h["tau"], L.ptr(alone.step.t),
                                         L.ptr(alone.gnorm.t), L.ptr(alone.scratch.t), stream)
    assert _returned(rcode, "pqlk_clip_adamw_polyak") == 0
    _sync_or_stop("pqlk_clip_adamw_polyak")
    want = alone.state()
    assert float(want[4][0]) > MAX_NORM and int(alone.step.t.cpu()[0]) == 1        # the clip is active
    # ---- the fused pair
    fused = _Opt(dev, n)
    job.fresh_outputs()
    job.ws.t.fill_(NAN)
    job.sumsq, job.step = fused.scratch, fused.step
    if route == "norm":
        assert job.backward(job.acts, norm=True) == 0
    elif route == "td":
        assert job.backward_td(norm=True) == 0
    else:
        acts = job.fresh_stash()
        assert job.forward_td(acts) == 0
        assert job.tail(acts, norm=True) == 0
    assert int(fused.step.t.cpu()[0]) == 1
    loss_parts = 0 if route == "norm" else len(bc.td_loss_parts(name))
    rcode = L.lib.pqlk_adamw_polyak_fused(C.byref(job.desc), L.ptr(fused.p.t), L.ptr(job.grads.t), L.ptr(fused.m.t), L.ptr(fused.v.t),
                                          L.ptr(fused.target.t), None, None, 1.0, MAX_NORM, h["lr"], h["b1"], h["b2"], h["eps"], h["wd"],
                                          h["tau"], L.ptr(fused.step.t), L.ptr(fused.gnorm.t), L.ptr(fused.scratch.t), job.norm_parts,
                                          L.ptr(job.loss.t) if loss_parts else None, loss_parts, 1.0 / B, L.ptr(fused.ring.t) if loss_parts else None,
                                          RING_LEN if loss_parts else 0, stream)
    assert _returned(rcode, "pqlk_adamw_polyak_fused") == 0
    _sync_or_stop("pqlk_adamw_polyak_fused")
    for got, ref, what in zip(fused.state(), want, ("p", "m", "v", "target", "gnorm")):
        assert bc.bits_equal(got, ref), f"{route}: {what} differs from the stand-alone pair"
    assert int(fused.step.t.cpu()[0]) == 1
    ring = fused.ring.host()
    if loss_parts:
        S = float((job.p.dq ** 2).sum())
        assert ring[0] == F32(F32(S) * F32(1.0 / B)) and F32(S) == S
    else:
        assert ring[0] == POISON
    assert np.all(ring[1:] == POISON), f"{route}: a ring slot beside (t - 1) % ring_len was written"
    assert fused.intact() and alone.intact()
    job.assert_guards(route)


# ------------------------------------------------------------------------------------------------ operand order
def _db_of(grads, dims):
    ns = bc.net_stride(dims)
    _, bo = bc.layer_offsets(dims, len(dims) - 2)
    return np.array([grads[bo], grads[ns + bo]], dtype=F32)


def test_td_error_is_formed_in_the_documented_operand_order(dev):
    """B = 1, non-dyadic fp32 inputs, gamma^n = 0.99 (backward_cases.ORDER: values at which another order moves the last bit): the
    head's db of each net equals 2 (Q - (r + ((1 - d) gamma^n) min Q')) as numpy float32 evaluates it in that order, out of
    pqlk_mlp_backward_td and out of pqlk_mlp_forward_td + the tail."""
    p = bc.order_problem(bc.ORDER_BWD_NAME)
    job = TdJob(dev, problem=p)
    job.gamma_n = bc.ORDER["gamma_n"]
    assert job.backward_td() == 0
    got = _db_of(job.grads.host(), p.case.dims)
    want = np.array([bc.td_db_in_order(q) for q in p.q[:, 0]], dtype=F32)
    print(f"TDPATH operand order bwd: db={got} want={want}")
    assert np.array_equal(got, want), (got, want)
    p = bc.order_problem(bc.ORDER_FWD_NAME)
    job = TdJob(dev, problem=p)
    job.gamma_n = bc.ORDER["gamma_n"]
    job.pack()
    acts = job.fresh_stash()
    assert job.forward_td(acts) == 0
    assert job.tail(acts) == 0
    off, _ = bc.act_offset(p.case.dims, 2, 1, 0, len(p.case.dims) - 2)
    stash = acts.host()
    q = [stash[off], stash[off + 32]]
    assert np.array_equal(np.array(q, dtype=F64), p.q[:, 0])
    got = _db_of(job.grads.host(), p.case.dims)
    want = np.array([bc.td_db_in_order(v) for v in q], dtype=F32)
    print(f"TDPATH operand order fwd: db={got} want={want}")
    assert np.array_equal(got, want), (got, want)
