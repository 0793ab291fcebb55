"""The P-learner's default step, entry by entry, against a float64 reference: pqlk_dpg_backward_fused (k_dpg_minnet_head, the
compact dX products, k_dx_slice<D, QPW> at all four head-carrying instances) + pqlk_mlp_backward_tail (the actor's lower layers,
k_reduce_slabs folding the head partials of the tiles in use, with and without the squared-norm partials), and
pqlk_mlp_forward_qc in its concatenated and split input forms on an exactly evaluable network.  Cases, inputs, mirror, references
and checks: tests/dpg_fused_cases.py, proved without a GPU in tests/test_dpg_fused_cases_cpu.py.

The stash and qc are inputs the test writes (the backward never runs the forward); the partition and the loss partials are
compared with `==` at every B, the float outputs with `==` for B a power of two and within the derived bound otherwise.
Workspaces, gradients and partials start as NaN, dz_a as poison; every buffer is guarded."""
import ctypes as C

import numpy as np
import pytest
import torch

import backward_cases as bc
import dpg_fused_cases as fc
from backward_job import Guarded, _returned, _sync_or_stop
from support import dev  # noqa: F401

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
POISON, SLACK, IN_ONE = bc.POISON, bc.SLACK, bc.IN_ONE
NAN = float("nan")
PART_ROOM = 2048          # floats of room in sumsq_part (include/pqlk.h)
STEP0 = 5
LD_DZ = 32


def _same(a, b):
    return bool((a.view(torch.int32) == b.view(torch.int32)).all())


class FusedJob:
    """One case on the device.  Inputs (1.0 in front and behind): both arenas, both stashes, the observations, the tanh block,
    qc.  Outputs (NaN, poison behind): both workspaces, grads, loss_part, sumsq_part; dz_a is poison throughout."""

    def __init__(self, dev, p, c_acts=None, qc=None):
        from pql_amd import _lib as L
        self.dev, self.p, self.c = dev, p, p.c
        c, B = p.c, p.c.B
        self.A = A = c.adims[-1]
        self.cdesc, self.adesc = L.mlp_desc(c.cdims, 2), L.mlp_desc(c.adims, 1)
        self.c_arena = Guarded(dev, (bc.net_stride(c.cdims) * 2,), IN_ONE, fc.arena_of(c.cdims, p.Wc), off=SLACK)
        self.a_arena = Guarded(dev, (bc.net_stride(c.adims),), IN_ONE, fc.arena_of(c.adims, [p.Wa]), off=SLACK)
        self.c_acts = c_acts if c_acts is not None else Guarded(dev, (bc.acts_floats(c.cdims, 2, B),), IN_ONE, fc.stash_of(c.cdims, p.Hc, B), off=SLACK)
        self.a_acts = Guarded(dev, (bc.acts_floats(c.adims, 1, B),), IN_ONE, fc.stash_of(c.adims, [p.Ha], B), off=SLACK)
        self.x_obs = Guarded(dev, (B, 64), IN_ONE, fc.tiled(p.xa, B), off=SLACK)
        self.ld_tanh = fc.ld_tanh(c)
        self.a_out = Guarded(dev, (B, self.ld_tanh), IN_ONE, off=SLACK)
        self.a_out.t[:, :A] = bc.rc.T(fc.tiled(p.tanh, B)).to(dev)
        self.qc = qc if qc is not None else Guarded(dev, (2, B), IN_ONE, p.q, off=SLACK)
        self.inputs = [self.c_arena, self.a_arena, self.c_acts, self.a_acts, self.x_obs, self.a_out, self.qc]
        self.before = [g.full.clone() for g in self.inputs]
        self.ws = fc.compact_ws(bc.max_hidden_ld(c.cdims), B)
        self.ws_c_floats = int(L.lib.pqlk_dpg_backward_ws_floats(C.byref(self.cdesc), B))
        self.ws_a_floats = int(L.lib.pqlk_mlp_bwd_ws_floats(C.byref(self.adesc), B, c.splits))
        assert self.ws_c_floats == bc.dpg_ws_floats(c.cdims, 2, B) and self.ws_a_floats == bc.bwd_ws_floats(c.adims, 1, B, c.splits)
        self.mn_off = int(L.lib.pqlk_dpg_fused_mn_offset(C.byref(self.cdesc), B))
        self.head_parts = int(L.lib.pqlk_dpg_fused_head_parts(B))
        self.norm_parts = int(L.lib.pqlk_mlp_norm_parts(C.byref(self.adesc)))
        assert self.mn_off == self.ws["mn"] and self.head_parts == fc.head_parts(B) and self.norm_parts <= PART_ROOM
        self.ws_c = Guarded(dev, (self.ws_c_floats,), POISON, body=NAN)
        self.ws_a = Guarded(dev, (self.ws_a_floats,), POISON, body=NAN)
        self.step = Guarded(dev, (1,), 77, init=np.array([STEP0], dtype=np.int32), dtype=torch.int32)
        self.fresh_outputs()

    def fresh_outputs(self):
        self.grads = Guarded(self.dev, (self.a_arena.n,), POISON, body=NAN)
        self.dz_a = Guarded(self.dev, (self.c.B, LD_DZ), POISON)
        self.loss = Guarded(self.dev, (64,), POISON, body=NAN)
        self.sumsq = Guarded(self.dev, (PART_ROOM,), POISON, body=NAN)

    def outputs(self):
        return [self.ws_c, self.ws_a, self.grads, self.dz_a, self.loss, self.sumsq, self.step]

    def fused(self, B=None, ws_floats=None, a_ws_floats=None):
        from pql_amd import _lib as L
        c = self.c
        rcode = L.lib.pqlk_dpg_backward_fused(
            C.byref(self.cdesc), L.ptr(self.c_arena.t), None, bc.ld(c.cdims[0]), c.B if B is None else B, L.ptr(self.c_acts.t), L.ptr(self.qc.t),
            L.ptr(self.dz_a.t), LD_DZ, c.col0, L.ptr(self.a_out.t), self.ld_tanh, L.ptr(self.loss.t), L.ptr(self.ws_c.t),
            self.ws_c_floats if ws_floats is None else ws_floats, C.byref(self.adesc), L.ptr(self.a_arena.t), L.ptr(self.a_acts.t),
            L.ptr(self.ws_a.t), self.ws_a_floats if a_ws_floats is None else a_ws_floats, c.splits, L.stream(self.dev))
        _returned(rcode, f"pqlk_dpg_backward_fused on {c.name}")
        _sync_or_stop(f"pqlk_dpg_backward_fused on {c.name}")
        return rcode

    def tail(self, norm=False):
        from pql_amd import _lib as L
        c = self.c
        mn_ptr = C.c_void_p(self.ws_c.t.data_ptr() + 4 * self.mn_off)
        rcode = L.lib.pqlk_mlp_backward_tail(
            C.byref(self.adesc), L.ptr(self.a_arena.t), L.ptr(self.x_obs.t), 64, c.B, L.ptr(self.a_acts.t), L.ptr(self.grads.t), c.splits,
            L.ptr(self.ws_a.t), self.ws_a_floats, L.ptr(self.sumsq.t) if norm else None, L.ptr(self.step.t) if norm else None,
            self.head_parts, mn_ptr, L.stream(self.dev))
        _returned(rcode, f"pqlk_mlp_backward_tail on {c.name}")
        _sync_or_stop(f"pqlk_mlp_backward_tail on {c.name}")
        return rcode

    def assert_guards(self, what):
        for g in self.outputs():
            assert g.intact(), f"{what}: slack behind a written buffer was written"
        for g, b in zip(self.inputs, self.before):
            assert _same(g.full, b), f"{what}: an input buffer or its slack was written"

    def collect(self, with_grads=True):
        """What the calls left, as the checks of dpg_fused_cases take it; also asserts that the workspace's integer blocks are
        untouched behind the rows in use and behind mn."""
        w, cap = self.ws, self.ws["rows_cap"]
        ints = self.ws_c.t.view(torch.int32)
        perm, tie0 = ints[w["perm"]: w["perm"] + cap].cpu().numpy(), ints[w["tie0"]: w["tie0"] + cap].cpu().numpy()
        mn = ints[w["mn"]: w["mn"] + 64].cpu().numpy()
        nan_bits = np.array(NAN, dtype=F32).view(np.int32)
        used = int(mn[3])
        assert 0 <= used <= cap, f"{self.c.name}: mn[3] = {used}"
        assert (perm[used:] == nan_bits).all() and (tie0[used:] == nan_bits).all(), f"{self.c.name}: perm / tie0 written behind the rows in use"
        assert (mn[4:] == nan_bits).all(), f"{self.c.name}: the mn block written behind its four ints"
        Kh = bc.ld(self.c.adims[-2])
        return dict(perm=perm, tie0=tie0, mn=mn[:4], loss=self.loss.host(), dz_a=self.dz_a.host(),
                    dxh=self.ws_a.t[: self.c.B * Kh].view(self.c.B, Kh).cpu().numpy()[:, : self.c.adims[-2]],
                    grads=self.grads.host() if with_grads else None)

    def step_value(self):
        return int(self.step.t.cpu()[0])


def _run_and_check(job, ref, name):
    """fused -> checks -> tail -> checks -> a second round over the dirty workspaces.  Returns the worst err / bound."""
    assert job.fused() == 0
    out = job.collect(with_grads=False)
    fc.check_partition(out["perm"], out["tie0"], out["mn"], ref, name)
    fc.check_loss(out["loss"], ref, name)
    ratio = fc.check_floats(out["dz_a"], out["dxh"], None, ref, name)
    assert bool(torch.isnan(job.grads.t).all()), f"{name}: grads written before the tail"
    job.assert_guards(name)
    assert job.tail() == 0
    out = job.collect()
    assert not np.isnan(out["grads"]).any(), f"{name}: the arena holds NaN"
    ratio = max(ratio, fc.check_all(out, ref, f"{name} after the tail"))
    assert bool(torch.isnan(job.sumsq.t).all()) and job.step_value() == STEP0, f"{name}: sumsq_part / step_dev touched without being given"
    job.assert_guards(f"{name} tail")
    # ---- again, over the workspaces the calls left
    first = [g.full.clone() for g in job.outputs()]
    job.grads.t.fill_(NAN); job.dz_a.t.fill_(POISON); job.loss.t.fill_(NAN)
    assert job.fused() == 0 and job.tail() == 0
    for g, b, nm in zip(job.outputs(), first, ("critic_ws", "actor_ws", "grads", "dz_a", "loss_part", "sumsq_part", "step_dev")):
        assert _same(g.full, b), f"{name}: the second round leaves other bits in {nm}"
    job.assert_guards(f"{name} second round")
    return ratio


# ------------------------------------------------------------------------------------------------ fused backward + tail
@pytest.mark.parametrize("name", fc.NAMES)
def test_dpg_fused_case(dev, name):
    """pqlk_dpg_backward_fused + pqlk_mlp_backward_tail over NaN workspaces: mn, perm and tie0 equal the partition model,
    loss_part[:32] the float64 sums (loss_part[32:] untouched), columns [0, A) of dz_a, the actor's last-hidden dL/dZ and the whole
    gradient arena the float64 reference -- `==` for B a power of two, within the derived bound otherwise -- with dz_a's pad
    columns still poison and no NaN left in grads; a second round over the dirty workspaces leaves the same bits."""
    p, ref = fc.problem(name), fc.reference(name)
    job = FusedJob(dev, p)
    ratio = _run_and_check(job, ref, name)
    print(f"DPGFUSED {name} instance={fc.instance(p.c)} mn={ref['mn'].tolist()} exact={ref['exact']} err_over_bound={ratio:.3g}")


def test_short_workspaces_and_a_batch_past_the_limit_are_refused_with_nothing_touched(dev):
    """One float short of either workspace: PQLK_E_WORKSPACE; B = 131073 (buffers of that size, device-filled): PQLK_E_UNSUPPORTED;
    no output byte changes."""
    from pql_amd import _lib as L
    name = "p1-A5-c7-B127-mixed"
    job = FusedJob(dev, fc.problem(name))
    before = [g.full.clone() for g in job.outputs()]
    assert job.fused(ws_floats=job.ws_c_floats - 1) == fc.E_WORKSPACE
    assert job.fused(a_ws_floats=job.ws_a_floats - 1) == fc.E_WORKSPACE
    for g, b in zip(job.outputs(), before):
        assert _same(g.full, b), "a refused call wrote an output"
    job.assert_guards("refused")
    # ---- one batch past the limit, every buffer as large as that batch asks for
    B = fc.MAX_B + 1
    cdims, adims = fc.pair(1, 1)
    cd, ad = L.mlp_desc(cdims, 2), L.mlp_desc(adims, 1)
    assert int(L.lib.pqlk_dpg_fused_ok(C.byref(cd), C.byref(ad), B)) == 0 and int(L.lib.pqlk_dpg_fused_ok(C.byref(cd), C.byref(ad), B - 1)) == 1

    def buf(n, v):
        return torch.full((int(n),), v, device=dev)

    ws_c_n, ws_a_n = int(L.lib.pqlk_dpg_backward_ws_floats(C.byref(cd), B)), int(L.lib.pqlk_mlp_bwd_ws_floats(C.byref(ad), B, 16))
    c_arena, a_arena = buf(bc.net_stride(cdims) * 2, 0.0), buf(bc.net_stride(adims), 0.0)
    c_acts, a_acts = buf(bc.acts_floats(cdims, 2, B), 0.0), buf(bc.acts_floats(adims, 1, B), 0.0)
    qc, a_out = buf(2 * B, 0.0), buf(B * 32, 0.0)
    outs = [buf(B * 32, POISON), buf(64, NAN), buf(ws_c_n, NAN), buf(ws_a_n, NAN)]
    dz_a, loss, ws_c, ws_a = outs
    rcode = L.lib.pqlk_dpg_backward_fused(C.byref(cd), L.ptr(c_arena), None, 32, B, L.ptr(c_acts), L.ptr(qc), L.ptr(dz_a), 32, 8, L.ptr(a_out), 32,
                                          L.ptr(loss), L.ptr(ws_c), ws_c_n, C.byref(ad), L.ptr(a_arena), L.ptr(a_acts), L.ptr(ws_a), ws_a_n, 16,
                                          L.stream(dev))
    _returned(rcode, "pqlk_dpg_backward_fused at B = 131073")
    _sync_or_stop("pqlk_dpg_backward_fused at B = 131073")
    assert rcode == fc.E_UNSUPPORTED
    assert bool((dz_a == POISON).all()) and all(bool(torch.isnan(t).all()) for t in (loss, ws_c, ws_a)), "the refused call wrote an output"


def test_tail_with_the_squared_norm_partials(dev):
    """The tail as the learner calls it, with sumsq_part / step_dev, on B = 8 with gradients whose squares are exact: the same
    arena, the partials sum to the float64 sum g^2 and nothing is written behind them, step_dev goes up by 1."""
    name = fc.NORM_NAME
    p, ref = fc.problem(name), fc.reference(name)
    job = FusedJob(dev, p)
    assert job.fused() == 0 and job.tail(norm=True) == 0
    out = job.collect()
    ratio = fc.check_all(out, ref, name)
    got = job.sumsq.host()
    assert not np.isnan(got[: job.norm_parts]).any(), f"{name}: a squared-norm partial was not written"
    assert np.isnan(got[job.norm_parts:]).all(), f"{name}: sumsq_part written behind its {job.norm_parts} partials"
    total, want = float(got[: job.norm_parts].astype(F64).sum()), float((ref["grads"] ** 2).sum())
    assert total == want and want > 0, f"{name}: the squared-norm partials sum to {total}, sum g^2 is {want}"
    assert job.step_value() == STEP0 + 1, f"{name}: step_dev moved by {job.step_value() - STEP0}"
    job.assert_guards(name)
    # ---- without the two arguments: the same gradient bits, both buffers untouched
    grads1 = job.grads.full.clone()
    job.fresh_outputs()
    assert job.fused() == 0 and job.tail() == 0
    assert _same(job.grads.full, grads1) and bool(torch.isnan(job.sumsq.t).all()) and job.step_value() == STEP0 + 1
    job.assert_guards(f"{name} plain tail")
    print(f"DPGFUSED {name} tail+norm instance={fc.instance(p.c)} mn={ref['mn'].tolist()} exact={ref['exact']} err_over_bound={ratio:.3g}")


# ------------------------------------------------------------------------------------------------ pqlk_mlp_forward_qc
class QcJob:
    """The exact network of dpg_fused_cases.qc_problem on the device, packed."""

    def __init__(self, dev, B, twin):
        from pql_amd import _lib as L
        self.dev, self.B = dev, B
        self.case, self.W, self.bias, self.x, self.H, self.q = fc.qc_problem(B, twin)
        self.desc = L.mlp_desc(self.case.dims, 2)
        self.arena = Guarded(dev, (bc.net_stride(self.case.dims) * 2,), IN_ONE, fc.qc_arena(self.case, self.W, self.bias), off=SLACK)
        n = int(L.lib.pqlk_mlp_packed_floats(C.byref(self.desc)))
        assert n > 0
        self.packed = Guarded(dev, (n,), IN_ONE, body=NAN, off=SLACK)
        assert _returned(L.lib.pqlk_mlp_pack(C.byref(self.desc), L.ptr(self.arena.t), L.ptr(self.packed.t), L.stream(dev)), "pqlk_mlp_pack") == 0
        _sync_or_stop("pqlk_mlp_pack")
        assert self.packed.intact() and not bool(torch.isnan(self.packed.t).any())

    def inputs(self, form):
        """(x, ldx, x2, ldx2, x2_col0) of one input form; the columns of x past x2_col0 and of x2 past its share hold NaN."""
        O, K = fc.QC_O, self.case.dims[0]
        if form == "cat":
            return Guarded(self.dev, (self.B, 32), IN_ONE, self.x, off=SLACK), 32, None, 0, 0
        col0, ldx = {"split4": (4, 32), "splitO": (O, 32), "split64": (O, 64)}[form]
        x = np.full((self.B, ldx), np.nan, dtype=F32)
        x[:, :col0] = self.x[:, :col0]
        x2 = np.full((self.B, 32), np.nan, dtype=F32)
        x2[:, : K - col0] = self.x[:, col0: K]
        return Guarded(self.dev, x.shape, IN_ONE, x, off=SLACK), ldx, Guarded(self.dev, x2.shape, IN_ONE, x2, off=SLACK), 32, col0

    def forward(self, form):
        from pql_amd import _lib as L
        x, ldx, x2, ldx2, col0 = self.inputs(form)
        acts = Guarded(self.dev, (bc.acts_floats(self.case.dims, 2, self.B),), POISON, body=NAN)
        qc = Guarded(self.dev, (2, self.B), POISON, body=NAN)
        rcode = L.lib.pqlk_mlp_forward_qc(C.byref(self.desc), L.ptr(self.arena.t), L.ptr(self.packed.t), 1, L.ptr(x.t), ldx,
                                          L.ptr(x2.t) if x2 is not None else None, ldx2, col0, self.B, L.ptr(acts.t), L.ptr(qc.t), L.stream(self.dev))
        assert _returned(rcode, f"pqlk_mlp_forward_qc {form}") == 0
        _sync_or_stop(f"pqlk_mlp_forward_qc {form} on {self.case.name}")
        assert acts.intact() and qc.intact() and x.intact() and (x2 is None or x2.intact()) and self.arena.intact() and self.packed.intact()
        return acts, qc


FORMS = ("cat", "split4", "splitO", "split64")


@pytest.mark.parametrize("twin", [False, True])
@pytest.mark.parametrize("B", fc.QC_BATCHES)
def test_forward_qc_forms_leave_the_exact_forward(dev, B, twin):
    """The concatenated tile, the split forms with x2_col0 in {4, O} and the split form with ldx rounded to 64 and ldx2 = 32 (the
    learner's) all leave the float64 forward in the stash and in qc, bit for bit the same; the masked columns hold NaN."""
    job = QcJob(dev, B, twin)
    want, first = fc.qc_stash(job.case, job.H, job.q), None
    for form in FORMS:
        acts, qc = job.forward(form)
        stash, q = acts.host(), qc.host()
        bad = np.argwhere(~(stash == want))
        assert bad.size == 0, f"{form}: the stash differs from the exact network at {int(bad[0][0])}: {stash[bad[0][0]]} != {want[bad[0][0]]}"
        assert np.array_equal(q.astype(F64), job.q), f"{form}: qc differs from the float64 forward"
        if first is None:
            first = (stash, q)
        assert bc.bits_equal(stash, first[0]) and bc.bits_equal(q, first[1]), f"{form}: other bits than the concatenated tile leaves"


def test_forward_into_fused_backward_into_tail(dev):
    """The real chain on the exact network: pqlk_mlp_forward_qc (split input, ldx = 64) leaves the stash and qc that
    pqlk_dpg_backward_fused reads; the partition follows the network's integer Q (ties included) and every output equals the
    float64 reference."""
    p, (case, W, bias, x, H, q) = fc.chain_problem()
    ref = fc.reference_of(p)
    qjob = QcJob(dev, fc.CHAIN_B, False)
    acts, qc = qjob.forward("split64")
    assert np.array_equal(acts.host(), fc.qc_stash(case, H, q)) and np.array_equal(qc.host().astype(F64), q)
    job = FusedJob(dev, p, c_acts=acts, qc=qc)
    job.c_arena = qjob.arena                      # the network's own arena, biases included: the backward reads none
    job.inputs[0], job.before[0] = qjob.arena, qjob.arena.full.clone()
    ratio = _run_and_check(job, ref, p.c.name)
    assert ratio == 0.0
    print(f"DPGFUSED {p.c.name} instance={fc.instance(p.c)} mn={ref['mn'].tolist()} exact={ref['exact']} err_over_bound={ratio:.3g}")
