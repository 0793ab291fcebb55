"""Every kernel choice of pqlk_mlp_backward, pqlk_mlp_backward_layers and pqlk_dpg_critic_backward on exactly summable data: the
fused head (k_skinny_bwd in all nine instantiations and three block heights), k_skinny_dw<4> / <16> + k_skinny_dx, the GEMM head,
k_gemm dW / dX in both tile sizes, both main loops and all three block orders, empty splits, an input tile wider than its logical
width, the zsum GEMM, k_dx_slice<16 / 4 / 1>, the slice GEMM, the compact-row chain.  Shapes, inputs, the float64 reference and
the checks themselves: tests/backward_cases.py (proved without a GPU in tests/test_backward_cases_cpu.py).

The activation stash is an input the test writes, every product is a dyadic rational and every sum fits 24 bits, so each output
element has ONE right value in any summation order: every comparison is an equality.  The workspace and the gradient arena start
as NaN, dx as poison; every written buffer has SLACK floats of poison behind it, which must come back intact; every read buffer
has 1.0 in front of and behind it, which would move a sum by a whole unit."""
import ctypes as C

import numpy as np
import pytest
import torch

import backward_cases as bc
import reduction_cases as rc
from backward_job import Guarded, _Job, _returned, _sync_or_stop
from support import dev  # noqa: F401

pytestmark = pytest.mark.gpu

T = rc.T
POISON, SLACK, IN_ONE = bc.POISON, bc.SLACK, bc.IN_ONE
NAN = float("nan")


@pytest.mark.parametrize("name", [c.name for c in bc.CASES])
def test_backward_case(dev, name):
    """One pqlk_mlp_backward per table row over a workspace of exactly pqlk_mlp_bwd_ws_floats NaNs: the whole gradient arena and
    the input gradient equal the float64 reference, pads are zero, nothing else is written; a second call over the dirty
    workspace leaves the same bits; a workspace one float short is refused before anything is launched."""
    case = bc.CASE_BY_NAME[name]
    job = _Job(dev, case)
    # ---- a workspace one float short of what the call insists on: PQLK_E_WORKSPACE, nothing touched
    need = bc.bwd_ws_required(case.dims, case.nets, case.B, case.splits, job.want_grads)
    assert need <= job.ws_floats
    assert job.call(ws_floats=need - 1, what="short workspace") == bc.E_WORKSPACE
    assert bool(torch.isnan(job.ws.t).all()) and (job.grads is None or bool(torch.isnan(job.grads.t).all()))
    assert job.dx is None or bool((job.dx.t == POISON).all())
    # ---- the call
    assert job.call() == 0
    print(f"BWDPATH {name} plan={bc.plan(case)}")
    grads1, dx1 = job.check(name)
    # ---- again, over the workspace the first call left
    job.fresh_outputs()
    assert job.call(what="second call") == 0
    grads2, dx2 = job.check(f"{name} second call")
    assert grads1 is None or bc.bits_equal(grads1, grads2), f"{name}: the second call leaves other gradient bits"
    assert dx1 is None or bc.bits_equal(dx1, dx2), f"{name}: the second call leaves other dx bits"


@pytest.mark.parametrize("name", bc.LAYERS_CASES)
def test_backward_layers_leave_the_single_call_bits(dev, name):
    """pqlk_mlp_backward_layers in the learner's buckets and in one bucket per layer, on rows with empty splits and on a
    non-fused skinny head: the union of the calls leaves the arena bits of one pqlk_mlp_backward call."""
    from pql_amd import _lib as L
    from pql_amd.utils.dp import layer_buckets
    case = bc.CASE_BY_NAME[name]
    job = _Job(dev, bc.Case(*case[:5], "g", *case[6:]))      # the bucket calls take no dx
    assert job.call() == 0
    single, _ = job.check(name)
    n_layers = len(case.dims) - 1
    for buckets in (layer_buckets(n_layers), [(l, l) for l in range(n_layers - 1, -1, -1)]):
        job.fresh_outputs()
        job.ws.t.fill_(NAN)
        for hi, lo in buckets:
            rcode = L.lib.pqlk_mlp_backward_layers(C.byref(job.desc), L.ptr(job.arena.t), L.ptr(job.x.t), case.ldx, case.B, L.ptr(job.acts.t),
                                                   L.ptr(job.dy.t), None, None, None, 0.0, None, L.ptr(job.grads.t), case.splits,
                                                   L.ptr(job.ws.t), job.ws_floats, hi, lo, L.stream(dev))
            assert _returned(rcode, f"pqlk_mlp_backward_layers on {name}") == 0
            _sync_or_stop(f"pqlk_mlp_backward_layers on {name}")
        got, _ = job.check(f"{name} buckets {buckets}")
        assert bc.bits_equal(got, single), (name, buckets)


def _dpg_call(dev, job, c, owner_t, what):
    from pql_amd import _lib as L
    ws_floats = int(L.lib.pqlk_dpg_backward_ws_floats(C.byref(job.desc), c.B))
    assert ws_floats == bc.dpg_ws_floats(c.dims, c.nets, c.B)
    ws = Guarded(dev, (ws_floats,), POISON, body=NAN)
    job.fresh_outputs()
    rcode = L.lib.pqlk_dpg_critic_backward(C.byref(job.desc), L.ptr(job.arena.t), L.ptr(job.x.t), job.case.ldx, c.B, L.ptr(job.acts.t),
                                           L.ptr(job.dy.t), L.ptr(job.dx.t), job.ld_dx, c.col0, c.cols, L.ptr(job.tanh.t), job.ld_tanh,
                                           C.c_void_p(owner_t.data_ptr()) if owner_t is not None else None, L.ptr(ws.t), ws_floats,
                                           L.stream(dev))
    assert _returned(rcode, what) == 0
    _sync_or_stop(what)
    assert ws.intact(), f"{what}: slack behind the workspace was written"
    job.assert_guards(what)
    return job.dx.host()


@pytest.mark.parametrize("name", [c.name for c in bc.DPG_CASES if c.compact])
def test_dpg_critic_backward_compact_rows(dev, name):
    """The compact-row chain (k_minnet_partition, k_minnet_head_dx, the compact dX GEMMs, k_dx_slice with the scatter) against the
    float64 reference of the dense product: mixed owners, every row a tie, every row net 0's, every row net 1's; the owners given
    as bytes (the stash's output block is then NaN: it must not be read) and derived from a Q block that says the same.  The
    slice columns equal the reference and every other column of the poisoned dx is zero."""
    c = bc.DPG_BY_NAME[name]
    case = bc.as_case(c)
    for pattern in bc.OWNERS:
        own, q = bc.owner_input(case, pattern)
        dy = bc.dpg_dy_input(case, own)
        ref = bc.reference(case, pattern)
        got = {}
        for form in ("bytes", "from_q"):
            what = f"{name} owners {pattern} {form}"
            job = _Job(dev, case, stash=bc.stash(case, q if form == "from_q" else None), dy=dy)
            owner_t = None
            if form == "bytes":      # ties behind the B owner bytes: an over-read would add rows to both runs
                owner_t = torch.full((c.B + SLACK,), 3, dtype=torch.uint8, device=dev)
                owner_t[: c.B] = T(own).to(dev)
            got[form] = _dpg_call(dev, job, c, owner_t, what)
            bc.check_dx_slice(got[form], job.dx_before, case, ref, what, rest="zero")
        assert bc.bits_equal(got["bytes"], got["from_q"]), f"{name} owners {pattern}"


@pytest.mark.parametrize("name", [c.name for c in bc.DPG_CASES if not c.compact])
def test_dpg_critic_backward_dense_chain_writes_the_slice_alone(dev, name):
    """A critic the compact chain declines (51 outputs) takes pqlk_mlp_backward's dense chain (include/pqlk.h): the slice columns
    equal the reference and every other column of dx keeps what it held -- the caller keeps them zero itself."""
    c = bc.DPG_BY_NAME[name]
    case = bc.as_case(c)
    assert not bc.minnet_ok(c.dims, c.nets, c.cols)
    for form in ("bytes", "null"):
        job = _Job(dev, case)
        owner_t = torch.full((c.B + SLACK,), 3, dtype=torch.uint8, device=dev) if form == "bytes" else None
        dx = _dpg_call(dev, job, c, owner_t, f"{name} {form}")
        bc.check_dx_slice(dx, job.dx_before, case, what=f"{name} {form}", rest="untouched")
