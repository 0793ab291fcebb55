"""The hidden layers of pqlk_mlp_forward on every path: k_mlp_fwd_fused<1, 2>, <2, 2>, <1, 4> through every ring-group shape,
tiles-per-wave choice, stash route and block map, and k_gemm<FWD, EPI_ELU> on both tiles and all three tile orders -- each hidden
block of the stash against a float64 reference.  Shapes, inputs, references and the checks themselves: tests/forward_hidden_cases.py
(proved without a GPU in tests/test_forward_hidden_cases_cpu.py).

The stash starts as poison, with poison in front of it and behind it: what the call must not write comes back bit for bit.  A
second call over the dirty stash must leave the same bits; on the fused path its input tile carries NaN, not 1e30, in the columns
the kernel is to ignore.  A HIP error ends the session: nothing more may be started on a device that has faulted."""
import ctypes as C

import numpy as np
import pytest

import forward_hidden_cases as hc
import reduction_cases as rc
from backward_job import _returned, _sync_or_stop
from guarded import Guarded, T
from support import dev  # noqa: F401

pytestmark = pytest.mark.gpu

POISON, SLACK = hc.POISON, hc.SLACK


class _Net:
    """One case and design on the device: arena, packed weights, the input tile in its three forms."""

    def __init__(self, dev, case, design):
        from pql_amd import _lib as L
        from pql_amd.models.mlp import ArenaLayout, PackedWeights
        self.dev, self.case = dev, case
        self.lay = lay = ArenaLayout(case.dims, case.nets)
        host = hc.arena(case, design)
        assert host.size == lay.total
        self.arena = T(host).to(dev)
        self.x = Guarded(dev, (case.B, case.ldx), rc.IN_BIG, hc.x_tile(case, design), off=SLACK)
        self.x_nan = Guarded(dev, (case.B, case.ldx), rc.IN_BIG, hc.x_tile(case, design, np.nan), off=SLACK)
        self.x_clean = Guarded(dev, (case.B, case.ldx), rc.IN_BIG, hc.x_tile(case._replace(packed=False), design), off=SLACK)
        self.pk = PackedWeights(lay, dev)
        assert (self.pk.tensor is not None) == bool(hc.fusable(case.dims))
        self.pk.refresh(self.arena)
        self.n_acts = lay.acts_floats(case.B)
        self.L = L

    def stash(self):
        return Guarded(self.dev, (self.n_acts,), POISON, off=SLACK)

    def forward(self, acts, x, packed, stash_all, what):
        """One pqlk_mlp_forward into `acts`; returns the flat stash on the host."""
        L, c = self.L, self.case
        rcode = L.lib.pqlk_mlp_forward(C.byref(self.lay.desc), L.ptr(self.arena), L.ptr(self.pk.tensor) if packed else None, stash_all,
                                       L.ptr(x.t), c.ldx, c.B, L.ACT_NONE, None, 0.0, 0.0, L.ptr(acts.t), None, 0, L.stream(self.dev))
        _returned(rcode, f"pqlk_mlp_forward on {what}")
        _sync_or_stop(f"pqlk_mlp_forward on {what}")
        L.check(rcode)
        assert acts.intact(), f"{what}: the slack in front of or behind the stash was written"
        assert x.intact(), f"{what}: the slack around the input tile was written"
        return acts.host()


@pytest.mark.parametrize("design", hc.DESIGNS)
@pytest.mark.parametrize("name", [c.name for c in hc.CASES])
def test_forward_hidden(dev, name, design):
    case = hc.CASE_BY_NAME[name]
    fused, what = hc.on_fused_path(case), f"{name} {design}"
    net = _Net(dev, case, design)

    acts = net.stash()
    first = net.forward(acts, net.x, case.packed, case.stash_all, what)
    second = net.forward(acts, net.x_nan if fused else net.x, case.packed, case.stash_all, what + " (second call)")
    assert hc.bits_equal(first, second), f"{what}: a second call over the dirty stash" + (", NaN in the ignored columns," if fused else "") + " leaves other bits"

    if case.stash_all:
        full, worst = first, hc.check_stash(case, design, first, what=what)
    else:       # the stash_all = 1 run supplies the previous blocks and the bits of what stash_all = 0 still writes
        full = net.forward(net.stash(), net.x, True, 1, what + " (stash_all = 1)")
        worst = hc.check_stash(case._replace(stash_all=1), design, full, what=what + " (stash_all = 1)")
        hc.check_stash(case, design, first, full, what=what)
    print(f"FWDHIDDEN {name} {design} path={'fused' if fused else 'gemm'} instance={hc.path_name(case)} share={worst:.3f}")
    assert design == "exact" or worst <= 1.0

    if hc.fusable(case.dims):     # include/pqlk.h: hidden activations are identical on the fused and the per-layer path
        other = net.forward(net.stash(), net.x_clean, not fused, 1, what + " (other path)")
        hc.check_same_hidden(case, full, other, what=f"{what}: fused vs per-layer")
