"""The output-layer epilogue of pqlk_mlp_forward on every head kernel: fused head (k_mlp_fwd_fused<1, 2>, <1, 4>, <2, 2>),
k_skinny_fwd, k_fwd_narrow<NT, EPI, D> on both of its epilogues, k_gemm<FWD, 64, 64> and <FWD, 128, 128>, each with NONE / TANH /
TANH_NOISE, with and without a second destination, on ragged row tiles.  Shapes, inputs, references and the checks themselves:
tests/forward_head_cases.py (proved without a GPU in tests/test_forward_head_cases_cpu.py).

Every buffer a kernel writes has SLACK floats of poison behind it, which must come back intact; x and the draw have slack that
would move the result.  The head is isolated from the layers below it: its float64 reference starts from the last hidden block
the kernel itself stashed."""
import ctypes as C

import numpy as np
import pytest
import torch

import forward_head_cases as fc
import reduction_cases as rc
from guarded import Guarded
from support import dev  # noqa: F401

pytestmark = pytest.mark.gpu

T = rc.T
POISON, SLACK = fc.POISON, fc.SLACK


class _Net:
    """One case on the device: arena, packed weights, input tile, draw."""

    def __init__(self, dev, case):
        from pql_amd.models.mlp import ArenaLayout, PackedWeights
        self.dev, self.case = dev, case
        self.lay = lay = ArenaLayout(case.dims, case.nets)
        self.host_w = fc.weights(case)
        self.arena = torch.zeros(lay.total, device=dev)
        for n in range(case.nets):
            for l in range(lay.n_layers):
                w, b = self.host_w[n][l]
                lay.weight(self.arena, n, l).copy_(T(w)); lay.bias(self.arena, n, l).copy_(T(b))
        self.host_x = fc.x_input(case)
        self.x = Guarded(dev, (case.B, lay.ld_in), rc.IN_BIG)
        self.x.t.zero_(); self.x.t[:, : case.dims[0]] = T(self.host_x).to(dev)
        self.host_draw = fc.draw_input(case)
        self.draw = Guarded(dev, self.host_draw.shape, rc.IN_BIG, self.host_draw)
        self.pk = PackedWeights(lay, dev)
        assert (self.pk.tensor is not None) == bool(fc.fusable(case.dims))
        self.pk.refresh(self.arena)

    def forward(self, act, packed, stash_all=1, x=None, out2_ptr=None, ld_out2=0):
        """One pqlk_mlp_forward into a fresh poisoned stash; returns (stash on the device, output block (nets, B, ld) on the host)."""
        from pql_amd import _lib as L
        lay, B = self.lay, self.case.B
        x = self.x if x is None else x
        acts = Guarded(self.dev, (lay.acts_floats(B),), POISON)
        pk = self.pk.tensor if packed else None
        rcode = L.lib.pqlk_mlp_forward(C.byref(lay.desc), L.ptr(self.arena), L.ptr(pk), stash_all, L.ptr(x.t), x.t.stride(0), B, act,
                                       L.ptr(self.draw.t) if act == fc.ACT_TANH_NOISE else None, fc.NOISE_STD, fc.NOISE_CLIP, L.ptr(acts.t),
                                       out2_ptr, ld_out2, L.stream(self.dev))
        if rcode < 0:      # a HIP error: nothing more may be started on this device
            pytest.exit(f"pqlk_mlp_forward: HIP error {rcode} on {self.case.name}", returncode=3)
        L.check(rcode)
        off, ldo = lay.act_offset(B, 0, lay.n_layers - 1)
        out = acts.t[off: off + self.case.nets * B * ldo].view(self.case.nets, B, ldo).cpu().numpy()
        assert acts.intact() and x.intact() and self.draw.intact(), "slack behind a buffer was written"
        return acts, out

    def hidden(self, acts, net):
        """The last hidden block (B, ld) of a stash, on the host."""
        lay, B = self.lay, self.case.B
        off, ldh = lay.act_offset(B, net, lay.n_layers - 2)
        return acts.t[off: off + B * ldh].view(B, ldh).cpu().numpy()


@pytest.mark.parametrize("name", [c.name for c in fc.CASES])
def test_forward_head(dev, name):
    case = fc.CASE_BY_NAME[name]
    dims, nets, B, N = case.dims, case.nets, case.B, case.dims[-1]
    L_, Kin, k_pad = len(dims) - 1, case.dims[-2], fc.ld(case.dims[-2])
    net = _Net(dev, case)

    # ---- 1-3: the three activations, no second destination
    base, worst_bound, worst_ulps = {}, 0.0, 0.0
    acts1, base[fc.ACT_NONE] = net.forward(fc.ACT_NONE, case.packed)
    for n in range(nets):
        if L_ >= 2:
            hblock = net.hidden(acts1, n)
            assert np.all(hblock[:, Kin:] == 0), "pad columns of the last hidden block"
            h = hblock[:, :Kin]
        else:
            h = net.host_x
        W, b = net.host_w[n][-1]
        worst_bound = max(worst_bound, fc.check_none(base[fc.ACT_NONE][n], h, W, b, N, k_pad, f"{name} net {n} NONE"))
    _, base[fc.ACT_TANH] = net.forward(fc.ACT_TANH, case.packed)
    ulps = [float(fc.ulps_off(base[fc.ACT_TANH][n][:, :N], np.tanh(base[fc.ACT_NONE][n][:, :N].astype(np.float64))).max()) for n in range(nets)]
    print(f"FWDHEAD {name} path={case.path} err/bound={worst_bound:.3f} tanh_ulps={max(ulps):.3f}")
    for n in range(nets):
        fc.check_tanh(base[fc.ACT_TANH][n], base[fc.ACT_NONE][n], N, fc.TANH_ULPS, f"{name} net {n} TANH")
    _, base[fc.ACT_TANH_NOISE] = net.forward(fc.ACT_TANH_NOISE, case.packed)
    for n in range(nets):
        fc.check_noise(base[fc.ACT_TANH_NOISE][n], base[fc.ACT_TANH][n], net.host_draw, N, f"{name} net {n} TANH_NOISE")

    # ---- 4: second destinations
    for place in fc.placements(case)[1:]:
        rows, stride, col0 = fc.out2_geometry(case, place)
        for act in fc.ACTS:
            what = f"{name} act {act} out2 {place}"
            if place == "alias":      # the learners' form: out2 = x[:, O:], columns >= O of x hold poison and must be ignored
                mat = Guarded(dev, (rows, stride), POISON)
                mat.t[:, : dims[0]] = T(net.host_x).to(dev)
                x = mat
            else:
                mat, x = Guarded(dev, (rows, stride), POISON), None
            before = mat.t.cpu().numpy()
            ptr = C.c_void_p(mat.t.data_ptr() + 4 * col0)
            assert (ptr.value % 16 == 0 and stride % 4 == 0) == (place == "aligned" or (place == "alias" and dims[0] % 4 == 0)), what
            _, out = net.forward(act, case.packed, x=x, out2_ptr=ptr, ld_out2=stride)
            assert mat.intact(), what
            assert fc.bits_equal(out, base[act]), f"{what}: the output block differs from the run without out2"
            fc.check_out2(mat.t.cpu().numpy(), col0, out[0], N, before, what)

    # ---- 5: stash
    if fc.fusable(dims):     # the other hidden path leaves the same last hidden block (include/pqlk.h: identical hidden activations)
        acts_o, _ = net.forward(fc.ACT_NONE, not case.packed)
        for n in range(nets):
            assert fc.bits_equal(net.hidden(acts1, n), net.hidden(acts_o, n)), f"{name} net {n}: last hidden block, fused vs per-layer"
    if case.path[0] == "fused":     # stash_all = 0: the same output block, the hidden blocks untouched
        off, _ = net.lay.act_offset(B, 0, L_ - 1)
        for act in fc.ACTS:
            acts0, out0 = net.forward(act, True, stash_all=0)
            assert fc.bits_equal(out0, base[act]), f"{name} act {act}: stash_all = 0 changes the output block"
            assert bool((acts0.t[:off] == POISON).all()), f"{name} act {act}: stash_all = 0 wrote a hidden block"
