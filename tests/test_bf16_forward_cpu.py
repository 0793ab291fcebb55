"""The bf16 law on the CPU (tests/bf16_model.py): what the exact data guarantee, how many rows are ambiguous, what the rms
criterion of the realistic data is worth, and the argument checks of the pqlk_mlp_*_bf16 entry points (nothing is launched)."""
import ctypes as C

import pytest
import torch

import bf16_model as M


@pytest.mark.parametrize("name", M.FIRST_FIVE)
def test_exact_data_make_every_order_of_summation_agree(name):
    """Seed 1, B = 96: the three model variants (float64, plain fp32, reversed 16-column chunks in fp32) have identical hidden
    activations on every row that is not ambiguous -- every partial sum is exact in fp32 -- and their outputs differ by
    <= 3.5e-7 of max|out|.  Ambiguous rows of the 96 with this generator: 6, 6, 0, 3, 0 for the five shapes (the second hidden
    layer's pre-activations live on a grid of multiples of 2^-8, so the same few grid points recur across rows); the bound that
    the tests hold every case to is 10 % of its rows."""
    c = M.exact_case(name)
    x = c["x"][:96]
    draw = None if c["draw"] is None else c["draw"][:96]
    ref = M.forward(c["dims"], c["W"], c["b"], x, c["out_act"], draw, "f64")
    for mode in ("f32", "f32rev"):
        got = M.forward(c["dims"], c["W"], c["b"], x, c["out_act"], draw, mode)
        keep = ~ref["ambiguous"]
        for n in range(c["n_nets"]):
            for h64, h32 in zip(ref["hidden"][n], got["hidden"][n]):
                assert torch.equal(h64[keep], h32[keep]), (name, mode)
        diff = (got["out"].double() - ref["out"])[:, keep].abs().max()
        assert float(diff) <= 3.5e-7 * float(ref["out"].abs().max()), (name, mode, float(diff))
    assert int(ref["ambiguous"].sum()) <= 0.10 * 96


@pytest.mark.parametrize("B", M.BATCHES)
@pytest.mark.parametrize("name", sorted(M.EXACT_CASES))
def test_ambiguous_rows_are_few(name, B):
    amb = M.exact_case(name)["model"]["ambiguous"][:B]
    assert int(amb.sum()) <= 0.10 * B, (name, B, int(amb.sum()))


@pytest.mark.parametrize("scale", (1, 3))
@pytest.mark.parametrize("name", sorted(M.REAL_CASES))
def test_rms_criterion_holds_for_two_fp32_orders(name, scale):
    """Realistic data: rounding flips differ between any two implementations, so the criterion is rms(y - o64) <= 1/8 of the
    law's own distance from the unrounded network.  Both fp32-accumulating model variants must pass it."""
    c = M.real_case(name, scale)
    dist = M.rms(c["o64"] - c["fp32"])
    assert dist > 0
    for mode in ("f32", "f32rev"):
        y = M.forward(c["dims"], c["W"], c["b"], c["x"], c["out_act"], None, mode)["out"]
        assert M.rms(y.double() - c["o64"]) <= dist / 8, (name, scale, mode, M.rms(y.double() - c["o64"]), dist)


def test_bf16_rounding_is_nearest_even_with_ties():
    x = torch.tensor([1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -20, -(1.0 + 2.0 ** -8), float("inf")])
    assert torch.equal(M.bf(x), torch.tensor([1.0, 1.0 + 2.0 ** -6, 1.0 + 2.0 ** -7, -1.0, float("inf")]))
    assert torch.isnan(M.bf(torch.tensor([float("nan")]))).all()


def test_unpack_inverts_the_documented_fragment_order():
    dims, n_nets = [24, 64, 5], 2
    o, ref, flat = 0, [], []
    for n in range(n_nets):
        layers = []
        for l in range(2):
            K, N = dims[l], dims[l + 1]
            Kp, Np = (K + 15) // 16 * 16, (N + 31) // 32 * 32
            w = torch.zeros((Np, Kp), dtype=torch.int16)
            w[:N, :K] = torch.arange(1, N * K + 1, dtype=torch.int16).view(N, K) + 1000 * (2 * n + l)
            blk = torch.zeros((Np // 32, Kp // 16, 64, 8), dtype=torch.int16)
            for t in range(Np // 32):
                for ks in range(Kp // 16):
                    for lane in range(64):
                        blk[t, ks, lane] = w[32 * t + (lane & 31), 16 * ks + 8 * (lane >> 5): 16 * ks + 8 * (lane >> 5) + 8]
            flat.append(blk.reshape(-1)); layers.append(w[:N, :K]); o += Np * Kp
        ref.append(layers)
    got = M.unpack(torch.cat(flat), dims, n_nets)
    assert all(torch.equal(got[n][l], ref[n][l]) for n in range(2) for l in range(2))


# ------------------------------------------------------------------------------------------------ the C boundary, no launch
def _desc(dims, nets):
    from pql_amd import _lib as L
    return L.mlp_desc(dims, nets)


def test_eligibility_and_packed_size():
    from pql_amd import _lib as L
    ok = lambda dims, nets=1: int(L.lib.pqlk_mlp_bf16_ok(C.byref(_desc(dims, nets))))   # noqa: E731
    elems = lambda dims, nets=1: int(L.lib.pqlk_mlp_packed_bf16_elems(C.byref(_desc(dims, nets))))   # noqa: E731
    assert ok([24, 128, 128, 1], 2) and ok([88, 256, 128, 16]) and ok([24, 128, 64, 51], 2) and ok([104, 1024, 1024, 64], 2)
    assert not ok([24, 1])                 # one layer
    assert not ok([24, 100, 1])            # hidden width not a multiple of 32
    assert not ok([24, 1056, 1])           # hidden width past 1024
    assert not ok([24, 128, 65])           # output wider than 64
    assert not ok([4000, 128, 1])          # input too wide for two 32-row images in LDS
    assert elems([24, 128, 128, 1], 2) == 2 * (128 * 32 + 128 * 128 + 32 * 128)   # K padded to 16, N to 32
    assert elems([88, 256, 128, 51]) == 256 * 96 + 128 * 256 + 64 * 128
    assert elems([24, 100, 1]) == 0


def test_argument_errors_come_back_as_codes():
    """Bad arguments are positive PQLK_E_* codes before anything is launched; 0x1000 stands in for a device pointer."""
    from pql_amd import _lib as L
    P = C.c_void_p
    good, bad = _desc([24, 128, 128, 1], 2), _desc([24, 100, 1], 2)
    fwd = lambda d, prm=0x1000, pk=0x1000, x=0x1000, ldx=32, b=8, act=0, draw=None, out=0x1000, out2=None, ld2=0: \
        L.lib.pqlk_mlp_forward_bf16(C.byref(d), P(prm), P(pk), P(x), ldx, b, act, draw, 0.0, 0.0, P(out), out2, ld2, None)   # noqa: E731
    assert fwd(bad) == 5                                         # PQLK_E_UNSUPPORTED: not eligible
    assert fwd(good, prm=None) == 1 and fwd(good, pk=None) == 1 and fwd(good, x=None) == 1 and fwd(good, out=None) == 1
    assert fwd(good, act=2) == 1                                 # TANH_NOISE without a draw
    assert fwd(good, x=0x1004) == 4 and fwd(good, pk=0x1002) == 4 and fwd(good, out=0x1008) == 4 and fwd(good, prm=0x1004) == 4
    assert fwd(good, ldx=24) == 4 and fwd(good, ldx=0) == 4      # ldx below pqlk_ld(dims[0]) / not a multiple of 32
    assert fwd(good, b=0) == 2
    assert fwd(good, act=3) == 5
    assert fwd(good, out2=P(0x1000), ld2=32) == 2                # out2 needs n_nets == 1
    assert L.lib.pqlk_mlp_forward_bf16(None, P(0x1000), P(0x1000), P(0x1000), 32, 8, 0, None, 0.0, 0.0, P(0x1000), None, 0, None) == 1
    pack = lambda d, prm=0x1000, pk=0x1000: L.lib.pqlk_mlp_pack_bf16(C.byref(d), P(prm), P(pk), None)   # noqa: E731
    assert pack(bad) == 5 and pack(good, prm=None) == 1 and pack(good, pk=None) == 1 and pack(good, pk=0x1008) == 4
    assert L.lib.pqlk_mlp_bf16_ok(None) == 0 and L.lib.pqlk_mlp_packed_bf16_elems(None) == 0


# ------------------------------------------------------------------------------------------------ config and checkpoints
def test_target_dtype_defaults_to_float32_and_is_structural():
    from pql_amd.utils import checkpoint as CK
    from pql_amd.utils.cfg import load_cfg
    cfg = load_cfg(["task.name=Toy"])
    assert cfg.algo.target_dtype == "float32"
    cur = CK.structure(cfg, 8, 2)
    assert cur["algo.target_dtype"] == "float32"
    bf = CK.structure(load_cfg(["task.name=Toy", "algo.target_dtype=bfloat16"]), 8, 2)
    with pytest.raises(ValueError, match=r"algo\.target_dtype='bfloat16'.*algo\.target_dtype='float32'"):
        CK.check_structure(cur, bf)
    with pytest.raises(ValueError, match=r"algo\.target_dtype='float32'.*algo\.target_dtype='bfloat16'"):
        CK.check_structure(bf, cur)
    old = {k: v for k, v in cur.items() if k != "algo.target_dtype"}   # a checkpoint from before the key existed means float32
    CK.check_structure(old, cur)
    with pytest.raises(ValueError, match=r"algo\.target_dtype"):
        CK.check_structure(old, bf)
