"""The table of tests/forward_head_cases.py means what tests/test_forward_heads_gpu.py assumes: every case reaches the head kernel
it names, every cell the suite had left dark is among the forwards the GPU test asserts, the noise makes both clamps bind, and
the checks fail on the wrong epilogues they are there to catch.  No GPU needed."""
import ctypes as C
import os

import numpy as np
import pytest

import forward_head_cases as fc

F32 = np.float32


# --------------------------------------------------------------------------- the mirror against the library and the table
def test_mirror_of_fusable_agrees_with_the_library():
    """pqlk_mlp_packed_floats is the one dispatch predicate the library exposes; it loads on a host without a GPU."""
    from pql_amd import _lib as L
    extra = [[8, 1024, 3], [8, 1056, 3], [8, 636, 640, 3], [40000, 32, 3], [12, 48, 6], [12, 6], [12, 64, 96, 128, 6]]
    for dims in [c.dims for c in fc.CASES] + extra:
        for nets in (1, 2):
            d = L.mlp_desc(dims, nets)
            assert (int(L.lib.pqlk_mlp_packed_floats(C.byref(d))) > 0) == bool(fc.fusable(dims)), dims
    assert not fc.fusable([40000, 32, 3]) and fc.fusable([8, 1024, 3]), "the LDS rule and the width rule are both exercised"
    for c in (1, 31, 32, 33, 100):
        assert int(L.lib.pqlk_ld(c)) == fc.ld(c)


@pytest.mark.parametrize("name", [c.name for c in fc.CASES])
def test_case_reaches_the_path_it_names(name):
    c = fc.CASE_BY_NAME[name]
    assert fc.head_path(c.dims, c.nets, c.packed, c.B) == c.path
    assert not c.packed or fc.fusable(c.dims), "packed weights exist only for a fusable stack"


def test_every_path_is_reached_with_one_and_two_nets_and_ragged_tiles():
    reached = {c.path for c in fc.CASES}
    assert reached == set(fc.PATHS), set(fc.PATHS) ^ reached
    for kernel in ("fused", "skinny", "narrow", "gemm"):
        mine = [c for c in fc.CASES if c.path[0] == kernel]
        assert {c.nets for c in mine} == {1, 2}, kernel
        for B in (1, 33, 65):       # 1: a lone row; 33: a 32-row tile plus one row; 65: a 64-row tile plus one row
            assert any(c.B == B and c.nets == 1 for c in mine), (kernel, B)
    for path in fc.PATHS:           # every kernel instantiation sees a ragged last row tile and a second destination
        mine = [c for c in fc.CASES if c.path == path]
        assert any(c.B % 128 for c in mine) and any(c.nets == 1 for c in mine), path


def test_threshold_batches_are_the_smallest():
    assert fc.B_FUSED_R2_2NETS == 4097 and fc.B_FUSED_R2_1NET == 8193 and fc.B_GEMM128_1NET == 255 * 128 + 1
    assert fc.head_path([12, 64, 6], 2, True, fc.B_FUSED_R2_2NETS - 1) == ("fused", 1, False)
    assert fc.head_path([12, 64, 6], 1, True, fc.B_FUSED_R2_1NET - 1) == ("fused", 1, False)
    assert fc.head_path([32, 100], 1, False, fc.B_GEMM128_1NET - 1) == ("gemm", 64)
    assert fc.head_path([32, 100], 2, False, fc.B_GEMM128_2NETS) == ("gemm", 128) and fc.B_GEMM128_2NETS % 128 == 3


def test_every_dark_cell_is_among_the_asserted_forwards():
    cells = fc.cells()
    noisy, tanh = fc.ACT_TANH_NOISE, fc.ACT_TANH

    def some(pred):
        return any(pred(c, act, pl) for c, act, pl in cells)

    for kernel in ("skinny", "narrow", "gemm"):          # TANH_NOISE, and out2 under every activation and both alignments
        assert some(lambda c, a, p: c.path[0] == kernel and a == noisy and p is None), kernel
        for act in fc.ACTS:
            for place in ("aligned", "misaligned"):
                assert some(lambda c, a, p: c.path[0] == kernel and a == act and p == place), (kernel, act, place)
    for path in fc.PATHS:                                # ... on every instantiation
        for place in (None, "aligned", "misaligned"):
            assert some(lambda c, a, p: c.path == path and a == noisy and p == place), (path, place)
    # k_fwd_narrow: both epilogues, each with and without out2; NT = 2 with an activation; depth 4 with K / 8 = 12; N <= 4
    for vec in (True, False):
        for with_out2 in (True, False):
            for act in fc.ACTS:
                assert some(lambda c, a, p: c.path[0] == "narrow" and a == act and (p is not None) == with_out2
                            and fc.narrow_vec(c.dims[-1], p) == vec), (vec, with_out2, act)
    for D in (4, 8):
        for act in (tanh, noisy):
            assert some(lambda c, a, p: c.path == ("narrow", 2, D) and a == act), (D, act)
    for NT in (1, 2):
        assert some(lambda c, a, p: c.path == ("narrow", NT, 4) and (fc.ld(c.dims[-2]) // 8) % 8 == 4 and a == noisy and p is not None), NT
    for n_out in (2, 4):
        assert some(lambda c, a, p: c.path[0] == "narrow" and c.dims[-1] == n_out and a == noisy and p == "misaligned"), n_out
    assert {c.dims[-1] for c in fc.CASES if c.path[:2] == ("narrow", 1)} >= {5, 20, 21, 32}
    assert {(c.dims[-1], c.dims[-2]) for c in fc.CASES if c.path[:2] == ("narrow", 2)} >= {(n, k) for n in (33, 51, 64) for k in (64, 96)}
    assert {fc.ld(c.dims[-2]) for c in fc.CASES if c.path[:2] == ("narrow", 1)} >= {32, 64, 96, 128}
    # k_gemm: the 16-byte `full` epilogue under TANH, the per-element one on the same shape with out2, an edge column tile
    assert some(lambda c, a, p: c.path == ("gemm", 64) and a == tanh and fc.gemm_full_tiles(c.B, c.dims[-1], 64, a, p) == 2)
    assert some(lambda c, a, p: c.path == ("gemm", 64) and a == tanh and p == "aligned" and c.B >= 64 and c.dims[-1] == 128)
    assert some(lambda c, a, p: c.path == ("gemm", 64) and c.dims[-1] % 64 != 0 and a == noisy and p == "misaligned")
    for c in fc.CASES:
        if c.path == ("gemm", 64):
            assert fc.hidden_path(c.dims, c.packed) == "gemm", "k_gemm's ELU epilogue runs under the head"
    # one layer with an activation, on three kernels
    assert {c.path[0] for c, a, p in cells if len(c.dims) == 2 and a == noisy and p is not None} == {"skinny", "narrow", "gemm"}
    # fused head: exactly 32 outputs; 6, 21 and 3 outputs; the wide and the 64-row kernels with out2; the learners' alias form
    assert some(lambda c, a, p: c.path[0] == "fused" and c.dims[-1] == 32 and a == noisy and p == "misaligned")
    for path in (("fused", 1, True), ("fused", 2, False)):
        for place in ("aligned", "misaligned", "alias"):
            assert some(lambda c, a, p: c.path == path and p == place and a == noisy), (path, place)
    for O in (12, 11):
        assert some(lambda c, a, p: c.path[0] == "fused" and c.dims[0] == O and p == "alias" and a == noisy), O
    assert some(lambda c, a, p: c.path[0] == "fused" and c.nets == 2 and ((c.B + 31) // 32) % 4 == 0), "the XCD-aware block map"


def test_out2_matrices_are_aligned_and_misaligned_as_named():
    for c in fc.CASES:
        for place in fc.placements(c)[1:]:
            rows, stride, col0 = fc.out2_geometry(c, place)
            assert rows == c.B and col0 + c.dims[-1] <= stride, (c.name, place)
            if place == "aligned":
                assert stride % 4 == 0 and col0 % 4 == 0
            elif place == "misaligned":
                assert stride % 2 == 1 and col0 % 4 != 0
            else:
                assert stride % 32 == 0 and stride >= fc.ld(c.dims[0]) and col0 == c.dims[0]


# --------------------------------------------------------------------------- the inputs
@pytest.mark.parametrize("name", [c.name for c in fc.CASES])
def test_noise_design_makes_both_clamps_bind(name):
    inner, outer = fc.noise_shares(fc.CASE_BY_NAME[name])
    assert 0.10 <= inner <= 0.90 and outer >= 0.02, (inner, outer)


def test_tanh_bar_is_twice_the_measurement_and_under_the_cap():
    assert fc.TANH_ULPS == int(np.ceil(2 * fc.TANH_MEASURED_ULPS))
    assert fc.TANH_ULPS * 2.0 ** -24 <= fc.TANH_ABS_CAP      # results lie in [-1, 1]: an ulp is at most 2^-24


# --------------------------------------------------------------------------- the checks pass on a right head and fail on wrong ones
_MODEL_CASES = ["12x64x6-n1-packed-B33", "12x96x21-n2-layers-B33", "16x48x70-n1-layers-B65", "40x3-n1-layers-B33"]


def _model_inputs(case):
    h = fc.x_input(case)
    if len(case.dims) > 2:      # a stand-in for the stashed last hidden block: float32 of the float64 hidden stack
        z = h.astype(np.float64)
        for w, b in fc.weights(case)[0][:-1]:
            z = fc.elu64(z @ w.astype(np.float64).T + b.astype(np.float64))
        h = z.astype(F32)
    W, b = fc.weights(case)[0][-1]
    return h, W, b, fc.draw_input(case)


@pytest.mark.parametrize("name", _MODEL_CASES)
def test_checks_pass_on_a_float32_model_and_catch_wrong_epilogues(name):
    case = fc.CASE_BY_NAME[name]
    N, k_pad = case.dims[-1], fc.ld(case.dims[-2])
    h, W, b, draw = _model_inputs(case)
    z = fc.model_head(h, W, b, fc.ACT_NONE)
    t = fc.model_head(h, W, b, fc.ACT_TANH)
    s = fc.model_head(h, W, b, fc.ACT_TANH_NOISE, draw)
    assert fc.check_none(z, h, W, b, N, k_pad) < 0.5          # numpy's own fp32 order sits well inside the doubled bound
    assert fc.check_tanh(t, z, N, fc.TANH_ULPS) <= 0.5
    fc.check_noise(s, t, draw, N)
    # the accumulation: one product dropped, the bias left out, a poisoned pad column
    z_bad = fc.model_head(h[:, :-1], W[:, :-1], b, fc.ACT_NONE)
    with pytest.raises(AssertionError, match="of the bound"):
        fc.check_none(z_bad, h, W, b, N, k_pad)
    with pytest.raises(AssertionError, match="of the bound"):
        fc.check_none(fc.model_head(h, W, 0 * b, fc.ACT_NONE), h, W, b, N, k_pad)
    if fc.ld(N) > N:
        z_pad = z.copy(); z_pad[0, N] = 1e-30
        with pytest.raises(AssertionError, match="pad"):
            fc.check_none(z_pad, h, W, b, N, k_pad)
    # tanh a few ulps off
    t_bad = t.copy(); t_bad[:, 0] = np.nextafter(t_bad[:, 0], F32(2))
    for _ in range(fc.TANH_ULPS):
        t_bad[:, 0] = np.nextafter(t_bad[:, 0], F32(2))
    with pytest.raises(AssertionError, match="ulps off"):
        fc.check_tanh(t_bad, z, N, fc.TANH_ULPS)
    # the clamps in the wrong order; the draw read with the output's row stride instead of N
    with pytest.raises(AssertionError, match="smooth32"):
        fc.check_noise(fc.model_head(h, W, b, fc.ACT_TANH_NOISE, draw, swap_clamps=True), t, draw, N)
    if case.B > 1:
        with pytest.raises(AssertionError, match="smooth32"):
            fc.check_noise(fc.model_head(h, W, b, fc.ACT_TANH_NOISE, draw, draw_stride=fc.ld(N)), t, draw, N)
    # noise_std and noise_clip exchanged
    with pytest.raises(AssertionError, match="smooth32"):
        swapped = t.copy(); swapped[:, :N] = fc.smooth32(t[:, :N], draw, fc.NOISE_CLIP, fc.NOISE_STD)
        fc.check_noise(swapped, t, draw, N)


@pytest.mark.parametrize("place", ["aligned", "misaligned", "alias"])
def test_out2_check_catches_a_shifted_or_spilled_copy(place):
    case = fc.CASE_BY_NAME["12x64x6-n1-packed-B33"]
    N = case.dims[-1]
    h, W, b, draw = _model_inputs(case)
    out = fc.model_head(h, W, b, fc.ACT_TANH_NOISE, draw)
    rows, stride, col0 = fc.out2_geometry(case, place)
    before = np.full((rows, stride), fc.POISON, dtype=F32)
    good = before.copy(); good[:, col0:col0 + N] = out[:, :N]
    fc.check_out2(good, col0, out, N, before)
    shifted = before.copy(); shifted[:, col0 + 1:col0 + 1 + N] = out[:, :N]
    with pytest.raises(AssertionError):
        fc.check_out2(shifted, col0, out, N, before)
    spilled = good.copy(); spilled[:, col0 + N] = 0.0          # a pad column written past the N outputs
    with pytest.raises(AssertionError, match="outside out2"):
        fc.check_out2(spilled, col0, out, N, before)
    if stride == fc.ld(N):
        return
    strided = before.copy().reshape(-1)                        # rows laid down with the output block's stride
    for r in range(rows):
        if r * fc.ld(N) + col0 + N <= strided.size:
            strided[r * fc.ld(N) + col0: r * fc.ld(N) + col0 + N] = out[r, :N]
    with pytest.raises(AssertionError):
        fc.check_out2(strided.reshape(rows, stride), col0, out, N, before)


# --------------------------------------------------------------------------- every case is asserted
def test_gpu_module_skips_nothing():
    src = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "test_forward_heads_gpu.py")).read()
    for word in ("skip", "xfail", "importorskip"):
        assert word not in src, word
