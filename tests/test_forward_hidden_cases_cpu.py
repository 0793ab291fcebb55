"""The table of tests/forward_hidden_cases.py means what tests/test_forward_hidden_gpu.py assumes: the mirror agrees with the
library where the library answers without a GPU, the union of the cases reaches every branch listed in COVERAGE, the exact design
is feasible on every case, and the checks pass on a plain float32 forward and fail on every wrong one.  No GPU needed."""
import ctypes as C
import os

import numpy as np
import pytest

import backward_cases as bc
import forward_hidden_cases as hc

F32 = np.float32
NAMES = [c.name for c in hc.CASES]


# --------------------------------------------------------------------------- the mirror against the library
def test_mirror_agrees_with_the_library():
    from pql_amd import _lib as L
    for c in hc.CASES:
        d = L.mlp_desc(c.dims, c.nets)
        assert (int(L.lib.pqlk_mlp_packed_floats(C.byref(d))) > 0) == bool(hc.fusable(c.dims)), c.name
        assert int(L.lib.pqlk_mlp_acts_floats(C.byref(d), c.B)) == bc.acts_floats(c.dims, c.nets, c.B), c.name
        for n in range(c.nets):
            for l in range(len(c.dims) - 1):
                off, ldh = C.c_int64(), C.c_int64()
                L.check(L.lib.pqlk_mlp_act_offset(C.byref(d), c.B, n, l, C.byref(off), C.byref(ldh)))
                assert (off.value, ldh.value) == bc.act_offset(c.dims, c.nets, c.B, n, l), (c.name, n, l)
        assert c.ldx % 32 == 0 and c.ldx >= hc.ld(c.dims[0])
        assert not c.packed or hc.fusable(c.dims), "packed weights exist only for a fusable stack"
        assert c.stash_all == 1 or hc.on_fused_path(c), "stash_all = 0 is a statement about the fused path"


def test_forward_mode_of_the_gemm_plan():
    """The forward has dX's grid and groups (gemm.hip:753-765) and never the LDS-DMA loop, whatever the shape."""
    for M, N in ((128, 128), (500, 48), (16385, 128)):
        for tile in (64, 128):
            fwd = bc.gemm_plan("FWD", "ELU", tile, M, N, 128, 128, 128, hc.ld(N), 2)
            dx = bc.gemm_plan("dX", "DELU", tile, M, N, 128, 128, 128, hc.ld(N), 2)
            assert fwd[0] == dx[0] and fwd[2] == dx[2] and fwd[1] == "staged"
    assert bc.gemm_plan("FWD", "NONE", 64, 128, 128, 128, 128, 128, 128, 1)[1] == "staged"
    assert bc.gemm_plan("dX", "NONE", 64, 128, 128, 128, 128, 128, 128, 1)[1] == "dma"


# --------------------------------------------------------------------------- coverage
def test_the_table_reaches_every_listed_branch():
    union = set()
    for c in hc.CASES:
        union |= hc.reached(c)
    missing = [item for item in hc.COVERAGE if item not in union]
    assert not missing, f"no case reaches {missing}"
    assert not [item for item in hc.UNREACHABLE if item in union], "an item listed as unreachable is reached: move it to COVERAGE"
    assert len(set(hc.COVERAGE)) == len(hc.COVERAGE)


def test_coverage_lists_what_the_issue_names():
    cov = set(hc.COVERAGE)
    assert {i[1:] for i in cov if i[0] == "kernel"} == {(1, 2), (2, 2), (1, 4)}
    for D in (4, 2):                                               # G = 0 / 1 / 2 / >= 3, remainder or not; G = 0 has a remainder
        assert {i[2:] for i in cov if i[:2] == ("ring", D)} == {(g, r) for g in range(4) for r in (False, True)} - {(0, False)}
    assert {i[1] for i in cov if i[0] == "defer" and isinstance(i[1], int)} == {8, 24, 72, 136, 256}
    assert {i[1] for i in cov if i[0] == "mask"} == {1, 2, 3}
    assert {i[1] for i in cov if i[0] == "width"} == {32, 96, 256, 288, 512, 544, 1024}
    gemm = {i[1:] for i in cov if i[0] == "gemm" and len(i) == 4} | {i[1:] for i in hc.UNREACHABLE}
    assert gemm == {(t, x, e) for t in (64, 128) for x in (0, "groups", "runs") for e in (False, True)}


def test_unreachable_items_are_unreachable():
    """k_gemm<FWD, 128, 128> in dispatch order: the 128 tile needs 256 tiles of 128 x 128, dispatch order fewer than 64 tiles."""
    for B in (1, 127 * 128, 127 * 128 + 1, 1 << 16):
        for N in (128, 256, 1024):
            for nets in (1, 2):
                if hc.gemm_tile(B, N, nets) == 128:
                    assert bc.gemm_plan("FWD", "ELU", 128, B, N, 128, 128, 128, N, nets)[2] != 0


def test_rem_is_reachable_on_layer_0_only():
    for c in hc.CASES:
        if hc.on_fused_path(c):
            assert all(hc.ring(c, l)[3] == 0 for l in range(1, hc.n_hidden(c))), c.name


def test_batches_named_smallest_are_minimal():
    assert (hc.B_R2_2NETS, hc.B_R2_1NET, hc.B_GEMM128) == (4097, 8193, 127 * 128 + 1)
    k = hc.fusable(hc.R2_DIMS)
    assert hc.fused_rows(hc.R2_DIMS, 2, k, hc.B_R2_2NETS - 1) == 1 and hc.fused_rows(hc.R2_DIMS, 2, k, hc.B_R2_2NETS) == 2
    assert hc.fused_rows(hc.R2_DIMS, 1, k, hc.B_R2_1NET - 1) == 1 and hc.fused_rows(hc.R2_DIMS, 1, k, hc.B_R2_1NET) == 2
    assert hc.gemm_tile(hc.B_GEMM128 - 1, 128, 2) == 64 and hc.gemm_tile(hc.B_GEMM128, 128, 2) == 128
    assert hc.B_R2_LAST33 % 64 == 33 and (hc.B_R2_XCD // 64) % 4 == 0 and hc.B_R2_XCD % 64 == 0
    for name in ("229x512x256x51-n2-packed-B4129", "10x32x64x2-n2-packed-B4352"):
        assert hc.kernel(hc.CASE_BY_NAME[name]) == (2, 2), name


# --------------------------------------------------------------------------- the exact design
@pytest.mark.parametrize("name", NAMES)
def test_exact_design_is_feasible(name):
    case = hc.CASE_BY_NAME[name]
    assert hc.exact_feasible(case) is None
    assert hc.exactness_bits(case) <= 24
    assert hc.n_hidden(case) <= 3, "deeper stacks outgrow 2^24 with weights up to 3: keep them off this design"
    x = hc.network(case, "exact")[1]
    assert np.abs(x[:, 1:]).max() <= 2 and set(np.unique(x[:, 0])) <= {0.0, float(hc.GATE)}


def test_dead_units_give_exactly_minus_one_in_fp32():
    """__expf is the hardware 2^x unit, accurate to a few ulps of its RESULT (the 2^-23 of gemm.hip:156 is its size next to 1):
    exp(-32) = 1.3e-14 lies so far under half an ulp of 1 (2^-25) that even a hundredfold error leaves the difference at -1."""
    assert F32(100 * np.exp(-32.0)) - F32(1) == F32(-1) and 100 * np.exp(-32.0) < 2.0 ** -25


# --------------------------------------------------------------------------- the checks on a right forward and on wrong ones
def _clean(case, design):
    full = hc.model_hidden(case, design, stash_all=1) if not case.stash_all else None
    return full


@pytest.mark.parametrize("name", NAMES)
def test_checks_pass_on_a_float32_model(name):
    case = hc.CASE_BY_NAME[name]
    for design in hc.DESIGNS:
        for garbage in (hc.GARBAGE, np.nan):
            share = hc.check_stash(case, design, hc.model_hidden(case, design, garbage=garbage), _clean(case, design))
            assert share < 0.5, "numpy's own fp32 order sits well inside the bar"
    if hc.fusable(case.dims) and case.stash_all:
        other = case._replace(packed=not case.packed)
        hc.check_same_hidden(case, hc.model_hidden(case, "exact"), hc.model_hidden(other, "exact"))


_MODEL_CASES = ["13x96x32x3-n1-packed-B33", "13x96x32x3-n2-packed-B33-s0", "33x96x64x40-n1-packed-B33-s0", "8x544x288x32x3-n1-packed-B33",
                "3x32x1-n1-packed-B1", "48x100x36x12-n1-layers-B130", "16x48x128x5-n2-layers-B250"]


@pytest.mark.parametrize("fault", hc.FAULTS)
def test_every_check_fails_on_every_fault(fault):
    garbage = np.nan if fault == "quad_mask" else hc.GARBAGE
    hit = 0
    for name in _MODEL_CASES:
        case = hc.CASE_BY_NAME[name]
        if not hc.fault_applies(case, fault):
            continue
        for design in hc.DESIGNS:
            if case.B == 1 and fault == "drop_last_step" and design == "exact":
                continue                                           # one row: the dropped columns of x may all be zero
            hit += 1
            with pytest.raises(AssertionError):
                hc.check_stash(case, design, hc.model_hidden(case, design, fault, garbage), _clean(case, design))
    assert hit >= 2, f"{fault} applies to no model case"


def test_finite_garbage_cannot_show_a_whole_quad_mask():
    """1e30 in the ignored columns meets the arena's zero pad columns: 1e30 * 0 = 0 leaves every bit alone even when the mask inside
    the last quad is missing.  NaN * 0 = NaN does not -- the reason the GPU test's second call carries NaN there."""
    case = hc.CASE_BY_NAME["13x96x32x3-n1-packed-B33"]
    for design in hc.DESIGNS:
        assert np.all(hc.x_tile(case, design)[:, case.dims[0]:] == F32(hc.GARBAGE))
        hc.check_stash(case, design, hc.model_hidden(case, design, "quad_mask", hc.GARBAGE))
        with pytest.raises(AssertionError):
            hc.check_stash(case, design, hc.model_hidden(case, design, "quad_mask", np.nan))


def test_same_hidden_check_catches_one_bit():
    case = hc.CASE_BY_NAME["13x96x32x3-n1-packed-B33"]
    a = hc.model_hidden(case, "dense")
    b = a.copy(); b[7] = np.nextafter(b[7], F32(9))
    with pytest.raises(AssertionError, match="differ"):
        hc.check_same_hidden(case, a, b)
    b = a.copy(); b[hc.hidden_floats(case) + 1] += 1               # the output block is not compared
    hc.check_same_hidden(case, a, b)


def test_dense_bar_is_the_stated_one():
    assert hc.EXPF_ABS == 2.0 ** -23 and hc.SUB_ABS == 2.0 ** -24
    import bf16_model
    assert bf16_model.AMBIG == 4 * hc.EXPF_ABS
    assert all(0 <= v <= 1 for v in hc.MEASURED_SHARE.values())


# --------------------------------------------------------------------------- every case is asserted
def test_gpu_module_skips_nothing():
    src = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "test_forward_hidden_gpu.py")).read()
    for word in ("skip", "xfail", "importorskip"):
        assert word not in src, word
