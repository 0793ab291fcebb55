"""The table of tests/backward_cases.py means what tests/test_backward_paths_gpu.py assumes: the mirror of the backward's dispatch
agrees with the library wherever the library lets it be asked, every row reaches the launches it names and the union of the
rows' plans is the declared list, the threshold batches are minimal, every row satisfies the exactness condition the equality
asserts rest on, the stashes exercise every branch of ELU', and the checks fail on the wrong results they are there to catch.
No GPU needed."""
import ctypes as C
import os

import numpy as np
import pytest

import backward_cases as bc

F32 = np.float32
_NAMES = [c.name for c in bc.CASES]


# --------------------------------------------------------------------------- the mirror against the library
# shapes on either side of each rule: the skinny caps (16 outputs, 1024 inputs), the fused head's register budget (NB x CH <= 16),
# one layer, the compact chain's width rules
_EXTRA_DIMS = [[8, 1024, 16], [8, 1024, 17], [8, 1056, 1], [8, 256, 16], [8, 288, 16], [8, 512, 8], [8, 544, 8], [8, 1024, 4],
               [8, 1024, 5], [8, 32, 17], [40, 1], [40, 16], [40, 17], [24, 128, 128, 1], [24, 128, 96, 1], [24, 96, 128, 1],
               [24, 128, 100, 1], [24, 128, 1], [104, 512, 512, 256, 1], [88, 512, 256, 128, 16]]
_EXTRA_B = [1, 31, 32, 33, 127, 128, 129, 4095, 4096, 4097, 8160, 8161, 16320, 16321, 16383, 16385]


def _all_dims():
    seen = []
    for dims in [c.dims for c in bc.CASES] + [c.dims for c in bc.DPG_CASES] + _EXTRA_DIMS:
        if dims not in seen:
            seen.append(dims)
    return seen


def test_mirror_agrees_with_the_library_on_workspace_sizes_and_norm_parts():
    """pqlk_mlp_bwd_ws_floats (k_skinny_bwd's blocks: skinny_bwd_rows), pqlk_mlp_norm_parts (head_is_fused) and
    pqlk_dpg_backward_ws_floats load on a host without a GPU."""
    from pql_amd import _lib as L
    for c in (1, 31, 32, 33, 100):
        assert int(L.lib.pqlk_ld(c)) == bc.ld(c)
    fused = set()
    for dims in _all_dims():
        for nets in (1, 2):
            d = L.mlp_desc(dims, nets)
            assert int(L.lib.pqlk_mlp_net_stride(C.byref(d))) == bc.net_stride(dims), dims
            assert int(L.lib.pqlk_mlp_norm_parts(C.byref(d))) == bc.norm_parts(dims, nets), (dims, nets)
            fused.add(bc.head_is_fused(dims))
            batches = _EXTRA_B + [c.B for c in bc.CASES if c.dims == dims]
            for B in batches:
                for splits in (1, 8, 64):
                    assert int(L.lib.pqlk_mlp_bwd_ws_floats(C.byref(d), B, splits)) == bc.bwd_ws_floats(dims, nets, B, splits), (dims, nets, B, splits)
                assert int(L.lib.pqlk_dpg_backward_ws_floats(C.byref(d), B)) == bc.dpg_ws_floats(dims, nets, B), (dims, nets, B)
                assert int(L.lib.pqlk_mlp_acts_floats(C.byref(d), B)) == bc.acts_floats(dims, nets, B)
    assert fused == {True, False}
    # the head's partial area follows k_skinny_bwd's block count only where that exceeds the compact tiles' (b > 16 rows per 32)
    assert bc.skinny_bwd_blocks(37, 1) == 3 and bc.head_part_floats([8, 32, 1], 1, 37) == 8 * 64


def test_mirror_of_act_and_layer_offsets():
    from pql_amd import _lib as L
    for dims in ([8, 36, 12], [48, 100, 36, 12], [40, 3]):
        for nets in (1, 2):
            d = L.mlp_desc(dims, nets)
            for l in range(len(dims) - 1):
                w, b = C.c_int64(), C.c_int64()
                assert L.lib.pqlk_mlp_layer_offsets(C.byref(d), l, C.byref(w), C.byref(b)) == 0
                assert (w.value, b.value) == bc.layer_offsets(dims, l)
                for n in range(nets):
                    off, ldv = C.c_int64(), C.c_int64()
                    assert L.lib.pqlk_mlp_act_offset(C.byref(d), 37, n, l, C.byref(off), C.byref(ldv)) == 0
                    assert (off.value, ldv.value) == bc.act_offset(dims, nets, 37, n, l)


# --------------------------------------------------------------------------- the paths
@pytest.mark.parametrize("name", _NAMES)
def test_case_reaches_the_launches_it_names(name):
    c = bc.CASE_BY_NAME[name]
    plan = bc.plan(c)
    for launch in c.must:
        assert launch in plan, (launch, plan)
    assert c.form in bc.FORMS and c.ldx % 32 == 0 and c.ldx >= bc.ld(c.dims[0]) and 1 <= c.splits <= 64
    if c.form == "slice":
        assert c.cols > 0 and c.col0 + c.cols <= c.dims[0]
    assert (("reduce", True) in plan or ("reduce", False) in plan) == (c.form in ("gdx", "g"))


def test_union_of_the_plans_is_the_declared_list():
    reached = set()
    for c in bc.CASES:
        reached |= set(bc.plan(c))
    assert reached == set(bc.LAUNCHES), reached ^ set(bc.LAUNCHES)


def _rows(pred):
    return [c for c in bc.CASES if pred(c, bc.plan(c))]


def test_table_holds_what_the_suite_had_left_dark():
    sb = "skinny_bwd"
    # all nine k_skinny_bwd instantiations, each with one and with two nets and a batch that is no multiple of 16
    for nb, ch in ((1, 1), (1, 2), (1, 4), (4, 1), (4, 2), (4, 4), (8, 1), (8, 2), (16, 1)):
        mine = _rows(lambda c, p: (sb, nb, ch, 16) in p and c.B % 16 != 0)
        assert {c.nets for c in mine} == {1, 2}, (nb, ch)
        assert {c.form for c in mine} >= {"gdx", "g"}, (nb, ch)
    assert _rows(lambda c, p: (sb, 1, 1, 16) in p and c.B == 1)
    for rows, B in ((32, 8161), (64, 16321)):          # one row past a block boundary
        mine = _rows(lambda c, p: (sb, 1, 1, rows) in p)
        assert mine and all(c.B == B and c.B % rows == 1 and c.nets == 2 for c in mine)
    # the non-fused skinny head: both dY stagings, 5-8 outputs over more than 512 inputs, one layer with dx, CLS = 16 at its threshold,
    # k_skinny_dx alone past its grid cap
    for dims in ([8, 288, 9], [8, 288, 12], [8, 544, 5]):
        assert _rows(lambda c, p: c.dims == dims and ("skinny_dw", 4) in p and ("skinny_dx",) in p), dims
    assert _rows(lambda c, p: c.dims == [40, 3] and c.form == "gdx" and ("skinny_dw", 4) in p)
    assert _rows(lambda c, p: c.dims == [8, 1024, 6] and c.nets == 2 and c.splits == 8 and ("skinny_dw", 16) in p)
    assert _rows(lambda c, p: c.form == "dx" and p[0] == ("skinny_dx",) and bc.cdiv(c.B, 4) > 2048)
    # the GEMM head
    for dims in ([8, 64, 17], [8, 64, 51], [8, 1056, 4]):
        assert _rows(lambda c, p: c.dims == dims and p[0][0] in ("dW", "dX") and "skinny_dx" not in [t[0] for t in p]), dims
    # k_gemm: every (tile, loop) pair and every block order per mode; whole and ragged grids
    for mode, epi in (("dW", "NONE"), ("dX", "DELU")):
        mine = {t for c in bc.CASES for t in bc.plan(c) if t[:2] == (mode, epi)}
        assert {(t[2], t[3]) for t in mine} == {(64, "staged"), (64, "dma"), (128, "staged"), (128, "dma")}, mode
        assert {t[4] for t in mine} == {0, "groups", "runs"}, mode
        assert {t[5] for t in mine} == {False, True}, mode
    assert _rows(lambda c, p: c.dims == [48, 100, 36, 12])
    assert _rows(lambda c, p: c.ldx > bc.ld(c.dims[0]) and ("dW", "NONE", 64, "dma", 0, True) in p)
    # a reduction of exactly one four-stage DMA group, and of 96 on the register-staged interior loop, in both modes
    assert _rows(lambda c, p: c.B == 64 and c.splits == 1 and ("dW", "NONE", 64, "dma", 0, False) in p)
    assert _rows(lambda c, p: c.B == 96 and c.splits == 1 and ("dW", "NONE", 64, "staged", 0, False) in p)
    assert _rows(lambda c, p: c.dims == [8, 64, 64, 17] and ("dX", "DELU", 64, "dma", 0, False) in p)
    assert _rows(lambda c, p: c.dims == [8, 64, 96, 17] and ("dX", "DELU", 64, "staged", 0, False) in p)
    # splits: 1, default_splits(B) > 1, a count with empty trailing slabs, 64 -- on the GEMM dW, on k_skinny_dw, under a fused head
    for kind in ("dW", "skinny_dw"):
        mine = _rows(lambda c, p: any(t[0] == kind for t in p))
        assert any(c.splits == 1 for c in mine), kind
        assert any(c.splits == bc.default_splits(c.B) > 1 for c in mine), kind
        assert any(c.B == 96 and c.splits == 8 and bc.empty_splits(c.B, c.splits) == 5 for c in mine), kind
        assert any(c.splits == 64 and bc.empty_splits(c.B, c.splits) > 0 for c in mine), kind
    assert _rows(lambda c, p: p[0][0] == sb and bc.empty_splits(c.B, c.splits) > 0 and any(t[0] == "dW" for t in p))
    assert _rows(lambda c, p: ("dW", "NONE", 128, "staged", "groups", False) in p and bc.empty_splits(c.B, c.splits) > 0)
    # the input gradient: zsum GEMM with one and two nets; k_dx_slice at every depth with one and two nets, col0 % 4 != 0 and == 0,
    # 1, 5 and 32 columns; the slice GEMM through its three doors, with col0 % 4 != 0
    assert {c.nets for c in _rows(lambda c, p: any(t[:2] == ("dX", "NONE") for t in p))} == {1, 2}
    sl = _rows(lambda c, p: p[-1][0] == "dx_slice")
    assert {c.cols for c in sl} >= {1, 5, 32} and {c.col0 % 4 == 0 for c in sl} == {True, False}
    assert any(c.B > 32 for c in sl) and any(c.B % 32 for c in sl)
    doors = _rows(lambda c, p: p[-1][:2] == ("dX", "DTANH_SLICE"))
    assert any(c.cols > 32 and c.col0 & 3 for c in doors) and any(c.dims[1] % 32 for c in doors)
    assert any(c.nets == 2 and c.dims[1] > 632 and c.cols <= 32 and c.dims[1] % 32 == 0 and c.col0 & 3 for c in doors)
    assert {c.form for c in bc.CASES} == set(bc.FORMS)
    for name in bc.LAYERS_CASES:
        assert name in bc.CASE_BY_NAME and bc.CASE_BY_NAME[name].form in ("gdx", "g")


def test_thresholds_are_the_smallest():
    assert (bc.B_ROWS32, bc.B_ROWS64, bc.B_DX_CAP, bc.B_DX128, bc.S_DW128, bc.S_CLS16) == (8161, 16321, 8193, 3969, 8, 8)
    assert bc.skinny_bwd_rows(bc.B_ROWS32 - 1, 2) == 16 and bc.skinny_bwd_rows(bc.B_ROWS64 - 1, 2) == 32
    assert bc.skinny_dx_blocks(bc.B_DX_CAP - 1) == 2048 == bc.cdiv(bc.B_DX_CAP - 1, 4)
    wide = lambda B, s: bc.backward_plan(bc.WIDE, 2, B, s, True, None)      # noqa: E731
    assert [t[2] for t in wide(bc.B_DX128, bc.S_DW128) if t[0] in ("dW", "dX")] == [128, 128, 64]
    assert [t[2] for t in wide(bc.B_DX128 - 1, bc.S_DW128) if t[0] in ("dW", "dX")] == [128, 64, 64]
    assert [t[2] for t in wide(bc.B_DX128, bc.S_DW128 - 1) if t[0] in ("dW", "dX")] == [64, 128, 64]
    assert bc.skinny_dw_cls(1024, bc.S_CLS16 - 1, 2) == 4 and bc.skinny_dw_cls(1024, bc.S_CLS16, 2) == 16
    # the slice kernel's LDS rule: two nets fit up to a first hidden width of 632
    assert bc.dx_slice_ok(2, 608, 5, 608) and not bc.dx_slice_ok(2, 640, 5, 640) and bc.dx_slice_ok(1, 1024, 5, 1024)
    assert not bc.dx_slice_ok(1, 64, 33, 64) and bc.dx_slice_ok(1, 64, 32, 64) and not bc.dx_slice_ok(1, 48, 5, 64)


def test_dpg_cases_take_the_chain_they_name():
    for c in bc.DPG_CASES:
        assert bc.minnet_ok(c.dims, c.nets, c.cols) == c.compact, c.name
        assert c.col0 + c.cols <= c.dims[0]
    assert {c.B for c in bc.DPG_CASES} == {1, 130, 257} and {(c.col0, c.cols) for c in bc.DPG_CASES} == {(8, 16), (19, 5)}
    dense = [c for c in bc.DPG_CASES if not c.compact]
    assert dense and all(bc.backward_plan(c.dims, 2, c.B, 1, False, ("slice", c.col0, c.cols))[-1] == ("dx_slice", 4, 2) for c in dense)
    for c in bc.DPG_CASES:
        for pattern in bc.OWNERS:
            own, q = bc.owner_input(bc.as_case(c), pattern)
            derived = (q[0] <= q[1]).astype(np.uint8) | ((q[1] <= q[0]).astype(np.uint8) << 1)      # minnet.h:25-26
            assert np.array_equal(own, derived)
            dy = bc.dpg_dy_input(bc.as_case(c), own)
            assert np.all((dy[0, :, 0] != 0) == ((own & 1) != 0)) and np.all((dy[1, :, 0] != 0) == ((own & 2) != 0))
        own, _ = bc.owner_input(bc.as_case(c), "mixed")
        assert c.B == 1 or set(own.tolist()) == {1, 2, 3}


# --------------------------------------------------------------------------- exactness
@pytest.mark.parametrize("name", _NAMES)
def test_case_is_exactly_summable(name):
    assert bc.exactness_bits(bc.CASE_BY_NAME[name]) <= 24


@pytest.mark.parametrize("name", [c.name for c in bc.DPG_CASES])
def test_dpg_case_is_exactly_summable(name):
    c = bc.DPG_BY_NAME[name]
    for pattern in (bc.OWNERS if c.compact else (None,)):
        assert bc.exactness_bits(bc.as_case(c), pattern) <= 24, pattern


def test_exactness_condition_is_what_makes_fp32_sums_order_free():
    """The condition on a sum that meets it and on one that does not: 2^12 terms of 2^12 + 0.5 reach 2^24 + 2^11 (a granularity of
    0.5 at 25 bits), and fp32 partial sums taken forward and pairwise then differ from each other or from the float64 sum."""
    ok = np.full(4096, 2.0 ** 11 - 0.5, dtype=F32)
    bad = np.full(4096, 2.0 ** 12 + 0.5, dtype=F32)
    for v, exact in ((ok, True), (bad, False)):
        bits = np.log2(np.abs(v).astype(np.float64).sum() * 2)
        assert (bits <= 24) == exact
        fwd = F32(0)
        for t in v:
            fwd = F32(fwd + t)
        assert (float(fwd) == float(v.astype(np.float64).sum())) == exact


# --------------------------------------------------------------------------- the design reaches the branches
@pytest.mark.parametrize("name", _NAMES + [c.name for c in bc.DPG_CASES])
def test_every_stash_patch_holds_every_branch_of_elu_prime(name):
    """Every 32-row by 32-column patch of every hidden block (clipped at the block's edge) holds h > 0, -1 < h <= 0 and h = -1."""
    case = bc.CASE_BY_NAME[name] if name in bc.CASE_BY_NAME else bc.as_case(bc.DPG_BY_NAME[name])
    for net in bc.hidden(case):
        for h in net:
            for r0 in range(0, h.shape[0], 32):
                for c0 in range(0, h.shape[1], 32):
                    p = h[r0: r0 + 32, c0: c0 + 32]
                    assert (p > 0).any() and ((p <= 0) & (p > -1)).any() and (p == -1).any(), (name, r0, c0)


def test_inputs_have_zero_pads_and_poisoned_outputs():
    for name in ("48x100x36x12-n1-B130-s1-gdx", "88x64x3-n1-B128-s1-gdx-ldx128", "8x288x12-n2-B96-s8-gdx"):
        c = bc.CASE_BY_NAME[name]
        x, a, s = bc.x_input(c), bc.arena(c), bc.stash(c)
        assert np.all(x[:, c.dims[0]: bc.ld(c.dims[0])] == 0) and np.all(x[:, bc.ld(c.dims[0]):] == bc.IN_ONE)
        assert set(np.unique(x[:, : c.dims[0]])) == {-2, -1, 0, 1, 2}
        ns = bc.net_stride(c.dims)
        for n in range(c.nets):
            for l in range(len(c.dims) - 1):
                wo, bo = bc.layer_offsets(c.dims, l)
                w = a[n * ns + wo: n * ns + bo].reshape(c.dims[l + 1], bc.ld(c.dims[l]))
                assert np.all(w[:, c.dims[l]:] == 0) and set(np.unique(w[:, : c.dims[l]])) == {-1, 0, 1}
                assert np.all(a[n * ns + bo + c.dims[l + 1]: n * ns + bo + bc.ld(c.dims[l + 1])] == 0)
                if l < len(c.dims) - 2:
                    off, ldh = bc.act_offset(c.dims, c.nets, c.B, n, l)
                    assert np.all(s[off: off + c.B * ldh].reshape(c.B, ldh)[:, c.dims[l + 1]:] == 0)
        off, _ = bc.act_offset(c.dims, c.nets, c.B, 0, len(c.dims) - 2)
        assert np.all(np.isnan(s[off:])) and not np.any(np.isnan(s[:off]))
        assert np.all(bc.dy_input(c)[:, :, c.dims[-1]:] == 0)


# --------------------------------------------------------------------------- the checks pass on a right result and fail on wrong ones
_MODEL_CASES = ["8x64x64x17-n2-B96-s8-gdx", "8x288x12-n2-B96-s8-gdx", "48x100x36x12-n1-B130-s1-gdx", "40x64x1-n2-B37-s1-slice-c7+32",
                "24x1024x1-n2-B130-s1-slice-c19+5"]


def _run_checks(case, grads, dx):
    before = np.full(dx.shape, bc.POISON, dtype=F32)
    if case.form in ("gdx", "g"):
        bc.check_grads(grads, case)
    if case.form in ("gdx", "dx"):
        bc.check_dx_full(dx, before, case)
    if case.form == "slice":
        bc.check_dx_slice(dx, before, case)


@pytest.mark.parametrize("name", _MODEL_CASES)
def test_checks_pass_on_a_plain_backward_and_catch_planted_faults(name):
    case = bc.CASE_BY_NAME[name]
    _run_checks(case, *bc.model_backward(case))
    for fault in bc.FAULTS:
        if fault == "stale_slab" and not (case.form != "slice" and bc.empty_splits(case.B, case.splits)):
            continue
        if fault == "slice_shift" and not (case.form == "slice" and case.col0 & 3):
            continue
        if fault == "pad" and (case.form == "slice" or bc.ld(case.dims[0]) == case.dims[0]):
            continue
        if fault == "nets_not_summed" and case.nets == 1:
            continue
        with pytest.raises(AssertionError):
            _run_checks(case, *bc.model_backward(case, fault))
    # each gradient on its own: the fault moves dW AND dx where both exist
    if case.form == "gdx":
        for fault in ("last_row", "stage", "no_elu"):
            grads, dx = bc.model_backward(case, fault)
            with pytest.raises(AssertionError, match="arena"):
                bc.check_grads(grads, case)
            with pytest.raises(AssertionError, match="dx"):
                bc.check_dx_full(dx, np.full(dx.shape, bc.POISON, dtype=F32), case)


def test_every_fault_is_planted_somewhere():
    planted = set()
    for name in _MODEL_CASES:
        case = bc.CASE_BY_NAME[name]
        planted |= {"last_row", "stage", "no_elu"}
        if case.form != "slice" and bc.empty_splits(case.B, case.splits):
            planted.add("stale_slab")
        if case.form == "slice" and case.col0 & 3:
            planted.add("slice_shift")
        if case.form != "slice" and bc.ld(case.dims[0]) > case.dims[0]:
            planted.add("pad")
        if case.nets == 2:
            planted.add("nets_not_summed")
    assert planted == set(bc.FAULTS)


def test_dx_checks_catch_a_write_outside_the_columns():
    case = bc.CASE_BY_NAME["48x100x36x12-n1-B130-s1-gdx"]
    _, dx = bc.model_backward(case)
    before = np.full(dx.shape, bc.POISON, dtype=F32)
    spilled = dx.copy(); spilled[3, bc.ld(case.dims[0])] = 0.0
    with pytest.raises(AssertionError, match="past"):
        bc.check_dx_full(spilled, before, case)
    dirty = dx.copy(); dirty[3, case.dims[0]] = bc.POISON
    with pytest.raises(AssertionError, match="pad"):
        bc.check_dx_full(dirty, before, case)
    nan = dx.copy(); nan[0, 0] = np.nan
    with pytest.raises(AssertionError, match="differ"):
        bc.check_dx_full(nan, before, case)
    case = bc.CASE_BY_NAME["40x64x1-n2-B37-s1-slice-c7+32"]
    _, dx = bc.model_backward(case)
    before = np.full(dx.shape, bc.POISON, dtype=F32)
    spilled = dx.copy(); spilled[:, case.cols] = 0.0
    with pytest.raises(AssertionError, match="past the slice written"):
        bc.check_dx_slice(spilled, before, case)
    with pytest.raises(AssertionError, match="not zero"):
        bc.check_dx_slice(dx, before, case, rest="zero")


# --------------------------------------------------------------------------- every case is asserted, with equality only
def test_gpu_module_skips_nothing_and_has_no_tolerance():
    src = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "test_backward_paths_gpu.py")).read()
    for word in ("skip", "xfail", "importorskip", "rtol", "atol", "allclose", "assert_close"):
        assert word not in src, word
