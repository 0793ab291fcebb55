"""The table of tests/backward_cases.py means what tests/test_backward_paths_gpu.py assumes: the mirror of the backward's dispatch
agrees with the library wherever the library lets it be asked, every row reaches the launches it names and the union of the
rows' plans is the declared list, the threshold batches are minimal, every row satisfies the exactness condition the equality
asserts rest on, the stashes exercise every branch of ELU', and the checks fail on the wrong results they are there to catch.
The same for the TD family (tests/test_td_paths_gpu.py): the mirror of the fused forward's and the TD entries' dispatch against
the library's host-only counts, the kernel instances the tables reach, the data rules, exact summability, and the exactly
evaluable network of the forward path.  No GPU needed."""
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


# =========================================================================== the TD family (tests/test_td_paths_gpu.py)
_TD_EXTRA_DIMS = [bc.TD_TAKEN, bc.TD_REFUSED, [8, 32, 32, 1], [8, 1024, 32, 1], [8, 1056, 32, 1], [8, 100, 32, 1], [8, 288, 32, 2],
                  [8, 288, 36, 1], [8, 128, 1], [8, 288, 1], [8, 640, 32, 1], [620, 32, 288, 1], [8, 288, 288, 32, 1],
                  [104, 512, 512, 256, 1], [8, 288, 32, 17]]
_TD_EXTRA_B = [1, 31, 32, 33, 63, 64, 65, 4095, 4096, 4097, 8160, 8161, 8191, 8192, 8193, 16320, 16321, 16384, 16385]


def _td_dims():
    seen = []
    for dims in [c.dims for c in bc.TD_CASES] + _TD_EXTRA_DIMS + [bc.NORM_PLAIN_DIMS]:
        if dims not in seen:
            seen.append(dims)
    return seen


def test_td_mirror_agrees_with_the_library():
    """pqlk_td_forward_loss_parts (fusable / buf_ld, fused_lds_bytes, fused_rows, td_forward_tiles), pqlk_td_head_loss_parts
    (skinny_bwd_blocks) and pqlk_mlp_norm_parts over every TD case and a sweep across the edges: buf_ld - Kh = 256, one hidden
    layer, a width over 1024 or no multiple of 32, two outputs, the R = 1 | 2 switch at 4096 | 4097, a tile too wide for R = 2, the
    16 | 32 | 64-row switches of k_skinny_bwd."""
    from pql_amd import _lib as L
    fwd, head, rows2 = set(), set(), set()
    for dims in _td_dims():
        for nets in (1, 2):
            d = L.mlp_desc(dims, nets)
            assert int(L.lib.pqlk_mlp_norm_parts(C.byref(d))) == bc.norm_parts(dims, nets), (dims, nets)
            for B in _TD_EXTRA_B + [c.B for c in bc.TD_CASES if c.dims == dims]:
                got = int(L.lib.pqlk_td_forward_loss_parts(C.byref(d), B))
                assert got == bc.td_forward_loss_parts(dims, nets, B), (dims, nets, B)
                fwd.add(got > 0)
                if got:
                    rows2.add(bc.fused_rows(dims, nets, B))
                got = int(L.lib.pqlk_td_head_loss_parts(C.byref(d), B))
                assert got == bc.td_head_loss_parts(dims, nets, B) == (bc.skinny_bwd_blocks(B, 2) * 2 if got else 0), (dims, nets, B)
                head.add(got > 0)
    assert fwd == {True, False} and head == {True, False} and rows2 == {1, 2}
    # the edges themselves
    assert bc.buf_ld(bc.TD_TAKEN) - bc.TD_TAKEN[-2] == 260 and bc.buf_ld(bc.TD_REFUSED) - bc.TD_REFUSED[-2] == 228
    assert bc.td_forward_tiles(bc.TD_TAKEN, 2, 33) == 2 and bc.td_forward_tiles(bc.TD_REFUSED, 2, 33) == 0
    assert bc.buf_ld([300, 64, 64, 1]) == 324 and bc.buf_ld([8, 1056, 32, 1]) == 0 and bc.buf_ld([8, 100, 32, 1]) == 0
    assert bc.fused_rows(bc.TD_TAKEN, 2, 4096) == 1 and bc.fused_rows(bc.TD_TAKEN, 2, 4097) == 2 and bc.fused_rows(bc.TD_TAKEN, 2, 8192) == 2
    assert bc.fused_rows(bc.TD_TAKEN, 2, 8193) == 1
    assert bc.fused_rows([620, 32, 288, 1], 2, 8192) == 1 and bc.td_forward_tiles([620, 32, 288, 1], 2, 8192) == 256
    assert bc.td_forward_tiles(bc.TD_TAKEN, 1, 33) == 0 and bc.td_forward_tiles([8, 288, 32, 2], 2, 33) == 0
    assert bc.td_head_loss_parts([8, 32, 1], 2, 8160) == 1020 and bc.td_head_loss_parts([8, 32, 1], 2, 8161) == 512
    assert bc.td_head_loss_parts([8, 32, 1], 2, 16320) == 1020 and bc.td_head_loss_parts([8, 32, 1], 2, 16321) == 512
    assert bc.td_head_loss_parts([8, 1056, 1], 2, 16) == 0 and bc.td_head_loss_parts([8, 32, 2], 2, 16) == 0


def test_td_tables_reach_every_kernel_instance():
    bwd = [c for c in bc.TD_CASES if c.path == "bwd"]
    fwd = [c for c in bc.TD_CASES if c.path == "fwd"]
    assert {bc.td_instance(c) for c in bwd} == set(bc.TD_BWD_INSTANCES)
    assert {bc.td_instance(c) for c in fwd} == set(bc.TD_FWD_INSTANCES)
    for c in bc.TD_CASES:
        d = c.dims
        assert c.splits == bc.default_splits(c.B) and bc.td_head_loss_parts(d, 2, c.B) > 0, c.name
        assert c.path == "bwd" or bc.td_forward_loss_parts(d, 2, c.B) > 0, c.name
    # k_skinny_bwd<1, CH, true>: CH by the last hidden ld; every row count with a whole and with a ragged last block
    assert {bc.ld(c.dims[-2]) for c in bwd} >= {32, 288, 512, 1024}
    assert {c.B for c in bwd} >= {1, 15, 16, 17, 8160, 8161, 8192, 16320, 16321} and max(c.B for c in bc.TD_CASES) == 16321
    for rows in (16, 32, 64):
        mine = [c for c in bwd if bc.td_instance(c)[1] == rows]
        assert any(c.B % rows for c in mine), rows
    assert any(bc.td_instance(c) == (1, 32) and bc.is_pow2(c.B) for c in bwd)
    # k_mlp_fwd_fused: R = 1 at 1, 31, 32, 33; R = 2 at its first batch (one row in the last 64-row tile) and at 8192; TM = 4; the
    # last hidden widths; two chunks of the head-backward quad loop under both TM; an input wider than every hidden layer
    r1 = {c.B for c in fwd if bc.td_instance(c) == (1, 2) and c.dims == bc.TD_TAKEN}
    assert r1 >= {1, 31, 32, 33} and {c.B for c in fwd if bc.td_instance(c)[0] == 2} == {4097, 8192} and 4097 % 64 == 1
    assert {c.dims[-2] for c in fwd} == {32, 64, 256, 288}
    assert {bc.td_instance(c)[1] for c in fwd if c.dims[-2] // 4 > 64} == {2, 4}
    assert any(bc.ld(c.dims[0]) > max(c.dims[1:-1]) for c in fwd)
    # section 4's batches on both paths; done = 0.5 on both paths
    for path in (bwd, fwd):
        assert {c.B for c in path} >= {33, 65, 95, 4097}
        assert any(c.data == "half" for c in path)
    for names in (bc.TD_LAYERS_NAMES, bc.TD_NORM_BWD_NAMES, bc.TD_NORM_FWD_NAMES):
        assert all(n in bc.TD_BY_NAME for n in names)
    assert any(len(bc.TD_BY_NAME[n].dims) == 3 for n in bc.TD_LAYERS_NAMES) and any(len(bc.TD_BY_NAME[n].dims) == 4 for n in bc.TD_LAYERS_NAMES)
    assert any(not bc.is_pow2(bc.TD_BY_NAME[n].B) for n in bc.TD_LAYERS_NAMES)


@pytest.mark.parametrize("name", [c.name for c in bc.TD_CASES])
def test_td_case_holds_the_data_rules_and_is_exactly_summable(name):
    """Q' integers in [-2, 2] with ties and rows where net 1 is the minimum, gamma^n = 0.5, r a multiple of 0.5, done in {0, 1} (or
    0.5 where the case says so); on path "bwd" Q integers in [-2, 2]; every loss partial exactly summable; for B a power of two
    every gradient element exactly summable (at most 24 bits), dy = 2 / B dq exact."""
    p, tc = bc.td_problem(name), bc.TD_BY_NAME[name]
    assert bc.GAMMA_N == 0.5
    assert np.array_equal(p.qt, np.round(p.qt)) and np.abs(p.qt).max() <= 2
    tie, net1 = p.qt[0] == p.qt[1], p.qt[1] < p.qt[0]
    assert net1[0] and (tc.B < 3 or (tie.any() and net1.any() and (p.qt[0] < p.qt[1]).any()))
    assert np.array_equal(p.rew * 2, np.round(p.rew * 2))
    assert set(np.unique(p.done)) <= ({0.0, 0.5, 1.0} if tc.data == "half" else {0.0, 1.0})
    assert tc.data != "half" or {0.0, 0.5, 1.0} == set(np.unique(p.done))
    assert tc.B < 16 or {0.0, 1.0} <= set(np.unique(p.done))
    assert np.array_equal(p.q, np.round(p.q))
    if tc.path == "bwd":
        assert np.abs(p.q).max() <= 2
    assert np.array_equal(p.y, p.rew + ((1.0 - p.done) * 0.5) * np.minimum(p.qt[0], p.qt[1])) and np.array_equal(p.dq, p.q - p.y)
    bits, loss_bits = bc.td_exactness_bits(name)
    assert loss_bits <= 24
    parts = bc.td_loss_parts(name)
    n_parts = bc.td_head_loss_parts(tc.dims, 2, tc.B) if tc.path == "bwd" else bc.td_forward_loss_parts(tc.dims, 2, tc.B)
    assert len(parts) == n_parts and parts.sum() == (p.dq ** 2).sum()
    assert np.log2(max(parts.sum(), 1.0) * 4.0 ** bc._gran(p.dq)) <= 24          # ... and so is their fold
    if bc.is_pow2(tc.B):
        assert bits <= 24
        assert np.array_equal(p.dy[:, :, 0].astype(np.float64), 2.0 / tc.B * p.dq)
    assert np.all(p.dy[:, :, 1:] == 0)


@pytest.mark.parametrize("name", bc.TD_FWD_NAMES)
def test_forward_case_is_exactly_evaluable(name):
    """Weights over {-1, 0, 1} and sparse, x and biases integers, every hidden pre-activation (float64) an integer >= 0 or <= -32
    with both branches in every hidden layer of every net; the fp32 ELU of such a z is z or exactly -1; the sums of the forward
    stay far below 2^24, so any order gives them."""
    p = bc.td_problem(name)
    case, dims = p.case, p.case.dims
    Z, H, Q = bc.exact_forward(case, p.W, p.bias, p.x)
    assert np.array_equal(p.x, np.round(p.x)) and np.all(p.x[:, dims[0]:] == 0)
    for n in range(2):
        for l, w in enumerate(p.W[n]):
            assert set(np.unique(w)) <= {-1.0, 0.0, 1.0} and (w != 0).sum(1).max() <= max(3, dims[-2] // 8)
            assert np.array_equal(p.bias[n][l], np.round(p.bias[n][l]))
            mass = np.abs(p.x[:, : dims[0]] if l == 0 else H[n][l - 1]).astype(np.float64) @ np.abs(w).T.astype(np.float64)
            assert (mass + np.abs(p.bias[n][l])).max() < 2 ** 20
        for l, z in enumerate(Z[n]):
            assert np.array_equal(z, np.round(z)) and np.all((z >= 0) | (z <= -32)), (n, l)
            assert (z > 0).any() and (z <= -32).any(), (n, l)
            elu = np.where(z > 0, z, np.exp(np.minimum(z, 0.0)).astype(F32) - F32(1)).astype(F32)
            assert np.array_equal(elu, H[n][l]) and np.array_equal(H[n][l], p.H[n][l])
        if case.B > 4:      # layer 0's gated units are dead on some rows and alive on others
            z = Z[n][0][:, 2]
            assert (z <= -32).any() and (z >= 0).any()
    assert np.array_equal(Q, p.q)
    assert p.tc.data == "int" or not np.array_equal(p.W[0][0], p.W[1][0])


def test_exp_of_minus_32_vanishes_beside_one():
    """exp(z) < 2^-25 for z <= -32: whatever a fast exponential returns there, within a factor of two, `__expf(z) - 1.f` is -1."""
    assert 2 * np.exp(-32.0) < 2.0 ** -25 and F32(F32(2 * np.exp(-32.0)) - F32(1)) == F32(-1)


def test_norm_cases_have_integer_gradients_within_24_bits():
    for name in bc.TD_NORM_BWD_NAMES + bc.TD_NORM_FWD_NAMES:
        ref, p = bc.td_reference(name), bc.td_problem(name)
        assert p.case.B == 8 and np.array_equal(p.dq / 4, np.round(p.dq / 4)), name
        assert np.array_equal(ref["grads"], np.round(ref["grads"])) and 0 < ref["sumsq"] <= 2 ** 24, name
        assert bc.sumsq_bits(ref["grads"]) == (float(np.log2(ref["sumsq"])), 0)
        assert bc.head_is_fused(p.case.dims)
    # head only: every hidden-layer gradient is zero, the head's dW and db are not
    name = [n for n in bc.TD_NORM_BWD_NAMES if n.endswith("head_only")][0]
    g, dims = bc.td_reference(name)["grads"], bc.TD_BY_NAME[name].dims
    for net in range(2):
        a, b = bc.head_range(dims, net)
        assert np.all(g[net * bc.net_stride(dims): a] == 0) and np.count_nonzero(g[a: a + dims[-2]]) == dims[-2] and g[a + dims[-2]] != 0
    # the non-fused head of pqlk_mlp_backward_norm
    case = bc.norm_plain_case()
    assert not bc.head_is_fused(case.dims) and bc.skinny_bwd_ok(case.dims[-1], bc.ld(case.dims[-2]))
    assert bc.norm_parts(case.dims, 2) == bc.cdiv(bc.net_stride(case.dims) * 2 // 4, 256)
    g = bc.norm_plain_reference(case)
    assert np.array_equal(g, np.round(g)) and 0 < (g * g).sum() <= 2 ** 24
    assert not np.isnan(bc.norm_plain_stash(case)[: bc.act_offset(case.dims, 2, case.B, 0, 1)[0]]).any()


def test_head_sum_bound_catches_a_dropped_and_a_doubled_row():
    """The bound of the forward path's head sums, (B + 8) 2^-24 sum |t|, is about B^2 2^-24 average terms: at B = 95 one dropped or
    doubled row moves a sum by hundreds of times the bound; at B = 4097 it is about one average term, and there the bit-equal
    hidden gradients (which read every row's dL/dQ) and the exact loss partials carry the row count.  fp32 sums taken forward and
    reversed stay inside the bound at either size."""
    for name, factor in (("8x288x32x1-B95-fwd", 100.0), ("8x288x32x1-B4097-fwd", 1.0)):
        p, ref = bc.td_problem(name), bc.td_reference(name)
        a, _ = bc.head_range(p.case.dims, 0)
        Kh = p.case.dims[-2]
        bound = bc.head_sum_bound(p, ref)[a: a + Kh + 1]
        row = int(np.argmax(np.abs(p.dy[0, :, 0])))
        moved = np.abs(np.concatenate([p.dy[0, row, 0] * p.H[0][-1][row].astype(np.float64), [p.dy[0, row, 0]]]))
        assert moved.max() > factor * bound.max(), name
        terms = p.dy[0, :, :1] * p.H[0][-1]
        for order in (terms, terms[::-1]):
            got = np.cumsum(order, axis=0, dtype=F32)[-1]
            assert np.all(np.abs(got - ref["grads"][a: a + Kh]) <= bound[:Kh]), name


def test_td_gpu_module_skips_nothing():
    src = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "test_td_paths_gpu.py")).read()
    for word in ("skip", "xfail", "importorskip", "rtol", "atol", "allclose", "assert_close"):
        assert word not in src, word


def test_operand_order_values_tell_the_orders_apart():
    for name in (bc.ORDER_BWD_NAME, bc.ORDER_FWD_NAME):
        p = bc.order_problem(name)
        assert p.case.B == 1 and p.qt[1, 0] < p.qt[0, 0]
        for q in p.q[:, 0]:
            want = bc.td_db_in_order(q)
            assert want != bc.td_db_in_order(q, "gamma_first") and want != bc.td_db_in_order(q, "fma"), (name, q)
