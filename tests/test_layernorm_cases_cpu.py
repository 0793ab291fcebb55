"""What tests/layernorm_cases.py guarantees, proven without a GPU: the shape table crosses every seam and cap the header documents,
torch's own fp32 CPU result stays inside the bars the GPU tests use on every generic input, and on the exact design the op-by-op
model of the law gives the same bits in any summation order -- the bits of torch's fp32 CPU `layer_norm`."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import layernorm_cases as lc

F32 = np.float32
T = lc.T


def test_shape_table_crosses_every_seam_and_cap():
    assert lc.header_constant("PQLK_LN_CHUNKS") == lc.CHUNKS, "PQLK_LN_CHUNKS moved: update layernorm_cases.CHUNKS"
    assert lc.header_constant("PQLK_LN_ROW_BLOCKS") == lc.ROW_BLOCKS, "PQLK_LN_ROW_BLOCKS moved: update layernorm_cases.ROW_BLOCKS"
    cols = {c for _, c in lc.SHAPES}
    ms = {m for m, _ in lc.SHAPES}
    assert {1, 2, 33, 64, 65, 128, 130, 512, 1024, 1025} <= cols
    for seam in lc.REG_SEAMS:
        assert seam in cols and seam + 1 in cols, seam
    assert {1, 3, 5, 257} <= ms
    assert lc.ROWS_PER_BLOCK * lc.CHUNKS + 1 in ms and lc.ROWS_PER_BLOCK * lc.ROW_BLOCKS + 1 in ms
    # past the chunk cap on the register path (scalar tail and ragged vector width) and on the strided path
    assert {(lc.M_PAST_CHUNKS, 33), (lc.M_PAST_CHUNKS, 130), (lc.M_PAST_CHUNKS, 1025)} <= set(lc.SHAPES)
    # the fold launch: fewer chunks than groups (m = 1, 3, 5), a ragged last group (m = 257: 65 chunks), every group full (513 chunks
    # would not exist: the cap makes it 512)
    assert -(-257 // lc.ROWS_PER_BLOCK) % lc.FOLD_GROUPS != 0


def test_torch_fp32_cpu_stays_inside_the_bars():
    """torch's fp32 CPU `F.elu(F.layer_norm)` and its autograd against the float64 reference on EVERY generic input: inside the
    forward bar (rtol 1e-5, atol 5e-6) and the backward bar (rtol 2e-5, atol 2e-5 max|ref|).  The bars are therefore wide enough
    for a correct fp32 implementation.  Largest fractions of the bar used (printed): see the assert messages."""
    worst = dict(y=0.0, bwd=0.0)
    for m, cols in lc.SHAPES:
        inp, ref = lc.generic_case(m, cols)
        got = lc.torch_reference(*inp, dtype=torch.float32)
        frac = np.abs(got["y"] - ref["y"]) / (lc.Y_BAR["atol"] + lc.Y_BAR["rtol"] * np.abs(ref["y"]))
        worst["y"] = max(worst["y"], float(frac.max()))
        assert frac.max() <= 1.0, (m, cols, float(frac.max()))
        for k in ("dz", "dgamma", "dbeta"):
            if cols < 2:
                continue
            frac = np.abs(got[k] - ref[k]) / (lc.bwd_atol(ref[k]) + lc.BWD_RTOL * np.abs(ref[k]))
            worst["bwd"] = max(worst["bwd"], float(frac.max()))
            assert frac.max() <= 1.0, (m, cols, k, float(frac.max()))
    print(f"torch fp32 CPU uses at most {worst['y']:.3f} of the forward bar and {worst['bwd']:.4f} of the backward bar")
    assert worst["y"] < 0.5 and worst["bwd"] < 0.5


def test_generic_inputs_run_both_elu_branches():
    _, ref = lc.generic_case(5, 130)
    assert (ref["y"] > 0).mean() > 0.2 and (ref["y"] < 0).mean() > 0.2


@pytest.mark.parametrize("cols", sorted(set(lc.EXACT_COLS + lc.EXACT_COLS_TORCH)))
def test_exact_design_is_order_free_and_equals_torch(cols):
    """Rows are permutations of a zero-sum multiset of integers in [-2, 2]: mean = 0 and sum z^2 an integer in any order, so the
    model's bits do not depend on the summation order; and they are the bits of torch's fp32 CPU layer_norm."""
    m = 3
    z, gamma, beta = lc.exact_inputs(m, cols)
    assert np.all(z.sum(1) == 0) and np.all(np.abs(z) <= 2) and np.all(z == np.round(z))
    assert set(np.unique(gamma)) <= {0.25, 0.5, 0.75, 1.0} and np.all(beta == 20.0)
    y0, mean0, rstd0 = lc.model_forward(z, gamma, beta)
    assert np.all(mean0 == 0) and np.all(y0 > 0)
    rs = np.random.RandomState(5)
    for order in (np.arange(cols)[::-1], rs.permutation(cols), rs.permutation(cols), "exact"):
        y1, mean1, rstd1 = lc.model_forward(z, gamma, beta, order=order)
        assert np.array_equal(y0.view(np.uint32), y1.view(np.uint32))
        assert np.array_equal(rstd0.view(np.uint32), rstd1.view(np.uint32)) and np.all(mean1 == 0)
    if cols in lc.EXACT_COLS_TORCH:
        yt = F.elu(F.layer_norm(T(z), (cols,), T(gamma), T(beta), lc.EPS)).numpy()
        assert np.array_equal(y0.view(np.uint32), yt.view(np.uint32))


def test_model_matches_float64_on_generic_rows():
    """The numpy model is the law: on generic rows (both ELU branches) it sits inside the forward bar of the float64 reference."""
    inp, ref = lc.generic_case(5, 130)
    y, mean, rstd = lc.model_forward(*inp[:3])
    np.testing.assert_allclose(y, ref["y"], **lc.Y_BAR)
    np.testing.assert_allclose(mean, ref["mean"], rtol=lc.STAT_RTOL, atol=lc.MEAN_ATOL)
    np.testing.assert_allclose(rstd, ref["rstd"], rtol=lc.STAT_RTOL)


def test_near_constant_rows_orientation():
    """1000 + 0.01 U(-1, 1): what torch's fp32 CPU layer_norm and a purely sequential form of the law err by against float64 (the GPU
    test holds the kernel to 8x torch's error).  Both are far above the forward bar: the input, not the implementation, is the
    limit."""
    z, gamma, beta = lc.near_constant_rows()
    ref = F.elu(F.layer_norm(T(z).double(), (512,), T(gamma).double(), T(beta).double(), lc.EPS)).numpy()
    e_torch = np.abs(F.elu(F.layer_norm(T(z), (512,), T(gamma), T(beta), lc.EPS)).numpy() - ref).max()
    e_seq = np.abs(lc.model_forward(z, gamma, beta)[0] - ref).max()
    print(f"near-constant rows: torch fp32 CPU errs by {e_torch:.3g}, the sequential model by {e_seq:.3g}")
    assert 1e-4 < e_torch < 1e-1 and e_seq < 1e-1
