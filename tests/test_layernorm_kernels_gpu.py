"""pqlk_ln_elu_forward / pqlk_ln_elu_backward (pql_amd/csrc/ln.hip) over the shape table of tests/layernorm_cases.py: every dispatch
seam and grid cap, the 16-byte and the scalar path, in the guarded, poisoned buffers of tests/row_harness.py (pad columns of the
inputs hold POISON too: an over-read moves a row sum by whole units, an over-write is seen).  Bars: those of the BatchNorm pair's
tests, named in layernorm_cases; equality where the design makes the result exact."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import layernorm_cases as lc
from row_harness import _backward, _forward, _np, _pads_intact
from support import dev  # noqa: F401

pytestmark = pytest.mark.gpu

T, F32 = lc.T, np.float32


# =========================================================================== forward
@pytest.mark.parametrize("align", lc.ALIGN)
@pytest.mark.parametrize("shape", lc.SHAPES, ids=lc.shape_id)
def test_ln_elu_forward_shapes(dev, shape, align):
    m, cols = shape
    (z, gamma, beta, _), ref = lc.generic_case(m, cols)
    b = _forward(dev, z, gamma, beta, align)
    np.testing.assert_allclose(_np(b["y"], cols), ref["y"], **lc.Y_BAR)
    np.testing.assert_allclose(_np(b["mean"]), ref["mean"], rtol=lc.STAT_RTOL, atol=lc.MEAN_ATOL)
    np.testing.assert_allclose(_np(b["rstd"]), ref["rstd"], rtol=lc.STAT_RTOL)
    assert _pads_intact(b["y"], cols) and b["mean"].intact() and b["rstd"].intact()


# =========================================================================== backward
@pytest.mark.parametrize("align", lc.ALIGN)
@pytest.mark.parametrize("shape", [s for s in lc.SHAPES if s[1] >= 2], ids=lc.shape_id)
def test_ln_elu_backward_shapes(dev, shape, align):
    m, cols = shape
    (z, gamma, beta, dy), ref = lc.generic_case(m, cols)
    b = _forward(dev, z, gamma, beta, align)
    gdz, dg, db, sc = _backward(dev, b, dy)
    for name, got in (("dz", _np(gdz, cols)), ("dgamma", _np(dg)), ("dbeta", _np(db))):
        np.testing.assert_allclose(got, ref[name], rtol=lc.BWD_RTOL, atol=lc.bwd_atol(ref[name]), err_msg=name)
    assert _pads_intact(gdz, cols) and dg.intact() and db.intact() and sc.intact()


@pytest.mark.parametrize("align", lc.ALIGN)
@pytest.mark.parametrize("shape", [(257, 130), (5, 1025)], ids=lc.shape_id)
def test_ln_elu_backward_alias_and_frozen(dev, shape, align):
    """dz aliased to dy gives the bits of the separate-buffer call; without parameter gradients dz has those bits too, and nothing
    else is written (the call gets NULL for dgamma, dbeta and scratch)."""
    m, cols = shape
    (z, gamma, beta, dy), ref = lc.generic_case(m, cols)
    b = _forward(dev, z, gamma, beta, align)
    sep, dg, db, _ = _backward(dev, b, dy)
    ali, dg2, db2, _ = _backward(dev, b, dy, alias=True)
    fro, *_ = _backward(dev, b, dy, params=False)
    assert torch.equal(sep.t[:, :cols], ali.t[:, :cols]) and torch.equal(dg.t, dg2.t) and torch.equal(db.t, db2.t)
    assert _pads_intact(ali, cols)
    assert torch.equal(sep.t[:, :cols], fro.t[:, :cols]) and _pads_intact(fro, cols)
    np.testing.assert_allclose(_np(fro, cols), ref["dz"], rtol=lc.BWD_RTOL, atol=lc.bwd_atol(ref["dz"]))


# =========================================================================== one column
@pytest.mark.parametrize("align", lc.ALIGN)
@pytest.mark.parametrize("m", lc.M_SMALL)
def test_ln_one_column(dev, m, align):
    """cols = 1: z - mean = 0 exactly, so y = elu(beta) to the bit, dz = 0 and dgamma = 0 exactly (the float64 reference is ~1e-17
    there: a relative bar would mean nothing); dbeta = sum of g."""
    z = lc.generic_inputs(m, 1)[0]
    dy = lc.generic_inputs(m, 1)[3]
    for beta_v in (0.3, -0.3):
        gamma, beta = np.array([1.25], F32), np.array([beta_v], F32)
        b = _forward(dev, z, gamma, beta, align)
        y = _np(b["y"], 1)
        assert np.all(_np(b["mean"]) == z[:, 0])
        if beta_v > 0:
            assert np.array_equal(y.view(np.uint32), np.full((m, 1), beta_v, F32).view(np.uint32))
        else:   # expm1f(beta): the device's own libm, so the same bits in every row and the value to fp32 precision
            assert np.all(y.view(np.uint32) == y.view(np.uint32)[0, 0])
            np.testing.assert_allclose(y[0, 0], np.expm1(np.float64(beta[0])), rtol=1e-6)
        gdz, dg, db, _ = _backward(dev, b, dy)
        assert np.all(_np(gdz, 1) == 0) and np.all(_np(dg) == 0)
        g = dy[:, 0].astype(np.float64) * (1.0 if beta_v > 0 else np.float64(y[0, 0]) + 1.0)
        np.testing.assert_allclose(_np(db)[0], g.sum(), rtol=lc.BWD_RTOL, atol=lc.BWD_ATOL_REL * np.abs(g).max())


# =========================================================================== exact design
@pytest.mark.parametrize("align", lc.ALIGN)
@pytest.mark.parametrize("shape", [(lc.M_PAST_ROW_BLOCKS, 64), (lc.M_PAST_CHUNKS, 130), (lc.M_PAST_CHUNKS, 1026)], ids=lc.shape_id)
def test_ln_exact_design(dev, shape, align):
    """Zero-sum integer rows: the forward's bits are those of the op-by-op numpy model of the law (mean, rstd and y); with integer
    dy and every y > 0, dbeta is the integer column sum exactly."""
    m, cols = shape
    z, gamma, beta = lc.exact_inputs(m, cols)
    y, mean, rstd = lc.model_forward(z, gamma, beta, order="exact")
    b = _forward(dev, z, gamma, beta, align)
    assert np.all(_np(b["mean"]) == 0)
    assert np.array_equal(_np(b["rstd"]).view(np.uint32), rstd.view(np.uint32))
    assert np.array_equal(_np(b["y"], cols).view(np.uint32), y.view(np.uint32))
    dy = (lc.dd.integers((m, cols), 99, 7) - 3).astype(F32)
    _, _, db, _ = _backward(dev, b, dy)
    assert np.array_equal(_np(db), dy.astype(np.float64).sum(0).astype(F32))


# =========================================================================== conditioning, determinism, NaN
def test_ln_near_constant_rows(dev, capsys):
    """Rows of 1000 + 0.01 U(-1, 1), 4 x 512: max error against float64 at most 8x that of torch's fp32 CPU layer_norm on the same rows
    (or the forward bar if that is larger) -- the margin of test_batch_moments_constant_and_offset_columns, for two summation trees of
    the same class of algorithm (two-pass, fp32).
    Measured on an MI355X: kernel 5.55e-3 (scalar path) / 7.66e-3 (16-byte path), torch fp32 CPU 8.68e-3."""
    z, gamma, beta = lc.near_constant_rows()
    zt, gt, bt = T(z), T(gamma), T(beta)
    ref = F.elu(F.layer_norm(zt.double(), (512,), gt.double(), bt.double(), lc.EPS)).numpy()
    e_torch = float(np.abs(F.elu(F.layer_norm(zt, (512,), gt, bt, lc.EPS)).numpy() - ref).max())
    for align in lc.ALIGN:
        b = _forward(dev, z, gamma, beta, align)
        e_kernel = float(np.abs(_np(b["y"], 512) - ref).max())
        with capsys.disabled():
            print(f"\nnear-constant rows ({align}): kernel max error {e_kernel:.3g}, torch fp32 CPU {e_torch:.3g}")
        bar = max(8.0 * e_torch, float((lc.Y_BAR["atol"] + lc.Y_BAR["rtol"] * np.abs(ref)).max()))
        assert e_kernel <= bar, (e_kernel, e_torch)


@pytest.mark.parametrize("align", lc.ALIGN)
@pytest.mark.parametrize("shape", [(lc.M_PAST_CHUNKS, 130), (257, 1025)], ids=lc.shape_id)
def test_ln_same_input_same_bits(dev, shape, align):
    m, cols = shape
    (z, gamma, beta, dy), _ = lc.generic_case(m, cols)
    runs = []
    for _ in range(2):
        b = _forward(dev, z, gamma, beta, align)
        gdz, dg, db, _ = _backward(dev, b, dy)
        runs.append((b["y"].t[:, :cols].clone(), gdz.t[:, :cols].clone(), dg.t.clone(), db.t.clone()))
    for a, c in zip(*runs):
        assert torch.equal(a, c)


@pytest.mark.parametrize("align", lc.ALIGN)
@pytest.mark.parametrize("cols", [130, 1025])
def test_ln_nan_stays_in_its_row(dev, cols, align):
    m = 5
    (z, gamma, beta, _), _ = lc.generic_case(m, cols)
    clean = _np(_forward(dev, z, gamma, beta, align)["y"], cols)
    bad = z.copy()
    bad[2, 7] = np.nan
    y = _np(_forward(dev, bad, gamma, beta, align)["y"], cols)
    assert np.isnan(y[2]).all()
    keep = [0, 1, 3, 4]
    assert np.array_equal(y[keep].view(np.uint32), clean[keep].view(np.uint32))
