"""pqlk_drop_mask / pqlk_drop_ln_elu_forward / pqlk_drop_ln_elu_backward (pql_amd/csrc/ln.hip) over the shape table of
tests/droq_cases.py: the mask against the numpy model of the law bit for bit, the p = 0 tie to pqlk_ln_elu_* bit for bit, p > 0 against
float64 on u at the bars of tests/layernorm_cases.py, in the guarded, poisoned buffers of tests/row_harness.py."""
import numpy as np
import pytest
import torch

import droq_cases as dc
import layernorm_cases as lc
from guarded import Guarded, bits as _bits
from row_harness import _backward, _forward, _np, _pads_intact, backward, forward
from support import dev  # noqa: F401

pytestmark = pytest.mark.gpu

F32, POISON = np.float32, lc.POISON
E_NULL, E_SHAPE = 1, 2
TAG = dc.TAGS[1]          # the tag of droq_cases.drop_case's references


def _drop_forward(dev, z, gamma, beta, align, p, tag=TAG, seed=dc.SEED):
    return forward(dev, "pqlk_drop_ln_elu_forward", z, gamma, beta, align, extras=(p, seed, tag), p=p, tag=tag, seed=seed)


def _drop_backward(dev, b, dy, params=True, alias=False):
    """As row_harness._backward, through the dropout entry with the forward's (p, seed, tag)."""
    _, _, gdz, _, dg, db, sc = backward(dev, "pqlk_drop_ln_elu_backward", b, dy, extras=(b["p"], b["seed"], b["tag"]), params=params, alias=alias)
    return gdz, dg, db, sc


# =========================================================================== the mask
@pytest.mark.parametrize("p", dc.P)
@pytest.mark.parametrize("shape", dc.MASK_SHAPES, ids=lc.shape_id)
def test_drop_mask_is_the_laws(dev, shape, p):
    from pql_amd import _lib as L
    m, cols = shape
    for tag, ldk in zip(dc.TAGS, (cols, cols + 5)):
        g = Guarded(dev, (m, ldk), 7, dtype=torch.uint8)
        L.check(L.lib.pqlk_drop_mask(dc.SEED, tag, p, m, cols, g.ptr, ldk, L.stream(dev)))
        torch.cuda.synchronize()
        got = g.t.cpu().numpy()
        assert np.array_equal(got[:, :cols], dc.keep_mask(dc.SEED, tag, p, m, cols).astype(np.uint8)), hex(tag)
        assert g.intact() and bool((got[:, cols:] == 7).all())


def test_numpy_philox_is_torchs_device_generator(dev):
    """The model of droq_cases against torch.randint on a seeded device generator, by the mapping in pql_amd/csrc/philox.hip's header:
    element li of a draw of n <= 256 * blocks values is component 0 of the first block of subsequence li past the offset -- key = the
    seed, counter = (offset / 4 low, offset / 4 high, li low, li high) -- modulo the range."""
    n, rng, seed = 1000, (1 << 28) - 57, 0x1234567887654321
    for off in (0, 8):
        g = torch.Generator(device=dev); g.manual_seed(seed); g.set_offset(off)
        want = torch.randint(rng, (n,), generator=g, device=dev).cpu().numpy()
        x = dc.philox4x32_10((seed & dc.MASK32, seed >> 32), (off // 4, 0, np.arange(n), 0))[0]
        assert np.array_equal(x.astype(np.int64) % rng, want)


# =========================================================================== p = 0: the bits of the plain entries
@pytest.mark.parametrize("align", lc.ALIGN)
@pytest.mark.parametrize("shape", dc.MASK_SHAPES, ids=lc.shape_id)
def test_p_zero_is_the_plain_layernorm_bit_for_bit(dev, shape, align):
    m, cols = shape
    z, gamma, beta, dy = lc.generic_inputs(m, cols)
    a, b = _forward(dev, z, gamma, beta, align), _drop_forward(dev, z, gamma, beta, align, 0.0)
    for k in ("y", "mean", "rstd"):
        assert torch.equal(a[k].t.view(torch.int32), b[k].t.view(torch.int32)), k     # (pad columns: POISON on both sides)
    assert _pads_intact(b["y"], cols) and b["mean"].intact() and b["rstd"].intact()
    for kw in (dict(), dict(alias=True), dict(params=False)):
        ra, rb = _backward(dev, a, dy, **kw), _drop_backward(dev, b, dy, **kw)
        assert torch.equal(ra[0].t.view(torch.int32), rb[0].t.view(torch.int32)), ("dz", kw)
        assert _pads_intact(rb[0], cols)
        if kw.get("params", True):
            assert torch.equal(ra[1].t.view(torch.int32), rb[1].t.view(torch.int32)), ("dgamma", kw)
            assert torch.equal(ra[2].t.view(torch.int32), rb[2].t.view(torch.int32)), ("dbeta", kw)
            assert rb[1].intact() and rb[2].intact() and rb[3].intact()


# =========================================================================== p > 0: float64 on u
@pytest.mark.parametrize("align", lc.ALIGN)
@pytest.mark.parametrize("case", dc.fwd_cases(), ids=dc.case_id)
def test_drop_forward_shapes(dev, case, align):
    (m, cols), p = case
    (z, gamma, beta, _), keep, u, ref = dc.drop_case(m, cols, p)
    b = _drop_forward(dev, z, gamma, beta, align, p)
    y = _np(b["y"], cols)
    np.testing.assert_allclose(y, ref["y"], **lc.Y_BAR)
    np.testing.assert_allclose(_np(b["mean"]), ref["mean"], rtol=lc.STAT_RTOL, atol=lc.MEAN_ATOL)
    np.testing.assert_allclose(_np(b["rstd"]), ref["rstd"], rtol=lc.STAT_RTOL)
    assert _pads_intact(b["y"], cols) and b["mean"].intact() and b["rstd"].intact()
    # a row with nothing kept, and any one-column row: u - mean = 0 exactly, so y = elu(beta_j) to the bit -- beta_j itself where it is
    # positive, the device's expm1f(beta_j), the same in every such row, elsewhere
    flat = ~keep.any(1) if cols > 1 else np.ones(m, bool)
    if flat.any():
        rows = y[flat]
        assert np.all(_np(b["mean"])[flat] == (u[flat, 0] if cols == 1 else 0))
        assert np.array_equal(_bits(rows[:, beta > 0]), _bits(np.broadcast_to(beta[beta > 0], rows[:, beta > 0].shape)))
        assert np.all(_bits(rows) == _bits(rows[:1]))


@pytest.mark.parametrize("align", lc.ALIGN)
@pytest.mark.parametrize("case", dc.bwd_cases(), ids=dc.case_id)
def test_drop_backward_shapes(dev, case, align):
    (m, cols), p = case
    (z, gamma, beta, dy), keep, _, ref = dc.drop_case(m, cols, p)
    b = _drop_forward(dev, z, gamma, beta, align, p)
    gdz, dg, db, sc = _drop_backward(dev, b, dy)
    dz = _np(gdz, cols)
    for name, got in (("dz", dz), ("dgamma", _np(dg)), ("dbeta", _np(db))):
        np.testing.assert_allclose(got, ref[name], rtol=lc.BWD_RTOL, atol=lc.bwd_atol(ref[name]), err_msg=name)
    assert np.all(_bits(dz)[~keep] == 0)          # a dropped column's dz is +0.0f
    assert _pads_intact(gdz, cols) and dg.intact() and db.intact() and sc.intact()


@pytest.mark.parametrize("align", lc.ALIGN)
@pytest.mark.parametrize("p", dc.P[1:])
@pytest.mark.parametrize("m", dc.M_SMALL)
def test_drop_one_column(dev, m, p, align):
    """cols = 1: u - mean = 0 whether the unit is kept or not: dz and dgamma are exactly 0 (dz +0.0f where dropped), dbeta = sum of g."""
    (z, gamma, beta, dy), keep, _, _ = dc.drop_case(m, 1, p)
    b = _drop_forward(dev, z, gamma, beta, align, p)
    gdz, dg, db, _ = _drop_backward(dev, b, dy)
    dz, y = _np(gdz, 1), _np(b["y"], 1).astype(np.float64)
    assert np.all(dz == 0) and np.all(_bits(dz)[~keep] == 0) and np.all(_np(dg) == 0)
    g = dy[:, 0].astype(np.float64) * np.where(y[:, 0] > 0, 1.0, y[:, 0] + 1.0)
    np.testing.assert_allclose(_np(db)[0], g.sum(), rtol=lc.BWD_RTOL, atol=lc.BWD_ATOL_REL * np.abs(g).max())


@pytest.mark.parametrize("align", lc.ALIGN)
@pytest.mark.parametrize("p", dc.P[1:])
@pytest.mark.parametrize("shape", [(257, 130), (5, 1025), (5, 33)], ids=lc.shape_id)
def test_drop_backward_alias_and_frozen(dev, shape, p, align):
    """dz aliased to dy gives the bits of the separate-buffer call; with dgamma = dbeta = scratch = NULL dz has those bits too."""
    m, cols = shape
    (z, gamma, beta, dy), keep, _, ref = dc.drop_case(m, cols, p)
    b = _drop_forward(dev, z, gamma, beta, align, p)
    sep, dg, db, _ = _drop_backward(dev, b, dy)
    ali, dg2, db2, _ = _drop_backward(dev, b, dy, alias=True)
    fro, *_ = _drop_backward(dev, b, dy, params=False)
    assert torch.equal(sep.t[:, :cols], ali.t[:, :cols]) and torch.equal(dg.t, dg2.t) and torch.equal(db.t, db2.t)
    assert _pads_intact(ali, cols)
    assert torch.equal(sep.t[:, :cols], fro.t[:, :cols]) and _pads_intact(fro, cols)
    np.testing.assert_allclose(_np(fro, cols), ref["dz"], rtol=lc.BWD_RTOL, atol=lc.bwd_atol(ref["dz"]))
    assert np.all(_bits(_np(ali, cols))[~keep] == 0)


@pytest.mark.parametrize("align", lc.ALIGN)
@pytest.mark.parametrize("shape", [(lc.M_PAST_CHUNKS, 130), (257, 1025)], ids=lc.shape_id)
def test_drop_same_input_same_bits_and_tags_differ(dev, shape, align):
    m, cols = shape
    z, gamma, beta, dy = lc.generic_inputs(m, cols)
    runs = []
    for tag in (dc.TAGS[1], dc.TAGS[1], dc.TAGS[0]):
        b = _drop_forward(dev, z, gamma, beta, align, 0.5, tag=tag)
        gdz, dg, db, _ = _drop_backward(dev, b, dy)
        runs.append((b["y"].t[:, :cols].clone(), gdz.t[:, :cols].clone(), dg.t.clone(), db.t.clone()))
    for a, c in zip(runs[0], runs[1]):
        assert torch.equal(a, c)
    assert not torch.equal(runs[0][0], runs[2][0])


def test_error_codes_before_any_launch(dev):
    """A bad p or shape returns its code and launches nothing: the poisoned outputs are untouched."""
    from pql_amd import _lib as L
    z, gamma, beta, dy = lc.generic_inputs(5, 33)
    b = _drop_forward(dev, z, gamma, beta, "vector", 0.5)
    y0 = b["y"].t.clone()
    args = lambda p, m=5, cols=33: (b["z"].ptr, b["ld"], m, cols, b["gamma"].ptr, b["beta"].ptr, lc.EPS, p, 1, 2, b["y"].ptr,  # noqa: E731
                                    b["mean"].ptr, b["rstd"].ptr, L.stream(dev))
    for bad in (-0.5, 1.0, 2.0, float("nan"), float("inf")):
        assert L.lib.pqlk_drop_ln_elu_forward(*args(bad)) == E_SHAPE
        assert L.lib.pqlk_drop_mask(1, 2, bad, 5, 33, b["y"].ptr, 33, L.stream(dev)) == E_SHAPE
        assert L.lib.pqlk_drop_ln_elu_backward(b["z"].ptr, b["y"].ptr, b["z"].ptr, b["ld"], 5, 33, b["mean"].ptr, b["rstd"].ptr, b["gamma"].ptr,
                                               bad, 1, 2, b["y"].ptr, None, None, None, L.stream(dev)) == E_SHAPE
    assert L.lib.pqlk_drop_ln_elu_forward(*args(0.5, m=2 ** 32 + 1)) == E_SHAPE
    assert L.lib.pqlk_drop_ln_elu_forward(*args(0.5, m=0)) == E_SHAPE
    assert L.lib.pqlk_drop_ln_elu_forward(*args(0.5, cols=b["ld"] + 1)) == E_SHAPE
    a = list(args(0.5)); a[10] = None
    assert L.lib.pqlk_drop_ln_elu_forward(*a) == E_NULL
    torch.cuda.synchronize()
    assert torch.equal(b["y"].t.view(torch.int32), y0.view(torch.int32)) and b["y"].intact()
