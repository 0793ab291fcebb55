"""pqlk_ln_res_forward / pqlk_ln_sum_backward (pql_amd/csrc/ln.hip) over the shape table of tests/layernorm_cases.py: every dispatch
seam and grid cap, the 16-byte and the scalar path, in the guarded, poisoned buffers of tests/row_harness.py (pad
columns of the inputs hold POISON too).  Float64 at layernorm_cases' bars where the input is generic; equality wherever the law
makes two calls the same chain of roundings (the ties to pqlk_ln_elu_backward, to the pre-added gradient, between aliased and
separate buffers, between the frozen and the full call) and on the exact design."""
import functools

import numpy as np
import pytest
import torch

import bronet_cases as bc
import layernorm_cases as lc
from guarded import Guarded, bits as _bits
from row_harness import _backward, _forward, _layout, _mat, _np, _pads_intact, _vec, backward, forward
from support import dev  # noqa: F401

pytestmark = pytest.mark.gpu

F32, POISON = np.float32, lc.POISON
E_NULL, E_SHAPE = 1, 2
BWD_SHAPES = [s for s in bc.SHAPES if s[1] >= 2]


def _res_forward(dev, z, gamma, beta, res, align):
    return forward(dev, "pqlk_ln_res_forward", z, gamma, beta, align, res=res)


def _sum_backward(dev, b, dy, dy2=None, act=True, dsum=True, params=True, alias_dz=False, alias_dsum=False):
    """pqlk_ln_sum_backward on a forward's buffers (act: hand the forward's y on, i.e. an ELU stands behind the norm).
    Returns guarded (dz, dsum, dgamma, dbeta, scratch); what was not asked for is None."""
    m, cols = dy.shape
    gdy, gdy2, gdz, gds, dg, db, sc = backward(dev, "pqlk_ln_sum_backward", b, dy, params=params, alias=alias_dz, summed=True, dy2=dy2, act=act,
                                               dsum=dsum, alias_dsum=alias_dsum)
    if not alias_dz:
        assert torch.equal(gdy.t[:, :cols].cpu(), lc.T(dy)) and _pads_intact(gdy, cols)           # inputs are left alone
    if gdy2 is not None and not alias_dsum:
        assert torch.equal(gdy2.t[:, :cols].cpu(), lc.T(dy2)) and _pads_intact(gdy2, cols)
    for g in (gdz, gds):
        assert g is None or _pads_intact(g, cols)
    for g in (dg, db, sc):
        assert g is None or g.intact()
    return gdz, gds, dg, db, sc


def _same(a, b, cols):
    """Bitwise equality of two backward results, output by output."""
    assert len(a) == len(b)
    for x, y in zip(a[:4], b[:4]):
        assert (x is None) == (y is None)
        if x is not None:
            assert torch.equal(x.t[:, :cols] if x.t.dim() == 2 else x.t, y.t[:, :cols] if y.t.dim() == 2 else y.t)


# =========================================================================== forward
@pytest.mark.parametrize("align", bc.ALIGN)
@pytest.mark.parametrize("shape", bc.SHAPES, ids=bc.shape_id)
def test_ln_res_forward_shapes(dev, shape, align):
    m, cols = shape
    (z, gamma, beta, _, res, _), ref, _ = bc.generic_case(m, cols)
    b = _res_forward(dev, z, gamma, beta, res, align)
    np.testing.assert_allclose(_np(b["y"], cols), ref["y"], **bc.Y_BAR)
    np.testing.assert_allclose(_np(b["mean"]), ref["mean"], rtol=bc.STAT_RTOL, atol=bc.MEAN_ATOL)
    np.testing.assert_allclose(_np(b["rstd"]), ref["rstd"], rtol=bc.STAT_RTOL)
    assert _pads_intact(b["y"], cols) and b["mean"].intact() and b["rstd"].intact()
    for name, a in (("z", z), ("res", res)):            # inputs unmodified, their poisoned pads and guards too
        assert np.array_equal(_bits(_np(b[name], cols)), _bits(a)) and _pads_intact(b[name], cols), name
    # mean and rstd are those of the LayerNorm + ELU entry on the same z, bit for bit: the same row sums
    e = _forward(dev, z, gamma, beta, align)
    assert torch.equal(e["mean"].t, b["mean"].t) and torch.equal(e["rstd"].t, b["rstd"].t)


@functools.lru_cache(maxsize=None)
def _exact_case(m, cols):
    z, gamma, beta = lc.exact_inputs(m, cols)
    res = bc.exact_res(m, cols)
    return (z, gamma, beta, res), bc.model_res_forward(z, gamma, beta, res, order="exact")


EXACT_SHAPES = [(m, c) for m, c in zip((bc.M_PAST_ROW_BLOCKS, bc.M_PAST_CHUNKS, 257), bc.EXACT_COLS)]


@pytest.mark.parametrize("align", bc.ALIGN)
@pytest.mark.parametrize("shape", EXACT_SHAPES, ids=bc.shape_id)
def test_ln_res_forward_exact_design(dev, shape, align):
    """Zero-sum integer rows, dyadic gamma, beta = 20, res in multiples of 1/4: y, mean and rstd are the bits of the op-by-op model."""
    m, cols = shape
    (z, gamma, beta, res), (y, mean, rstd) = _exact_case(m, cols)
    b = _res_forward(dev, z, gamma, beta, res, align)
    assert np.all(_np(b["mean"]) == 0) and np.all(mean == 0)
    assert np.array_equal(_bits(_np(b["rstd"])), _bits(rstd))
    assert np.array_equal(_bits(_np(b["y"], cols)), _bits(y))


# =========================================================================== backward: the ties, all bitwise
@pytest.mark.parametrize("align", bc.ALIGN)
@pytest.mark.parametrize("shape", bc.SHAPES, ids=bc.shape_id)
def test_ln_sum_backward_ties(dev, shape, align):
    m, cols = shape
    (z, gamma, beta, dy, _, dy2), _, _ = bc.generic_case(m, cols)
    b = _forward(dev, z, gamma, beta, align)                   # LayerNorm + ELU: y takes both signs
    # (1) one addend, y given: pqlk_ln_elu_backward
    gdz, dg, db, _ = _backward(dev, b, dy)
    one = _sum_backward(dev, b, dy, dsum=False)
    assert torch.equal(one[0].t[:, :cols], gdz.t[:, :cols]) and torch.equal(one[2].t, dg.t) and torch.equal(one[3].t, db.t)
    added = (dy + dy2).astype(F32)                             # fl32(dy + dy2): one rounding, numpy's is the kernel's
    for act in (True, False):
        # (2) two addends = the pre-added gradient, every output; (3) dsum is the fp32 sum
        full = _sum_backward(dev, b, dy, dy2, act=act)
        _same(full, _sum_backward(dev, b, added, None, act=act), cols)
        assert np.array_equal(_bits(_np(full[1], cols)), _bits(added))
        assert torch.equal(full[1].t[:, :cols], (lc.T(dy).to(dev) + lc.T(dy2).to(dev)))
        # (5) each permitted alias, and both at once
        for alias in (dict(alias_dz=True), dict(alias_dsum=True), dict(alias_dz=True, alias_dsum=True)):
            _same(full, _sum_backward(dev, b, dy, dy2, act=act, **alias), cols)
        # (6) frozen: the dz and dsum bits of the full call; it is handed nothing else to write
        frozen = _sum_backward(dev, b, dy, dy2, act=act, params=False)
        assert torch.equal(frozen[0].t[:, :cols], full[0].t[:, :cols]) and torch.equal(frozen[1].t[:, :cols], full[1].t[:, :cols])
        _same(frozen, _sum_backward(dev, b, dy, dy2, act=act, params=False, alias_dz=True, alias_dsum=True), cols)
    # dsum left out: the other outputs do not move
    no_dsum = _sum_backward(dev, b, dy, dy2, dsum=False)
    full = _sum_backward(dev, b, dy, dy2)
    assert torch.equal(no_dsum[0].t[:, :cols], full[0].t[:, :cols]) and torch.equal(no_dsum[2].t, full[2].t) and torch.equal(no_dsum[3].t, full[3].t)


@pytest.mark.parametrize("align", bc.ALIGN)
@pytest.mark.parametrize("shape", EXACT_SHAPES, ids=bc.shape_id)
def test_ln_sum_backward_without_y_is_with_y_where_every_y_is_positive(dev, shape, align):
    """(4) The exact design's beta = 20 makes every y > 0: the ELU factor is 1 and y = NULL gives the bits of y given.  With integer
    dy and dy2, dbeta is the integer column sum exactly."""
    m, cols = shape
    (z, gamma, beta, _), _ = _exact_case(m, cols)
    dy, dy2 = bc.exact_grads(m, cols)
    b = _forward(dev, z, gamma, beta, align)
    assert bool((b["y"].t[:, :cols] > 0).all())
    with_y, without = _sum_backward(dev, b, dy, dy2, act=True), _sum_backward(dev, b, dy, dy2, act=False)
    _same(with_y, without, cols)
    assert np.array_equal(_np(without[3]), (dy.astype(np.float64) + dy2).sum(0).astype(F32))
    assert np.array_equal(_np(without[1], cols), dy + dy2)


# =========================================================================== backward against float64
@pytest.mark.parametrize("align", bc.ALIGN)
@pytest.mark.parametrize("shape", BWD_SHAPES, ids=bc.shape_id)
def test_ln_sum_backward_shapes(dev, shape, align):
    """The no-activation path with two addends (a block's second half) against float64 autograd of `res + LayerNorm(z)`."""
    m, cols = shape
    (z, gamma, beta, dy, res, dy2), _, ref = bc.generic_case(m, cols)
    b = _res_forward(dev, z, gamma, beta, res, align)
    gdz, gds, dg, db, _ = _sum_backward(dev, b, dy, dy2, act=False)
    for name, got in (("dsum", _np(gds, cols)), ("dz", _np(gdz, cols)), ("dgamma", _np(dg)), ("dbeta", _np(db))):
        np.testing.assert_allclose(got, ref[name], rtol=bc.BWD_RTOL, atol=bc.bwd_atol(ref[name]), err_msg=name)


@pytest.mark.parametrize("align", bc.ALIGN)
@pytest.mark.parametrize("m", lc.M_SMALL)
def test_ln_sum_one_column(dev, m, align):
    """cols = 1: z - mean = 0 exactly, so y = res + beta to the bit; dz = 0 and dgamma = 0 exactly, dsum = dy + dy2, dbeta its sum."""
    (z, _, _, dy, res, dy2), _, _ = bc.generic_case(m, 1)
    gamma, beta = np.array([1.25], F32), np.array([0.3], F32)
    b = _res_forward(dev, z, gamma, beta, res, align)
    assert np.array_equal(_bits(_np(b["y"], 1)), _bits((res + beta[0]).astype(F32))) and np.all(_np(b["mean"]) == z[:, 0])
    gdz, gds, dg, db, _ = _sum_backward(dev, b, dy, dy2, act=False)
    assert np.all(_np(gdz, 1) == 0) and np.all(_np(dg) == 0) and np.array_equal(_np(gds, 1), (dy + dy2).astype(F32))
    g = dy[:, 0].astype(np.float64) + dy2[:, 0]
    np.testing.assert_allclose(_np(db)[0], g.sum(), rtol=bc.BWD_RTOL, atol=lc.BWD_ATOL_REL * np.abs(g).max())


@pytest.mark.parametrize("align", bc.ALIGN)
@pytest.mark.parametrize("shape", [(bc.M_PAST_CHUNKS, 130), (257, 1025)], ids=bc.shape_id)
def test_same_input_same_bits(dev, shape, align):
    m, cols = shape
    (z, gamma, beta, dy, res, dy2), _, _ = bc.generic_case(m, cols)
    runs = []
    for _ in range(2):
        b = _res_forward(dev, z, gamma, beta, res, align)
        runs.append((b["y"], *_sum_backward(dev, b, dy, dy2, act=False)[:4]))
    _same(runs[0][1:], runs[1][1:], cols)
    assert torch.equal(runs[0][0].t[:, :cols], runs[1][0].t[:, :cols])


# =========================================================================== errors: refused on the host, nothing is launched
@pytest.mark.parametrize("align", bc.ALIGN)
def test_refused_calls_write_nothing(dev, align):
    from pql_amd import _lib as L
    m, cols = 5, 130
    (z, gamma, beta, dy, res, dy2), _, _ = bc.generic_case(m, cols)
    ld, off = _layout(align, cols)
    g = {k: _mat(dev, a, ld, off) for k, a in dict(z=z, res=res, dy=dy, dy2=dy2).items()}
    g.update(gamma=_vec(dev, gamma, off), beta=_vec(dev, beta, off))
    out = {k: Guarded(dev, (m, ld), POISON, off=off) for k in ("y", "dz", "dsum")}
    out.update({k: Guarded(dev, (m,), POISON, off=off) for k in ("mean", "rstd")})
    out.update({k: Guarded(dev, (cols,), POISON, off=off) for k in ("dgamma", "dbeta")})
    out["scratch"] = Guarded(dev, (int(L.lib.pqlk_ln_scratch_floats(cols)),), POISON)
    st = L.stream(dev)
    ok_f = [g["z"].ptr, ld, m, cols, g["gamma"].ptr, g["beta"].ptr, lc.EPS, g["res"].ptr, out["y"].ptr, out["mean"].ptr, out["rstd"].ptr, st]
    for i in (0, 4, 5, 7, 8, 9, 10):
        a = list(ok_f); a[i] = None
        assert L.lib.pqlk_ln_res_forward(*a) == E_NULL, i
    for i, v in ((2, 0), (2, -1), (3, 0), (3, -4), (1, cols - 1)):
        a = list(ok_f); a[i] = v
        assert L.lib.pqlk_ln_res_forward(*a) == E_SHAPE, (i, v)
    # the backward needs a forward's mean / rstd only as addresses here: every call below is refused
    ok_b = [g["dy"].ptr, g["dy2"].ptr, None, g["z"].ptr, ld, m, cols, out["mean"].ptr, out["rstd"].ptr, g["gamma"].ptr, out["dsum"].ptr,
            out["dz"].ptr, out["dgamma"].ptr, out["dbeta"].ptr, out["scratch"].ptr, st]
    for i in (0, 3, 7, 8, 9, 11, 14):
        a = list(ok_b); a[i] = None
        assert L.lib.pqlk_ln_sum_backward(*a) == E_NULL, i
    for i, v in ((5, 0), (5, -1), (6, 0), (6, -4), (4, cols - 1)):
        a = list(ok_b); a[i] = v
        assert L.lib.pqlk_ln_sum_backward(*a) == E_SHAPE, (i, v)
    torch.cuda.synchronize()
    for k, o in out.items():
        assert o.intact() and bool((o.t == POISON).all()), k
