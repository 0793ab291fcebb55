"""What tests/bronet_cases.py guarantees, proven without a GPU: torch's own fp32 CPU result stays inside the bars the GPU tests use
on every generic input (so the bars admit a correct fp32 implementation), the op-by-op model of the skip forward is the LayerNorm
model plus one addition and order-free on the exact design, and the torch twin has the documented keys and parameter count."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import bronet_cases as bc
import layernorm_cases as lc

F32 = np.float32
T = bc.T


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def test_shape_table_and_bars_are_layernorm_cases():
    assert bc.SHAPES is lc.SHAPES and bc.ALIGN is lc.ALIGN and bc.EXACT_COLS is lc.EXACT_COLS
    assert bc.Y_BAR is lc.Y_BAR and (bc.STAT_RTOL, bc.MEAN_ATOL, bc.BWD_RTOL) == (lc.STAT_RTOL, lc.MEAN_ATOL, lc.BWD_RTOL)
    assert bc.bwd_atol is lc.bwd_atol
    assert {(bc.M_PAST_CHUNKS, 130), (bc.M_PAST_CHUNKS, 1025), (bc.M_PAST_ROW_BLOCKS, 130)} <= set(bc.SHAPES)


def test_torch_fp32_cpu_stays_inside_the_bars():
    """torch's fp32 CPU `res + F.layer_norm` and the summed-gradient autograd against float64 on EVERY generic input: inside the
    forward bar and the backward bar, with room to spare."""
    worst = dict(y=0.0, bwd=0.0)
    for m, cols in bc.SHAPES:
        (z, gamma, beta, dy, res, dy2), fwd, bwd = bc.generic_case(m, cols)
        got = bc.res_reference(z, gamma, beta, res, dtype=torch.float32)
        frac = np.abs(got["y"] - fwd["y"]) / (bc.Y_BAR["atol"] + bc.Y_BAR["rtol"] * np.abs(fwd["y"]))
        worst["y"] = max(worst["y"], float(frac.max()))
        if bwd is None:
            continue
        got = bc.sum_reference(z, gamma, beta, dy, dy2, elu=False, dtype=torch.float32)
        for k in ("dsum", "dz", "dgamma", "dbeta"):
            frac = np.abs(got[k] - bwd[k]) / (bc.bwd_atol(bwd[k]) + bc.BWD_RTOL * np.abs(bwd[k]))
            worst["bwd"] = max(worst["bwd"], float(frac.max()))
    print(f"torch fp32 CPU uses at most {worst['y']:.3f} of the forward bar and {worst['bwd']:.4f} of the backward bar")
    assert worst["y"] < 0.5 and worst["bwd"] < 0.5


def test_generic_skip_and_addend_matter():
    """res and dy2 are of the size of what they are added to: dropping either moves the result by far more than a bar."""
    (z, gamma, beta, dy, res, dy2), fwd, bwd = bc.generic_case(5, 130)
    assert np.abs(res).mean() > 0.5 and np.abs(dy2).mean() > 0.25
    no_dy2 = bc.sum_reference(z, gamma, beta, dy, np.zeros_like(dy2), elu=False)
    assert np.abs(no_dy2["dz"] - bwd["dz"]).max() > 1e3 * bc.bwd_atol(bwd["dz"])


@pytest.mark.parametrize("cols", sorted(set(lc.EXACT_COLS + lc.EXACT_COLS_TORCH)))
def test_exact_design_model_is_layernorms_plus_one_addition(cols):
    """On the exact design the model's y is fl32(res + y of layernorm_cases.model_forward) bit for bit (ELU is the identity at
    beta = 20), in any summation order; and it is torch's fp32 CPU `res + layer_norm`."""
    m = 3
    z, gamma, beta = lc.exact_inputs(m, cols)
    res = bc.exact_res(m, cols)
    assert np.all(res * 4 == np.round(res * 4)) and np.abs(res).max() <= 2 and len(np.unique(res)) > 1
    t, mean0, rstd0 = lc.model_forward(z, gamma, beta)
    assert np.all(t > 0)
    y0, mean1, rstd1 = bc.model_res_forward(z, gamma, beta, res)
    assert np.array_equal(_bits(y0), _bits((res + t).astype(F32)))
    assert np.array_equal(_bits(mean0), _bits(mean1)) and np.array_equal(_bits(rstd0), _bits(rstd1))
    rs = np.random.RandomState(5)
    for order in (np.arange(cols)[::-1], rs.permutation(cols), "exact"):
        y1, _, rstd2 = bc.model_res_forward(z, gamma, beta, res, order=order)
        assert np.array_equal(_bits(y0), _bits(y1)) and np.array_equal(_bits(rstd0), _bits(rstd2))
    if cols in lc.EXACT_COLS_TORCH:
        yt = (T(res) + F.layer_norm(T(z), (cols,), T(gamma), T(beta), lc.EPS)).numpy()
        assert np.array_equal(_bits(y0), _bits(yt))


def test_model_matches_float64_on_generic_rows():
    (z, gamma, beta, _, res, _), fwd, _ = bc.generic_case(5, 130)
    y, mean, rstd = bc.model_res_forward(z, gamma, beta, res)
    np.testing.assert_allclose(y, fwd["y"], **bc.Y_BAR)
    np.testing.assert_allclose(mean, fwd["mean"], rtol=bc.STAT_RTOL, atol=bc.MEAN_ATOL)
    np.testing.assert_allclose(rstd, fwd["rstd"], rtol=bc.STAT_RTOL)


def test_exact_grads_sum_exactly():
    dy, dy2 = bc.exact_grads(257, 130)
    assert np.all(dy == np.round(dy)) and np.all(dy2 == np.round(dy2)) and np.abs(dy).max() <= 3 and np.abs(dy2).max() <= 3
    assert not np.array_equal(dy, dy2)
    assert np.array_equal((dy + dy2).astype(np.float64), dy.astype(np.float64) + dy2.astype(np.float64))


@pytest.mark.parametrize("in_dim,width,blocks", [(10, 64, 2), (10, 130, 0), (104, 512, 2)])
def test_twin_keys_count_and_state(in_dim, width, blocks):
    twin = bc.Twin(in_dim, width, blocks)
    keys = list(twin.state_dict().keys())
    want = []
    for n in (1, 2):
        pre = f"net_q{n}."
        want += [pre + "stem.0.weight", pre + "stem.0.bias", pre + "stem.1.weight", pre + "stem.1.bias"]
        for k in range(blocks):
            want += [f"{pre}blocks.{k}.{j}.{w}" for j in (0, 1, 3, 4) for w in ("weight", "bias")]
        want += [pre + "out.weight", pre + "out.bias"]
    assert keys == want
    assert sum(p.numel() for p in twin.parameters()) == bc.num_params(in_dim, width, blocks)
    st = bc.twin_state(in_dim, width, blocks, 7)
    twin.load_state_dict(st, strict=True)
    assert bool((st["net_q1.stem.1.weight"] >= 0.5).all()) and float(st["net_q1.stem.0.weight"].abs().max()) <= 1 / np.sqrt(in_dim)
    q1, q2 = twin(torch.zeros(3, in_dim))
    assert q1.shape == (3, 1) and not torch.equal(q1, q2)
