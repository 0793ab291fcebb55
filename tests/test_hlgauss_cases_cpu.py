"""tests/hlgauss_cases.py proved without a GPU: the float64 reference of the HL-Gauss law is a pmf and agrees with its torch autograd
form, the exact design has in fp32 arithmetic every property the GPU test's bitwise asserts rest on -- for every row of every case --
and the generic design puts y where it says and is covered by a finite bound."""
import math

import numpy as np
import pytest
import torch

import hlgauss_cases as hc

F32 = np.float32


# ------------------------------------------------------------------------------------------------ the reference
@pytest.mark.parametrize("K", hc.GENERIC_KS + [2, 5])
def test_reference_target_is_a_pmf(K):
    case = hc.generic_case(hc.GENERIC_B, K, 100 + K) if K > 5 else dict(hc.generic_case(64, 51, 7), K=K)
    if K <= 5:   # the same rewards on a coarse support
        rng = np.random.default_rng(K)
        case.update(logits=rng.standard_normal((2, 64, K)).astype(F32), logits_t=rng.standard_normal((2, 64, K)).astype(F32),
                    z=torch.linspace(hc.V_MIN, hc.V_MAX, K).numpy())
    ref = hc.ref_of(case)
    assert (ref["t"] >= 0.0).all() and np.abs(ref["t"].sum(axis=1) - 1.0).max() <= 1e-12
    assert ref["norm"].min() >= hc.NORM_FLOOR      # sigma_ratio = 0.75, y clamped into the support
    assert (ref["y"] >= hc.V_MIN).all() and (ref["y"] <= hc.V_MAX).all()


@pytest.mark.parametrize("K", [2, 5, 51, 256])
def test_normaliser_floor_at_the_default_sigma(K):
    """y on an end of the support is the worst case: c(u_K) - c(u_0) = erf(1 / (2 s sqrt 2)) + erf((K - 1/2) / (s sqrt 2)),
    2 x 0.7248 at K = 2 and 2 x 0.7475 from K = 5 on."""
    dz, inv, edges = hc.bins(hc.V_MIN, hc.V_MAX, K, hc.SIGMA)
    for y in (hc.V_MIN, hc.V_MAX, 0.0):
        c = hc.cdf((edges.astype(np.float64) - y) * float(inv))
        assert c[-1] - c[0] >= hc.NORM_FLOOR
    c = hc.cdf((edges.astype(np.float64) - hc.V_MIN) * float(inv))
    assert abs((c[-1] - c[0]) / 2.0 - (0.7248 if K == 2 else 0.7475)) < 1e-4


def test_saturation_is_what_a_correctly_rounded_erf_returns():
    assert float(F32(math.erf(4.0))) == 1.0 and float(F32(math.erf(-4.0))) == -1.0
    assert 0.0 < hc.SAT_JUMP < 2.0 ** -25
    assert (hc.cdf(np.array([4.0, 1e9, -4.0, -np.inf])) == [1.0, 1.0, -1.0, -1.0]).all()


@pytest.mark.parametrize("per", [False, True])
def test_reference_agrees_with_the_autograd_form(per):
    case = hc.generic_case(37, 51, 5, per=per)
    ref = hc.ref_of(case, per)
    t64 = lambda a: torch.from_numpy(np.asarray(a, np.float64))   # noqa: E731
    x = t64(case["logits"]).requires_grad_(True)
    args = (t64(case["logits_t"]), t64(case["rew"]), t64(case["done"]), t64(case["z"]), case["gamma_n"], case["v_min"], case["v_max"], case["sigma"])
    loss = hc.hl_torch(x, *args, wh=t64(ref["wh"]) if per else None)
    (grad,) = torch.autograd.grad(loss, x)
    assert abs(float(loss.detach()) - ref["loss"]) <= 1e-12 * ref["loss"]
    np.testing.assert_allclose(grad.numpy(), ref["dy"], rtol=0, atol=1e-14)
    np.testing.assert_allclose(hc.abs_td_torch(x.detach(), *args).numpy(), ref["abs_td"], rtol=0, atol=1e-12)
    t, _ = hc.hl_target_torch(*args)
    np.testing.assert_allclose(t.numpy(), ref["t"], rtol=0, atol=1e-13)   # (two float64 erf implementations)


# ------------------------------------------------------------------------------------------------ the exact design
def _fp32_law(case):
    """The law op by op in numpy fp32 (expf, logf and erff only where the design makes their value unambiguous)."""
    K, B = case["K"], case["B"]
    dz, inv, edges = hc.bins(case["v_min"], case["v_max"], K, case["sigma"])
    z = case["z"]
    assert np.exp(F32(hc.COLD)) == 0.0 and np.exp(F32(0.0)) == 1.0 and np.log(F32(1.0)) == 0.0
    pt = (case["logits_t"] == 0.0).astype(F32)       # expf(x - 0) / 1
    E = (pt * z).sum(axis=-1, dtype=F32)
    y = case["rew"] + ((F32(1.0) - case["done"]) * F32(case["gamma_n"])) * np.minimum(E[0], E[1])
    y = np.minimum(np.maximum(y, F32(case["v_min"])), F32(case["v_max"]))
    u = (edges[None] - y[:, None]) * inv
    assert u.dtype == F32
    return y, u, edges, dz


@pytest.mark.parametrize("per", [False, True])
@pytest.mark.parametrize("K", hc.EXACT_KS)
def test_exact_design_holds_on_every_row(K, per):
    B = 263
    case = hc.exact_case(B, K, per)
    v_min, v_max, _ = hc.exact_support(K)
    y, u, edges, dz = _fp32_law(case)
    dz64 = (v_max - v_min) / (K - 1)
    assert float(dz) == dz64 and (edges.astype(np.float64) == v_min + (np.arange(K + 1) - 0.5) * dz64).all()   # dyadic: exact
    assert hc.survives_fp32(v_min + dz64 * np.arange(K))
    # every row: y is the centre of bin j, every edge saturates, so t is exactly one-hot on j
    assert (y.astype(np.float64) == case["y"]).all()
    assert (np.abs(u) >= 7.07).all()
    c = np.where(u >= 4.0, F32(1.0), F32(-1.0))
    t = (c[:, 1:] - c[:, :-1]) / (c[:, -1:] - c[:, :1])
    assert (t == case["t"]).all() and (t.sum(axis=1) == 1.0).all() and (t[np.arange(B), case["j"]] == 1.0).all()
    # the closed form is the float64 law (whose softmax is one-hot up to exp(-200))
    ref = hc.ref_of(case, per)
    assert (ref["t"] == case["t"]).all()
    np.testing.assert_allclose(ref["dy"], case["dy"].astype(np.float64), rtol=0, atol=1e-9)
    np.testing.assert_allclose(ref["rows"], case["rows"], rtol=1e-12, atol=1e-70)
    np.testing.assert_allclose(ref["abs_td"], case["abs_td"].astype(np.float64), rtol=0, atol=1e-70)
    # dy in {-1/B, 0, +1/B} wh; every row loss 0 or 200 per net; integer partials
    g = (case["w"] * (F32(1.0) / F32(B))).astype(F32)
    for net in range(2):
        q = case["dy"][net] / g[:, None]
        assert np.isin(q, [-1.0, 0.0, 1.0]).all() and (q.sum(axis=1) == 0.0).all()
        assert ((np.abs(q).sum(axis=1) == 0.0) == (case["hot"][net] == case["j"])).all()
    per_net = case["rows"] / case["w"].astype(np.float64) / 200.0
    assert np.isin(per_net, [0.0, 1.0, 2.0]).all()
    assert (case["parts"] == np.round(case["parts"])).all() and case["parts"].sum() == case["rows"].sum()
    assert float(case["loss"]) == float(F32(F32(case["rows"].sum()) * (F32(1.0) / F32(B))))
    # the rows the design promises: terminal and not, rewards past both ends, net 1 smaller, hot logit on and off the target bin
    i = np.arange(B)
    assert set(case["done"]) == {0.0, 1.0} and set(case["place"]) == {0, 1, 2}
    past = case["place"] > 0
    raw = case["rew"].astype(np.float64) + (1.0 - case["done"]) * 0.5 * np.minimum(*case["z"][case["tgt_atoms"]].astype(np.float64))
    assert (raw[case["place"] == 1] < v_min).all() and (raw[case["place"] == 2] > v_max).all() and past.any()
    e = case["z"][case["tgt_atoms"]]
    assert (e[1] < e[0]).any() and (e[0] < e[1]).any() and (e[0] != e[1]).all()
    for net in range(2):
        on = case["hot"][net] == case["j"]
        assert on.any() and (~on).any()
    assert len({(a, b, c_, d, e_) for a, b, c_, d, e_ in zip(i % 2, case["place"], e[1] < e[0], *(case["hot"] == case["j"][None]))}) == hc.ROW_PERIOD


@pytest.mark.parametrize("B", hc.EXACT_B)
def test_exact_partials_follow_the_grid(B):
    """Row i belongs to wave i mod (4 blocks) and so to block (i mod (4 blocks)) // 4; past the cap a block has rows of two trips."""
    case = hc.exact_case(B, 5, True)
    blocks = hc.loss_blocks(B)
    assert len(case["parts"]) == blocks == min((B + 3) // 4, 1024)
    want = np.zeros(blocks)
    for i, r in enumerate(case["rows"]):
        want[(i % (4 * blocks)) // 4] += r
    assert (case["parts"] == want).all()
    if B == hc.B_PAST_CAP:
        assert B == 4 * 1024 + 7 and blocks == 1024


# ------------------------------------------------------------------------------------------------ the generic design
@pytest.mark.parametrize("K", hc.GENERIC_KS)
def test_generic_design_places_y_and_has_a_finite_bound(K):
    case = hc.generic_case(hc.GENERIC_B, K, 100 + K, per=True)
    ref = hc.ref_of(case, True)
    dz = (hc.V_MAX - hc.V_MIN) / (K - 1)
    y, kind = ref["y"], case["kind"]
    assert ((y[kind == 0] > hc.V_MIN) & (y[kind == 0] < hc.V_MAX)).all()
    assert ((y[kind == 1] - hc.V_MIN) <= dz + 1e-5).all() and ((hc.V_MAX - y[kind == 2]) <= dz + 1e-5).all()
    assert (y[kind == 3] == hc.V_MIN).all() and (y[kind == 4] == hc.V_MAX).all()
    assert set(case["done"]) == {0.0, 1.0}
    bound = hc.hl_bounds(ref, hc.loss_blocks(hc.GENERIC_B))
    for name in ("t", "dy", "abs_td"):
        assert np.isfinite(bound[name]).all() and (bound[name] > 0).all()
    # the bound is a bound on rounding, not a tolerance: far below the quantities themselves
    assert bound["t"].max() < 2e-3 and bound["loss"] < 1e-3 * ref["loss"] and bound["abs_td"].max() < 1e-3
    # a perturbation of y by the bound's own delta y moves the float64 target by less than the bound allows
    for sign in (1.0, -1.0):
        moved = hc.hl_ref(case["logits"], case["logits_t"], case["rew"].astype(np.float64) + sign * bound["d_y"], case["done"], case["z"],
                          case["gamma_n"], case["v_min"], case["v_max"], case["sigma"], case["w"], case["wmax"])
        assert (np.abs(moved["t"] - ref["t"]) <= bound["t"]).all() and (np.abs(moved["dy"] - ref["dy"]) <= bound["dy"]).all()
