"""The coloured exploration noise without a GPU: the tables against the NumPy model's bits, the configuration refusals, which agents
take a colour, the host argument errors of pqlk_action_noise_colored, and the statistics and the reset rule of the model itself."""
import os
import re

import numpy as np
import pytest
import torch

import colored_noise_model as M
from support import bits, cfg_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_NULL, E_SHAPE, E_RANGE = 1, 2, 3
F = np.float32


def _spec(*extra, algo="pql_algo"):
    from pql_amd.utils.noise import noise_color
    return noise_color(cfg_of(algo, *extra))


# --------------------------------------------------------------------------- tables
@pytest.mark.parametrize("extra", [(), ("algo.noise.corr_groups=1",), ("algo.noise.corr_groups=5", "algo.noise.corr_min=0.3", "algo.noise.corr_max=0.9"),
                                   ("algo.noise.corr_min=0.0", "algo.noise.corr_max=0.0", "algo.noise.corr_groups=2"),
                                   ("algo.noise.corr_groups=7", "algo.noise.corr_max=0.999")])
def test_ar1_tables_are_the_models_bits(extra):
    """Group counts up to the default 8: the model states torch.linspace's element-wise fp32 formula.  From 16 values on torch fills
    whole vectors from a per-vector base, in an order that depends on the host's vector width, which no model can pin."""
    from pql_amd.utils.noise import color_tables
    spec = _spec("algo.noise.color=ar1", *extra)
    assert spec.octaves == 1 and spec.color == "ar1"
    rho, coef, w = color_tables(spec)
    mr, mc, mw = M.tables("ar1", groups=spec.groups, corr_min=spec.corr_min, corr_max=spec.corr_max)
    assert rho.dtype == coef.dtype == torch.float32 and tuple(rho.shape) == tuple(coef.shape) == (spec.groups, 1)
    assert np.array_equal(bits(rho.numpy()), bits(mr)) and np.array_equal(bits(coef.numpy()), bits(mc))
    assert w == 1.0 and mw == F(1.0)
    _unit_variance(rho.numpy(), coef.numpy())


@pytest.mark.parametrize("octaves", [1, 2, 6, 8])
def test_pink_tables_are_the_models_bits_and_exact_dyadics(octaves):
    from pql_amd.utils.noise import color_tables
    spec = _spec("algo.noise.color=pink", f"algo.noise.octaves={octaves}")
    assert (spec.groups, spec.octaves) == (1, octaves)
    rho, coef, w = color_tables(spec)
    mr, mc, mw = M.tables("pink", octaves=octaves)
    assert np.array_equal(bits(rho.numpy()), bits(mr)) and np.array_equal(bits(coef.numpy()), bits(mc))
    assert np.array_equal(bits(np.array([w], dtype=F)), bits(np.array([mw]))) and F(w) == w
    r = rho.numpy().astype(np.float64)[0]
    assert r[0] == 0.0 and all(r[k] == 1.0 - 2.0 ** -k for k in range(1, octaves))   # exact, not rounded
    assert all(float(x * 2 ** k).is_integer() for k, x in enumerate(r))
    assert abs(float(w) ** 2 * octaves - 1.0) <= 2.0 ** -23
    _unit_variance(rho.numpy(), coef.numpy())


def _unit_variance(rho, coef):
    """coef^2 + rho^2 = 1 up to the rounding of coef to fp32: |d(coef^2)| <= 2 coef * (coef * 2^-24) <= 2^-23, and the float64
    evaluation in front of it adds less than 2^-50."""
    r, c = rho.astype(np.float64), coef.astype(np.float64)
    assert np.all(np.abs(c * c + r * r - 1.0) <= 2.0 ** -23 + 2.0 ** -50)


# --------------------------------------------------------------------------- refusals
@pytest.mark.parametrize("extra, key", [
    (("algo.noise.color=brown",), r"algo\.noise\.color"),
    (("algo.noise.color=None",), r"algo\.noise\.color"),
    (("algo.noise.corr_min=-0.1",), r"algo\.noise\.corr_min"),
    (("algo.noise.corr_min=1.0", "algo.noise.corr_max=1.0"), r"algo\.noise\.corr_min"),
    (("algo.noise.corr_max=1.0",), r"algo\.noise\.corr_max"),
    (("algo.noise.corr_max=-0.5",), r"algo\.noise\.corr_max"),
    (("algo.noise.corr_max=high",), r"algo\.noise\.corr_max"),
    (("algo.noise.corr_min=0.6", "algo.noise.corr_max=0.5"), r"algo\.noise\.corr_min.*algo\.noise\.corr_max"),
    (("algo.noise.octaves=0",), r"algo\.noise\.octaves"),
    (("algo.noise.octaves=9",), r"algo\.noise\.octaves"),
    (("algo.noise.octaves=2.5",), r"algo\.noise\.octaves"),
    (("algo.noise.corr_groups=0",), r"algo\.noise\.corr_groups"),
    (("algo.noise.corr_groups=-3",), r"algo\.noise\.corr_groups"),
    (("algo.noise.corr_groups=True",), r"algo\.noise\.corr_groups"),
])
@pytest.mark.parametrize("color", ["ar1", "pink"])
def test_config_refusals_name_the_key(extra, key, color):
    extra = extra if any(e.startswith("algo.noise.color=") for e in extra) else (f"algo.noise.color={color}", *extra)
    with pytest.raises(ValueError, match=key):
        _spec(*extra)


AGENTS = {"sac_algo": ("pql_amd.algo.sac", "AgentSAC"), "droq_algo": ("pql_amd.algo.sac", "AgentSAC"), "tqc_algo": ("pql_amd.algo.tqc", "AgentTQC"),
          "ppo_algo": ("pql_amd.algo.ppo", "AgentPPO"), "ddpg_algo": ("pql_amd.algo.ddpg", "AgentDDPG"),
          "crossq_algo": ("pql_amd.algo.crossq", "AgentCrossQ"), "pql_algo": ("pql_amd.algo.pql_actor", "PQLActor")}


def _construct(algo, cfg):
    import importlib
    mod, cls = AGENTS[algo]
    return getattr(importlib.import_module(mod), cls)(None, cfg)   # env = None: nothing may be touched before the refusal


def _colored_cfg(algo, color):
    from pql_amd.utils.cfg import Cfg
    cfg = cfg_of(algo)
    if "noise" in cfg.algo:
        cfg.algo.noise.color = color
    else:   # ppo_algo has no noise node of its own
        cfg.algo.noise = Cfg(color=color)
    return cfg


@pytest.mark.parametrize("color", ["ar1", "pink"])
@pytest.mark.parametrize("algo", ["sac_algo", "droq_algo", "tqc_algo", "ppo_algo"])
def test_agents_that_sample_their_own_policy_refuse_a_colour(algo, color):
    with pytest.raises(ValueError, match=rf"algo\.noise\.color={color}.*pql_algo.*ddpg_algo.*crossq_algo"):
        _construct(algo, _colored_cfg(algo, color))


@pytest.mark.parametrize("color", ["ar1", "pink"])
@pytest.mark.parametrize("algo", ["ddpg_algo", "crossq_algo", "pql_algo"])
def test_the_deterministic_policy_agents_accept_a_colour(algo, color):
    """The check passes (-> the law's spec), and the constructor gets past it: with env = None it stops at the env, not at a
    refusal."""
    from pql_amd.utils.noise import noise_color
    cfg = _colored_cfg(algo, color)
    spec = noise_color(cfg)
    assert spec is not None and spec.color == color and (spec.groups, spec.octaves) == ((8, 1) if color == "ar1" else (1, 6))
    with pytest.raises(AttributeError, match="observation_space"):
        _construct(algo, cfg)


@pytest.mark.parametrize("algo", sorted(AGENTS))
def test_white_and_a_config_without_the_keys_are_the_same_nothing(algo):
    from pql_amd.utils.noise import noise_color
    cfg = cfg_of(algo)
    assert noise_color(cfg) is None
    if "noise" in cfg.algo:
        assert cfg.algo.noise.color == "white"
        for k in ("color", "corr_min", "corr_max", "corr_groups", "octaves"):
            del cfg.algo.noise[k]
        assert noise_color(cfg) is None
        cfg.algo.noise.color = "ar1"   # the other keys still missing: their defaults
        if algo in ("ddpg_algo", "crossq_algo", "pql_algo"):
            assert tuple(noise_color(cfg)) == ("ar1", 8, 1, 0.0, 0.95)


def test_the_yaml_documents_the_keys_and_defaults_to_white():
    text = open(os.path.join(ROOT, "pql_amd", "cfg", "algo", "off_policy.yaml")).read()
    for key in ("color", "corr_min", "corr_max", "corr_groups", "octaves"):
        assert re.search(rf"#.*\b{key}\b", text), key
    n = cfg_of("pql_algo").algo.noise
    assert (n.color, n.corr_min, n.corr_max, n.corr_groups, n.octaves) == ("white", 0.0, 0.95, 8, 6)


# --------------------------------------------------------------------------- the entry's host checks
def test_prototype_declared_and_bound():
    import ctypes as C
    from pql_amd import _lib as L
    P, I32, I64, Fl = C.c_void_p, C.c_int32, C.c_int64, C.c_float
    assert L.PROTOTYPES["pqlk_action_noise_colored"] == (C.c_int, [P, P, P, Fl, P, P, I32, I32, I64, P, P, I64, I32, Fl, Fl, Fl, P, P])
    assert hasattr(L.lib, "pqlk_action_noise_colored") and L.NOISE_MAX_OCTAVES == 8


def test_host_argument_errors():
    """NULL pointers, rows <= 0, cols <= 0, octaves 0 and 9, groups 0, a negative env_offset and out inside state are refused on the
    host, before any launch (so this runs without a GPU)."""
    from pql_amd import _lib as L
    bufs = [torch.zeros(64) for _ in range(8)]      # valid, distinct host addresses: never dereferenced
    act, draw, std, rho, coef, fresh, state, out = (L.ptr(b) for b in bufs)
    fn = L.lib.pqlk_action_noise_colored
    # act draw std_rows std_scalar rho coef groups octaves env_offset fresh state rows cols w lo hi out stream
    ok = [act, draw, std, 0.5, rho, coef, 2, 1, 0, fresh, state, 4, 2, 1.0, -1.0, 1.0, out, None]
    for i in (0, 1, 4, 5, 9, 10, 16):
        a = list(ok); a[i] = None
        assert fn(*a) == E_NULL, i
    for i, v in ((11, 0), (11, -1), (12, 0), (12, -4), (7, 0), (7, 9), (7, -1), (6, 0), (6, -2), (8, -1)):
        a = list(ok); a[i] = v
        assert fn(*a) == E_SHAPE, (i, v)
        a[2] = None                                  # with the scalar sigma alike
        assert fn(*a) == E_SHAPE, (i, v)
    a = list(ok); a[14], a[15] = 1.0, -1.0
    assert fn(*a) == E_SHAPE                         # lo > hi
    a = list(ok); a[16] = state
    assert fn(*a) == E_RANGE                         # out may not alias state


# --------------------------------------------------------------------------- the model's statistics
STAT_STEPS, STAT_ELEMS, BURN_IN = 4096, 256, 512


def _series(rho, coef, w, seed):
    """n of the model over STAT_STEPS steps x STAT_ELEMS elements (act = 0, sigma = 1, bounds wide open): (steps, elements)."""
    R = rho.shape[1]
    rng = np.random.default_rng(seed)
    rows, cols = 16, STAT_ELEMS // 16
    state = np.zeros((rows, R, cols), dtype=F)
    zero, none = np.zeros((rows, cols), dtype=F), np.zeros(rows, dtype=np.uint8)
    out = np.empty((STAT_STEPS, rows * cols), dtype=F)
    for t in range(STAT_STEPS):
        draw = rng.standard_normal((rows, R * cols)).astype(F)
        n, state = M.step(zero, draw, F(1.0), rho, coef, w, 0, np.ones(rows, dtype=np.uint8) if t == 0 else none, state, lo=-1e30, hi=1e30)
        out[t] = n.reshape(-1)
    return out[BURN_IN:].astype(np.float64)


@pytest.mark.parametrize("r", [0.0, 0.5, 0.95])
def test_ar1_model_has_unit_variance_and_lag_one_correlation_rho(r):
    """Effective sample count = samples * (1 - rho) / (1 + rho) (the variance inflation of an AR(1) mean), samples = 3584 steps x 256
    elements.  A variance estimate of a unit Gaussian has standard error ~ sqrt(2 / n_eff) and a correlation estimate ~ 1 / sqrt(n_eff)
    or less, so 5 / sqrt(n_eff) is at least 3.5 standard errors: a condition on the law, not a measurement of it."""
    rho, coef, w = M.tables("ar1", groups=1, corr_min=r, corr_max=r)
    x = _series(rho, coef, w, seed=20 + int(100 * r))
    n_eff = x.size * (1.0 - r) / (1.0 + r)
    bound = 5.0 / np.sqrt(n_eff)
    var = x.var()
    lag1 = np.mean((x[1:] - x.mean()) * (x[:-1] - x.mean())) / var
    print(f"rho {r}: var {var:.5f} lag1 {lag1:.5f} bound {bound:.5f} n_eff {n_eff:.0f}")
    assert abs(var - 1.0) <= bound and abs(lag1 - float(rho[0, 0])) <= bound


def test_pink_model_has_unit_variance():
    """Six octaves: the slowest process has rho = 1 - 2^-5, which sets the effective sample count of the sum from below."""
    rho, coef, w = M.tables("pink", octaves=6)
    x = _series(rho, coef, w, seed=77)
    r = float(rho[0, -1])
    n_eff = x.size * (1.0 - r) / (1.0 + r)
    bound = 5.0 / np.sqrt(n_eff)
    print(f"pink: var {x.var():.5f} bound {bound:.5f} n_eff {n_eff:.0f}")
    assert abs(x.var() - 1.0) <= bound
    lag1 = np.mean((x[1:] - x.mean()) * (x[:-1] - x.mean())) / x.var()
    expect = float(np.mean(rho.astype(np.float64)))   # the mean of the octaves' coefficients
    assert abs(lag1 - expect) <= bound


# --------------------------------------------------------------------------- reset
@pytest.mark.parametrize("color, R, G", [("ar1", 1, 4), ("pink", 6, 1)])
def test_a_fresh_row_takes_the_draw_exactly(color, R, G):
    rho, coef, w = M.tables(color, groups=G, octaves=R)
    rows, cols = 9, 3
    rng = np.random.default_rng(5)
    state = rng.standard_normal((rows, R, cols)).astype(F)
    draw = rng.standard_normal((rows, R * cols)).astype(F)
    fresh = np.array([1, 0, 0, 1, 1, 0, 1, 0, 0], dtype=np.uint8)
    _, new = M.step(np.zeros((rows, cols), dtype=F), draw, F(0.3), rho, coef, w, 2, fresh, state)
    on = fresh != 0
    assert np.array_equal(bits(new[on]), bits(draw.reshape(rows, R, cols)[on]))
    assert not np.array_equal(new[~on], draw.reshape(rows, R, cols)[~on])
    if color == "pink":   # octave 0 has rho = 0, coef = 1: white whether fresh or not
        assert np.array_equal(bits(new[:, 0]), bits(draw.reshape(rows, R, cols)[:, 0]))
