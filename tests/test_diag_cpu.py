"""The critic diagnostics' host side, without a GPU: the two entries in the ABI, their refusals before any launch, the rules of
`algo.diag` (pql_amd/algo/diag.py), the keys' absence from a checkpoint's structure, and the probe's call arguments and decoding."""
import ctypes as C

import numpy as np
import pytest
import torch

import diag_cases as dc
from pql_amd import _lib as L
from pql_amd.algo.diag import OUT_OF_SCOPE, STAT_KEYS, UNIT_KEYS, diag_cfg, log_keys
from support import cfg_of

ON = "algo.diag.enabled=True"


def test_the_abi_declares_both_entries_and_their_constants():
    p, f, i32, i64 = C.c_void_p, C.c_float, C.c_int32, C.c_int64
    assert L.PROTOTYPES["pqlk_critic_stats"] == (C.c_int, [p, p, i64, i32, i32, p, f, f, p, p, f, i64, p, p, p])
    assert L.PROTOTYPES["pqlk_unit_stats"] == (C.c_int, [p, i64, i64, i32, f, p, p, p])
    assert L.PROTOTYPES["pqlk_critic_stats_scratch_floats"] == (i64, [i64, i32])
    assert L.PROTOTYPES["pqlk_unit_stats_scratch_floats"] == (i64, [i32])
    assert (L.CRITIC_STATS, L.UNIT_CHUNKS) == (dc.N_STATS, dc.UNIT_CHUNKS) == (10, 64)
    assert (L.HEAD_SCALAR, L.HEAD_CATEGORICAL, L.HEAD_QUANTILE) == (dc.SCALAR, dc.CATEGORICAL, dc.QUANTILE)
    assert L.VERSION == 100      # the binding is derived from the header: new entries do not move the version
    assert STAT_KEYS == dc.NAMES and len(UNIT_KEYS) == 3


def test_scratch_sizes():
    for b, k in ((1, 1), (257, 1), (262145, 1), (5, 51), (4097, 64)):
        assert L.lib.pqlk_critic_stats_scratch_floats(b, k) == 10 * L.lib.pqlk_loss_parts(b, k) == 10 * dc.blocks_of(b, k)
    assert L.lib.pqlk_critic_stats_scratch_floats(0, 1) == 0 == L.lib.pqlk_critic_stats_scratch_floats(4, 0)
    assert L.lib.pqlk_unit_stats_scratch_floats(513) == (2 * 64 + 1) * 513 and L.lib.pqlk_unit_stats_scratch_floats(0) == 0


# host arrays stand in for device buffers: a refused call returns before anything is launched or dereferenced
_BUF = {n: (C.c_float * 64)() for n in ("q", "qt", "z", "rew", "done", "out", "scr", "h")}


def _critic(head=dc.SCALAR, k=1, ld=32, b=4, v_min=-1.0, v_max=1.0, null=()):
    a = {n: (None if n in null else C.cast(v, C.c_void_p)) for n, v in _BUF.items()}
    return L.lib.pqlk_critic_stats(a["q"], a["qt"], ld, head, k, a["z"], v_min, v_max, a["rew"], a["done"], 0.5, b, a["out"], a["scr"], None)


def _unit(ld=32, rows=4, cols=8, tau=0.025, null=()):
    a = {n: (None if n in null else C.cast(v, C.c_void_p)) for n, v in _BUF.items()}
    return L.lib.pqlk_unit_stats(a["h"], ld, rows, cols, tau, a["out"], a["scr"], None)


def test_critic_stats_refusals():
    for name in ("q", "qt", "rew", "done", "out", "scr"):
        for head, k in ((dc.SCALAR, 1), (dc.CATEGORICAL, 8), (dc.QUANTILE, 8)):
            assert _critic(head, k, null=(name,)) == L.E_NULL, name
    assert _critic(dc.CATEGORICAL, 8, null=("z",)) == L.E_NULL
    for head in (-1, 3, 7):
        assert _critic(head, 1) == L.E_UNSUPPORTED
    for kw in (dict(b=0), dict(b=-2), dict(k=2), dict(k=0), dict(head=dc.CATEGORICAL, k=1), dict(head=dc.QUANTILE, k=1),
               dict(head=dc.CATEGORICAL, k=8, v_min=1.0, v_max=1.0), dict(head=dc.CATEGORICAL, k=8, v_min=2.0, v_max=-2.0)):
        assert _critic(**kw) == L.E_SHAPE, kw
    assert _critic(dc.CATEGORICAL, L.C51_MAX_ATOMS + 1, ld=512) == L.E_UNSUPPORTED
    assert _critic(dc.QUANTILE, L.QR_MAX_QUANTILES + 1, ld=96) == L.E_UNSUPPORTED
    for kw in (dict(ld=0), dict(ld=16), dict(ld=48), dict(head=dc.CATEGORICAL, k=51, ld=32), dict(head=dc.QUANTILE, k=64, ld=32)):
        assert _critic(**kw) == L.E_ALIGN, kw
    assert all(v == 0.0 for v in _BUF["out"]) and all(v == 0.0 for v in _BUF["scr"])


def test_unit_stats_refusals():
    for name in ("h", "out", "scr"):
        assert _unit(null=(name,)) == L.E_NULL, name
    for kw in (dict(rows=0), dict(rows=-1), dict(cols=0), dict(cols=-3), dict(ld=7), dict(tau=1.0), dict(tau=-0.1), dict(tau=1.5),
               dict(tau=float("nan")), dict(tau=float("inf"))):
        assert _unit(**kw) == L.E_SHAPE, kw
    assert all(v == 0.0 for v in _BUF["out"]) and all(v == 0.0 for v in _BUF["scr"])


# ------------------------------------------------------------------------------------------------ algo.diag
@pytest.mark.parametrize("algo", ["pql_algo", "ddpg_algo", "sac_algo", "droq_algo", "tqc_algo", "crossq_algo"])
def test_defaults_are_off_everywhere(algo):
    cfg = cfg_of(algo)
    assert dict(cfg.algo.diag) == {"enabled": False, "every": 10, "tau": 0.025}
    assert diag_cfg(cfg) is None


def test_ppo_has_no_node_and_stays_off():
    cfg = cfg_of("ppo_algo")
    assert cfg.algo.get("diag") is None and diag_cfg(cfg) is None


@pytest.mark.parametrize("algo", ["pql_algo", "ddpg_algo"])
def test_accepted_where_it_is_built(algo):
    assert diag_cfg(cfg_of(algo, ON)) == (10, 0.025)
    assert diag_cfg(cfg_of(algo, ON, "algo.diag.every=1", "algo.diag.tau=0")) == (1, 0.0)
    assert diag_cfg(cfg_of(algo, ON, "algo.diag.every=3", "algo.diag.tau=0.5")) == (3, 0.5)


@pytest.mark.parametrize("algo,name", [("sac_algo", "SAC"), ("droq_algo", "SAC"), ("tqc_algo", "TQC"), ("crossq_algo", "CrossQ")])
def test_out_of_scope_algos_are_refused_naming_the_key(algo, name):
    with pytest.raises(ValueError, match=r"algo\.diag\.enabled=True cannot run with algo\.name=" + name):
        diag_cfg(cfg_of(algo, ON))
    assert name in OUT_OF_SCOPE


def test_ppo_is_refused_naming_the_key():
    with pytest.raises(ValueError, match=r"algo\.diag\.enabled=True cannot run with algo\.name=PPO"):
        diag_cfg(cfg_of("ppo_algo", "+algo.diag.enabled=True"))


def test_agents_and_the_learner_refuse_before_anything_is_allocated(monkeypatch):
    """The constructors reach `diag_cfg` before they touch a device: with no GPU the refusal is still the config's."""
    from pql_amd.algo.pql_v_learner import PQLVLearner
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(ValueError, match=r"algo\.diag\.every"):
        PQLVLearner((8,), 2, cfg_of("pql_algo", ON, "algo.diag.every=0"))
    with pytest.raises(L.PqlkError, match="needs an MI355X"):     # an accepted config stops at the missing device
        PQLVLearner((8,), 2, cfg_of("pql_algo", ON))
    from pql_amd.algo.ppo import AgentPPO
    from pql_amd.algo.sac import AgentSAC
    for cls, cfg in ((AgentPPO, cfg_of("ppo_algo", "+algo.diag.enabled=True")), (AgentSAC, cfg_of("sac_algo", ON))):
        with pytest.raises(ValueError, match=r"algo\.diag\.enabled=True cannot run"):
            cls(None, cfg)


@pytest.mark.parametrize("extra,key", [(("algo.diag.every=0",), "algo.diag.every"), (("algo.diag.every=-3",), "algo.diag.every"),
                                       (("algo.diag.every=2.5",), "algo.diag.every"), (("algo.diag.every=null",), "algo.diag.every"),
                                       (("algo.diag.tau=1",), "algo.diag.tau"), (("algo.diag.tau=-0.1",), "algo.diag.tau"),
                                       (("algo.diag.tau=null",), "algo.diag.tau"), (("algo.diag.enabled=yes_please",), "algo.diag.enabled")])
def test_bad_values_are_refused_naming_the_key(extra, key):
    for on in ((ON,), ()):          # on or off: a bad value does not wait for the day the switch is turned
        if key == "algo.diag.enabled" and on:
            continue
        with pytest.raises(ValueError, match=key.replace(".", r"\.")):
            diag_cfg(cfg_of("pql_algo", *on, *extra))


@pytest.mark.parametrize("algo", ["pql_algo", "ddpg_algo"])
def test_the_keys_are_not_part_of_a_checkpoints_structure(algo):
    from pql_amd.utils import checkpoint as CK
    plain = CK.structure(cfg_of(algo), 8, 2)
    for extra in ((ON,), (ON, "algo.diag.every=1", "algo.diag.tau=0.5")):
        assert CK.structure(cfg_of(algo, *extra), 8, 2) == plain
    assert "diag" not in str(plain)


def test_log_keys():
    assert log_keys(2) == ["diag/q1_mean", "diag/q2_mean", "diag/q_min", "diag/q_max", "diag/target_mean", "diag/td_bias", "diag/td_abs_mean",
                           "diag/td_abs_max", "diag/twin_gap", "diag/nonfinite", "diag/dormant_l1", "diag/act_abs_l1", "diag/elu_slope_l1",
                           "diag/dormant_l2", "diag/act_abs_l2", "diag/elu_slope_l2"]


def test_decode_averages_the_twin_nets():
    from pql_amd.algo.diag import CriticProbe
    probe = CriticProbe.__new__(CriticProbe)
    probe.layers = 2
    vals = list(np.arange(10, dtype=np.float64)) + [0.0, 1.0, 0.5, 0.5, 2.0, 0.25,      # net 0: layer 1, layer 2
                                                    1.0, 3.0, 1.0, 0.0, 4.0, 0.75]      # net 1
    out = probe.decode(vals)
    assert list(out) == log_keys(2)
    assert [out[k] for k in log_keys(2)[:10]] == list(range(10))
    assert (out["diag/dormant_l1"], out["diag/act_abs_l1"], out["diag/elu_slope_l1"]) == (0.5, 2.0, 0.75)
    assert (out["diag/dormant_l2"], out["diag/act_abs_l2"], out["diag/elu_slope_l2"]) == (0.25, 3.0, 0.5)
