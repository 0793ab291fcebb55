"""`CriticHead` (pql_amd/algo/heads.py) without a GPU: for every reachable combination of head kind, prioritized replay, algo.qr_drop,
the soft target and the actor loss's owner / mean switch, WHICH of the thirteen loss entries it issues and with WHICH positional
arguments -- written out here from the parameter order of include/pqlk.h, so the positions of drop, logp / log_alpha and the
weights are held -- and the parts and the scale of its fold.  The entries are spies that return 0; the pointers are those of CPU tensors.
"""
import ctypes as C
import itertools
from types import SimpleNamespace

import pytest
import torch

from pql_amd import _lib as L
from pql_amd.algo.heads import CriticHead
from pql_amd.algo.learner import LOSS_RING, f32_recip

ENTRIES = ("pqlk_td_mse_loss", "pqlk_td_mse_loss_per", "pqlk_c51_bce_loss", "pqlk_qr_huber_loss", "pqlk_qr_huber_loss_per", "pqlk_tqc_huber_loss",
           "pqlk_tqc_huber_loss_per", "pqlk_tqc_huber_loss_soft", "pqlk_tqc_huber_loss_soft_per", "pqlk_dpg_loss", "pqlk_dpg_loss_owner",
           "pqlk_dpg_loss_quantile", "pqlk_dpg_loss_quantile_mean")
STREAM = "the stream"
B, LD, GAMMA_N, KAPPA, ATOMS, QUANTILES, V_MIN, V_MAX = 37, 64, 0.9702, 0.75, 51, 33, -7.5, 12.25


def _t(n=4, dtype=torch.float32):
    return torch.zeros(n, dtype=dtype)


T = {k: _t() for k in ("q", "qt", "rew", "done", "dy", "ring", "scratch", "w", "wmax", "abs_td", "logp", "log_alpha", "z")}
T["step"], T["owner"] = _t(1, torch.int32), _t(4, torch.uint8)
P = {k: v.data_ptr() for k, v in T.items()}
assert len(set(P.values())) == len(P)   # a swapped pair of pointers shows


def _critic(kind):
    if kind == "scalar":
        return SimpleNamespace(num_atoms=1)   # (no `head`: the LayerNorm / BatchNorm critics)
    if kind == "categorical":
        return SimpleNamespace(head=kind, num_atoms=ATOMS, z_atoms=T["z"])
    return SimpleNamespace(head=kind, num_atoms=1, num_quantiles=QUANTILES)


def _head(kind, drop=None):
    return CriticHead(_critic(kind), SimpleNamespace(qr_drop=drop, v_min=V_MIN, v_max=V_MAX))


@pytest.fixture
def calls(monkeypatch):
    seen = []
    for name in ENTRIES:
        monkeypatch.setattr(L.lib, name, lambda *a, _n=name: seen.append((_n, tuple(v.value if isinstance(v, C.c_void_p) else v for v in a))) or 0)
    monkeypatch.setattr(L, "stream", lambda device=None: STREAM)
    return seen


def _critic_loss(head, ring, per, soft):
    head.critic_loss(T["q"], T["qt"], LD, T["rew"], T["done"], GAMMA_N, B, T["dy"], T["ring"] if ring else None, T["step"], T["scratch"], None,
                     per=(T["w"], T["wmax"], T["abs_td"]) if per else None, soft=(T["logp"], T["log_alpha"]) if soft else None, kappa=KAPPA)


def test_every_loss_entry_is_watched():
    """The five critic-loss families with their `_per` / `_soft` instances and the four actor-loss entries: all a head may issue."""
    assert len(set(ENTRIES)) == 13 and all(name in L.PROTOTYPES for name in ENTRIES)
    assert not [n for n in L.PROTOTYPES if ("_loss" in n and n.startswith(("pqlk_td_mse", "pqlk_c51_bce", "pqlk_qr_", "pqlk_tqc_", "pqlk_dpg_loss")))
                and n not in ENTRIES]


@pytest.mark.parametrize("ring", [True, False])
@pytest.mark.parametrize("per", [False, True])
def test_scalar_critic_loss(calls, per, ring):
    _critic_loss(_head("scalar"), ring, per, False)
    out = (P["dy"], P["ring"] if ring else None, P["step"], LOSS_RING, P["scratch"])
    weights = (P["w"], P["wmax"], P["abs_td"]) if per else ()
    assert calls == [("pqlk_td_mse_loss_per" if per else "pqlk_td_mse_loss",
                      (P["q"], P["qt"], LD, P["rew"], P["done"], GAMMA_N, B, *out, *weights, STREAM))]


def test_categorical_critic_loss(calls):
    _critic_loss(_head("categorical"), True, False, False)
    assert calls == [("pqlk_c51_bce_loss", (P["q"], P["qt"], LD, ATOMS, P["rew"], P["done"], P["z"], GAMMA_N, V_MIN, V_MAX, B, P["dy"], P["ring"],
                                            P["step"], LOSS_RING, None, P["scratch"], STREAM))]


@pytest.mark.parametrize("per, drop, soft", [c for c in itertools.product([False, True], [None, 0, 2], [False, True]) if not (c[2] and c[1] is None)])
def test_quantile_critic_loss(calls, per, drop, soft):
    _critic_loss(_head("quantile", drop), True, per, soft)
    name = "pqlk_qr_huber_loss" if drop is None else "pqlk_tqc_huber_loss_soft" if soft else "pqlk_tqc_huber_loss"
    args = (P["q"], P["qt"], LD, QUANTILES, P["rew"], P["done"], GAMMA_N, KAPPA, B, P["dy"], P["ring"], P["step"], LOSS_RING, P["scratch"])
    if per:    # the weights stand behind scratch ...
        args += (P["w"], P["wmax"], P["abs_td"])
    if soft:   # ... logp and log_alpha behind them ...
        args += (P["logp"], P["log_alpha"])
    if drop is not None:   # ... and drop last, in front of the stream
        args += (drop,)
    assert calls == [(name + ("_per" if per else ""), args + (STREAM,))]
    assert all(type(v) is int for v in calls[0][1][2:4]) and type(calls[0][1][7]) is float


def test_unsupported_combinations_raise(calls):
    for kind, drop, per, soft in (("scalar", None, False, True), ("quantile", None, False, True), ("categorical", None, False, True),
                                  ("categorical", None, True, False)):
        with pytest.raises(ValueError):
            _critic_loss(_head(kind, drop), True, per, soft)
    with pytest.raises(ValueError):
        _head("scalar").actor_loss(T["q"], LD, B, T["dy"], T["ring"], T["step"], T["scratch"], None, mean=True)
    with pytest.raises(ValueError):
        _head("quantile").actor_loss(T["q"], LD, B, T["dy"], T["ring"], T["step"], T["scratch"], None, owner=T["owner"])
    with pytest.raises(ValueError):
        CriticHead(SimpleNamespace(head="gauss"), SimpleNamespace())
    assert calls == []


@pytest.mark.parametrize("kind", ["scalar", "categorical"])
@pytest.mark.parametrize("owner", [False, True])
def test_min_actor_loss(calls, kind, owner):
    """The `_owner` entry takes the categorical head too (the P-learner's call; the kernel writes no owner when k > 1)."""
    _head(kind).actor_loss(T["q"], LD, B, T["dy"], None, T["step"], T["scratch"], None, owner=T["owner"] if owner else None)
    k, z = (1, None) if kind == "scalar" else (ATOMS, P["z"])
    args = (P["q"], LD, k, z, B, P["dy"], None, P["step"], LOSS_RING, P["scratch"])
    assert calls == [("pqlk_dpg_loss_owner", args + (P["owner"], STREAM)) if owner else ("pqlk_dpg_loss", args + (STREAM,))]


@pytest.mark.parametrize("mean", [False, True])
def test_quantile_actor_loss(calls, mean):
    _head("quantile", 2).actor_loss(T["q"], LD, B, T["dy"], T["ring"], T["step"], T["scratch"], None, mean=mean)
    assert calls == [("pqlk_dpg_loss_quantile_mean" if mean else "pqlk_dpg_loss_quantile",
                      (P["q"], LD, QUANTILES, B, P["dy"], P["ring"], P["step"], LOSS_RING, P["scratch"], STREAM))]


@pytest.mark.parametrize("b", [1, 37, 4099, 70000])
def test_fold_parts_and_scale(b):
    for kind, drop, width, divisor in (("scalar", None, 1, None), ("categorical", None, ATOMS, ATOMS), ("quantile", None, QUANTILES, QUANTILES),
                                       ("quantile", 0, QUANTILES, 2 * QUANTILES), ("quantile", 2, QUANTILES, 2 * (QUANTILES - 2))):
        head = _head(kind, drop)
        assert (head.kind, head.width) == (kind, width)
        assert head.loss_parts(b) == L.lib.pqlk_loss_parts(b, width)
        assert head.critic_scale(b) == (f32_recip(b) if divisor is None else f32_recip(b, divisor))
