"""algo.distl_loss / algo.hl_sigma without a GPU: the defaults of every off-policy config, the refusals of `check_critic_class` with their
messages, that neither key reaches a critic's constructor or a checkpoint's structure, and `CriticHead`'s dispatch on spies -- which
entry of include/pqlk.h a categorical head issues under either law, with which positional arguments, and what divides its loss."""
import ctypes as C
from types import SimpleNamespace

import pytest
import torch

import critic_rule_cases as cc
from pql_amd import _lib as L
from pql_amd.algo.critics import check_critic_class, make_critic
from pql_amd.algo.heads import CriticHead
from pql_amd.algo.learner import LOSS_RING, f32_recip
from support import cfg_of

HL = ("algo.distl=True", "algo.distl_loss=hl_gauss")
ENTRIES = ("pqlk_c51_bce_loss", "pqlk_hlgauss_ce_loss", "pqlk_hlgauss_ce_loss_per", "pqlk_td_mse_loss", "pqlk_td_mse_loss_per")
STREAM = "the stream"
B, LD, GAMMA_N, ATOMS, V_MIN, V_MAX, SIGMA = 37, 64, 0.9702, 51, -7.5, 12.25, 0.625

T = {k: torch.zeros(4) for k in ("q", "qt", "rew", "done", "dy", "ring", "scratch", "w", "wmax", "abs_td", "z")}
T["step"] = torch.zeros(1, dtype=torch.int32)
P = {k: v.data_ptr() for k, v in T.items()}
assert len(set(P.values())) == len(P)


# ------------------------------------------------------------------------------------------------ config
@pytest.mark.parametrize("algo", cc.ALGOS)
def test_defaults_under_every_off_policy_config(algo):
    cfg = cfg_of(algo)
    assert cfg.algo.distl_loss == "c51" and cfg.algo.hl_sigma == 0.75
    check_critic_class(cfg)


def test_the_abi_declares_both_entries():
    a, b = L.PROTOTYPES["pqlk_hlgauss_ce_loss"], L.PROTOTYPES["pqlk_hlgauss_ce_loss_per"]
    p, f = C.c_void_p, C.c_float
    want = [p, p, C.c_int64, C.c_int32, p, p, p, f, f, f, f, C.c_int64, p, p, p, C.c_int32, p, p]
    assert a == (C.c_int, want + [p]) and b == (C.c_int, want + [p, p, p, p])
    c51 = L.PROTOTYPES["pqlk_c51_bce_loss"][1]
    assert a[1] == c51[:10] + [f] + c51[10:]      # C51's arguments with sigma_ratio behind v_max


@pytest.mark.parametrize("fused", cc.FUSED)
def test_refusals_name_the_key_and_the_value(fused):
    for algo, extra, words in (
            ("pql_algo", ("algo.distl=True", "algo.distl_loss=hlgauss"), ("algo.distl_loss", "'hlgauss'", "c51 or hl_gauss")),
            ("pql_algo", ("algo.distl_loss=null",), ("algo.distl_loss", "None")),
            ("pql_algo", ("algo.distl_loss=hl_gauss",), ("algo.distl_loss=hl_gauss", "algo.distl=True", "False")),
            ("ddpg_algo", ("algo.distl_loss=hl_gauss",), ("algo.distl_loss=hl_gauss", "algo.distl=True")),
            ("sac_algo", HL, ("algo.distl_loss=hl_gauss", "algo.name=SAC")),
            ("crossq_algo", HL, ("algo.distl_loss=hl_gauss", "algo.name=CrossQ")),
            ("tqc_algo", (*HL, "algo.cri_class=QuantileDoubleQ", "algo.qr_drop=2"), ("algo.distl_loss=hl_gauss", "algo.name=TQC")),
            ("droq_algo", HL, ("algo.distl_loss=hl_gauss", "algo.name=SAC")),
            ("pql_algo", (*HL, "algo.hl_sigma=0"), ("algo.hl_sigma", "> 0", "0")),
            ("pql_algo", (*HL, "algo.hl_sigma=-0.75"), ("algo.hl_sigma", "-0.75")),
            ("ddpg_algo", (*HL, "algo.hl_sigma=null"), ("algo.hl_sigma", "None")),
            ("pql_algo", ("algo.hl_sigma=0",), ("algo.hl_sigma", "> 0"))):     # a wrong sigma is refused under c51 as well
        if fused is not None and algo != "pql_algo":
            continue
        with pytest.raises(ValueError) as e:
            check_critic_class(cfg_of(algo, *extra), fused)
        for word in words:
            assert word in str(e.value), (extra, word, str(e.value))


@pytest.mark.parametrize("algo", ["pql_algo", "ddpg_algo"])
def test_hl_gauss_is_accepted_where_it_is_built(algo):
    for extra in (HL, (*HL, "algo.hl_sigma=1.5"), (*HL, "algo.num_atoms=256"), (*HL, "algo.per.enabled=True", "algo.per.refresh=run")):
        for fused in cc.FUSED if algo == "pql_algo" else (None,):
            check_critic_class(cfg_of(algo, *extra), fused)
    if algo == "pql_algo":   # where C51 takes the bf16 target forward, HL-Gauss does
        check_critic_class(cfg_of(algo, *HL, "algo.target_dtype=bfloat16"), "PQLVLearner")


@pytest.mark.parametrize("algo", ["pql_algo", "ddpg_algo"])
def test_neither_key_reaches_the_constructor_or_a_checkpoint(algo):
    from pql_amd.utils import checkpoint as CK
    made, structure = [], []
    for extra in (("algo.distl=True",), ("algo.distl=True", "algo.distl_loss=c51"), HL, (*HL, "algo.hl_sigma=1.5")):
        cfg = cfg_of(algo, *extra)
        structure.append(CK.structure(cfg, 8, 2))
        with cc._no_device_switch():
            torch.manual_seed(0)
            critic = make_critic(cfg, (8,), 2, torch.device("cpu"))
        made.append((type(critic).__name__, critic.init_kwargs, int(critic.num_params()), str(cfg.algo.cri_class)))
    assert all(m == made[0] for m in made) and all(s == structure[0] for s in structure)
    assert made[0][0] == "DistributionalDoubleQ" and "hl_sigma" not in str(made[0][1]) and "distl_loss" not in str(structure[0])


def test_neither_key_is_a_rules_row():
    from pql_amd.algo import critics
    for row in critics.TABLE.values():
        assert not {"distl_loss", "hl_sigma"} & ({k[0] for k in row.keys} | set(row.structure))
    assert not any("distl_loss" in k or "hl_sigma" in k for k in critics.STRUCTURE_DEFAULTS)


# ------------------------------------------------------------------------------------------------ CriticHead on spies
@pytest.fixture
def calls(monkeypatch):
    seen = []
    for name in ENTRIES:
        monkeypatch.setattr(L.lib, name, lambda *a, _n=name: seen.append((_n, tuple(v.value if isinstance(v, C.c_void_p) else v for v in a))) or 0)
    monkeypatch.setattr(L, "stream", lambda device=None: STREAM)
    return seen


def _head(**algo):
    critic = SimpleNamespace(head="categorical", num_atoms=ATOMS, z_atoms=T["z"])
    return CriticHead(critic, SimpleNamespace(qr_drop=None, v_min=V_MIN, v_max=V_MAX, **algo))


def _critic_loss(head, ring=True, per=False):
    head.critic_loss(T["q"], T["qt"], LD, T["rew"], T["done"], GAMMA_N, B, T["dy"], T["ring"] if ring else None, T["step"], T["scratch"], None,
                     per=(T["w"], T["wmax"], T["abs_td"]) if per else None, kappa=0.5)


FRONT = (P["q"], P["qt"], LD, ATOMS, P["rew"], P["done"], P["z"], GAMMA_N, V_MIN, V_MAX)


@pytest.mark.parametrize("ring", [True, False])
@pytest.mark.parametrize("per", [False, True])
def test_hl_gauss_dispatch(calls, per, ring):
    _critic_loss(_head(distl_loss="hl_gauss", hl_sigma=SIGMA), ring, per)
    out = (B, P["dy"], P["ring"] if ring else None, P["step"], LOSS_RING, None, P["scratch"])     # target_out = NULL in front of scratch
    tail = (P["w"], P["wmax"], P["abs_td"]) if per else ()
    assert calls == [("pqlk_hlgauss_ce_loss_per" if per else "pqlk_hlgauss_ce_loss", (*FRONT, SIGMA, *out, *tail, STREAM))]
    assert type(calls[0][1][10]) is float and all(type(v) is int for v in calls[0][1][2:4])


def test_hl_sigma_defaults_to_three_quarters(calls):
    _critic_loss(_head(distl_loss="hl_gauss"))
    assert calls[0][0] == "pqlk_hlgauss_ce_loss" and calls[0][1][10] == 0.75


@pytest.mark.parametrize("algo", [{}, {"distl_loss": "c51"}, {"distl_loss": "c51", "hl_sigma": 0.3}, {"distl_loss": None}])
def test_c51_call_is_unchanged_and_still_refuses_weights(calls, algo):
    """The key absent, null or c51: today's call, argument for argument (tests/test_heads_cpu.py's), and no weighted form."""
    _critic_loss(_head(**algo))
    assert calls == [("pqlk_c51_bce_loss", (*FRONT, B, P["dy"], P["ring"], P["step"], LOSS_RING, None, P["scratch"], STREAM))]
    with pytest.raises(ValueError, match="no weighted C51 loss"):
        _critic_loss(_head(**algo), per=True)
    assert len(calls) == 1


def test_the_law_is_read_when_a_loss_is_issued(calls):
    head = _head(distl_loss="c51")
    _critic_loss(head)
    head.algo.distl_loss = "hl_gauss"
    _critic_loss(head)
    assert [c[0] for c in calls] == ["pqlk_c51_bce_loss", "pqlk_hlgauss_ce_loss"]


@pytest.mark.parametrize("b", [1, 37, 4099, 70000])
def test_fold_parts_and_scale(b):
    hl, c51 = _head(distl_loss="hl_gauss"), _head()
    assert hl.critic_scale(b) == f32_recip(b) and c51.critic_scale(b) == f32_recip(b, ATOMS)
    assert hl.loss_parts(b) == c51.loss_parts(b) == L.lib.pqlk_loss_parts(b, ATOMS)
    assert (hl.kind, hl.width, hl.hl_gauss, c51.hl_gauss) == ("categorical", ATOMS, True, False)


def test_other_heads_ignore_the_key(calls):
    head = CriticHead(SimpleNamespace(num_atoms=1), SimpleNamespace(qr_drop=None, distl_loss="hl_gauss"))
    assert not head.hl_gauss and head.critic_scale(B) == f32_recip(B)
    _critic_loss(head, per=True)
    assert calls[0][0] == "pqlk_td_mse_loss_per"


def test_actor_loss_is_unchanged(monkeypatch):
    seen = []
    monkeypatch.setattr(L.lib, "pqlk_dpg_loss", lambda *a: seen.append(tuple(v.value if isinstance(v, C.c_void_p) else v for v in a)) or 0)
    monkeypatch.setattr(L, "stream", lambda device=None: STREAM)
    for algo in ({}, {"distl_loss": "hl_gauss"}):
        _head(**algo).actor_loss(T["q"], LD, B, T["dy"], None, T["step"], T["scratch"], None)
    assert seen[0] == seen[1] == (P["q"], LD, ATOMS, P["z"], B, P["dy"], None, P["step"], LOSS_RING, P["scratch"], STREAM)


def test_v_learner_refuses_prioritized_replay_under_c51_only(monkeypatch):
    """Before anything is allocated: C51 with today's message; HL-Gauss passes every refusal and stops at the missing device."""
    from pql_amd.algo.pql_v_learner import PQLVLearner
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    per = ("algo.distl=True", "algo.per.enabled=True", "algo.per.refresh=run")
    for extra in (per, (*per, "algo.distl_loss=c51")):
        with pytest.raises(ValueError, match="there is no weighted C51 loss"):
            PQLVLearner((8,), 2, cfg_of("pql_algo", *extra))
    with pytest.raises(L.PqlkError, match="needs an MI355X"):
        PQLVLearner((8,), 2, cfg_of("pql_algo", *per, "algo.distl_loss=hl_gauss"))
