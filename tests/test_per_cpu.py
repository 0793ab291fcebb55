"""Prioritized replay without a GPU: the entry points' declarations and sizing helpers, their argument errors, the config block, the
refusals of the PQL learners, the checkpoint structure and the beta schedule."""
import ctypes as C
import os
import re

import pytest

from support import cfg_of as _cfg
from task_cases import load_script

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("pqlk_per_insert", "pqlk_per_rebuild", "pqlk_per_sample", "pqlk_per_weights", "pqlk_per_update", "pqlk_td_mse_loss_per")
SIZING = ("pqlk_per_levels", "pqlk_per_tree_floats")
E_NULL, E_SHAPE, E_RANGE, E_ALIGN = 1, 2, 3, 4


def test_entries_are_declared_exported_and_bound():
    from pql_amd import _lib as L
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pqlk.h")).read(), flags=re.S)
    raw = C.CDLL(os.fspath(L.LIB_FILE))
    for name in NAMES + SIZING:
        assert re.search(rf"\b{name}\s*\(", hdr), name
        assert name in L.PROTOTYPES and hasattr(raw, name), name
    mk = open(os.path.join(ROOT, "pql_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS\s*=.*\bper\.hip\b", mk, re.M)
    assert L.lib.pqlk_version() == 100


def level_sizes(capacity):
    """Nodes per level: the leaves, then ceil(n / 64), until a level has at most 64."""
    n = [capacity]
    while n[-1] > 64:
        n.append(-(-n[-1] // 64))
    return n


@pytest.mark.parametrize("capacity,levels", [(1, 1), (64, 1), (65, 2), (4096, 2), (4097, 3), (5_000_000, 4)])
def test_sizing_helpers(capacity, levels):
    from pql_amd import _lib as L
    n = level_sizes(capacity)
    assert len(n) == levels == L.lib.pqlk_per_levels(capacity)
    assert L.lib.pqlk_per_tree_floats(capacity) == sum(-(-x // 64) * 64 for x in n)   # every level padded to a multiple of 64
    assert L.lib.pqlk_per_levels(0) == 0 and L.lib.pqlk_per_tree_floats(-3) == 0


def test_argument_errors_are_codes():
    """0x1000 stands in for a device pointer: validation comes before any launch and never dereferences it."""
    from pql_amd import _lib as L
    lib, P = L.lib, C.c_void_p(0x1000)
    # insert: (tree, capacity, pmax, dst_start, m, alpha, stream)
    assert lib.pqlk_per_insert(None, 100, P, 0, 4, 0.6, None) == E_NULL
    assert lib.pqlk_per_insert(P, 100, None, 0, 4, 0.6, None) == E_NULL
    assert lib.pqlk_per_insert(P, 0, P, 0, 4, 0.6, None) == E_SHAPE
    assert lib.pqlk_per_insert(P, 100, P, 0, 0, 0.6, None) == E_SHAPE
    assert lib.pqlk_per_insert(P, 100, P, 98, 4, 0.6, None) == E_RANGE     # rows 98..101 of a 100-row ring
    assert lib.pqlk_per_insert(P, 100, P, -1, 4, 0.6, None) == E_RANGE
    # rebuild: (tree, capacity, stream)
    assert lib.pqlk_per_rebuild(None, 100, None) == E_NULL
    assert lib.pqlk_per_rebuild(P, 0, None) == E_SHAPE
    # sample: (tree, capacity, u, b, idx_out, stream)
    assert lib.pqlk_per_sample(None, 100, P, 8, P, None) == E_NULL
    assert lib.pqlk_per_sample(P, 100, None, 8, P, None) == E_NULL
    assert lib.pqlk_per_sample(P, 100, P, 8, None, None) == E_NULL
    assert lib.pqlk_per_sample(P, 100, P, 0, P, None) == E_SHAPE
    assert lib.pqlk_per_sample(P, -1, P, 8, P, None) == E_SHAPE
    # weights: (tree, capacity, idx, b, n_valid, beta, w_out, wmax_out, stream)
    assert lib.pqlk_per_weights(P, 100, None, 8, 50, 0.4, P, P, None) == E_NULL
    assert lib.pqlk_per_weights(P, 100, P, 8, 50, 0.4, P, None, None) == E_NULL
    assert lib.pqlk_per_weights(P, 100, P, 0, 50, 0.4, P, P, None) == E_SHAPE
    assert lib.pqlk_per_weights(P, 100, P, 8, 0, 0.4, P, P, None) == E_SHAPE
    assert lib.pqlk_per_weights(P, 100, P, 8, 101, 0.4, P, P, None) == E_RANGE
    # update: (tree, capacity, pmax, idx, abs_td, b, eps, alpha, stream)
    assert lib.pqlk_per_update(P, 100, None, P, P, 8, 1e-6, 0.6, None) == E_NULL
    assert lib.pqlk_per_update(P, 100, P, P, None, 8, 1e-6, 0.6, None) == E_NULL
    assert lib.pqlk_per_update(P, 100, P, P, P, 0, 1e-6, 0.6, None) == E_SHAPE
    assert lib.pqlk_per_update(P, 0, P, P, P, 8, 1e-6, 0.6, None) == E_SHAPE
    # weighted loss: pqlk_td_mse_loss's arguments, then (w, wmax, abs_td_out, stream)
    loss = lambda b, ld, w, wmax, td: lib.pqlk_td_mse_loss_per(P, P, ld, P, P, 0.97, b, P, P, None, 1, P, w, wmax, td, None)  # noqa: E731
    assert loss(0, 32, P, P, P) == E_SHAPE
    assert loss(4, 20, P, P, P) == E_ALIGN
    assert loss(4, 32, None, P, P) == E_NULL and loss(4, 32, P, None, P) == E_NULL and loss(4, 32, P, P, None) == E_NULL
    assert L.PROTOTYPES["pqlk_td_mse_loss_per"][1] == L.PROTOTYPES["pqlk_td_mse_loss"][1][:-1] + [C.c_void_p] * 4


@pytest.mark.parametrize("algo", ["ddpg_algo", "sac_algo", "crossq_algo", "pql_algo"])
def test_config_default_is_off(algo):
    per = _cfg(algo).algo.per
    assert per.enabled is False
    assert (float(per.alpha), float(per.beta0), int(per.beta_iters), float(per.eps)) == (0.6, 0.4, 100000, 1.0e-6)
    from pql_amd.replay.prioritized_replay import per_cfg
    assert per_cfg(_cfg(algo).algo) is None
    on = per_cfg(_cfg(algo, "algo.per.enabled=True", "algo.per.alpha=0.5").algo)
    assert on is not None and float(on.alpha) == 0.5 and float(on.beta0) == 0.4
    text = open(os.path.join(ROOT, "pql_amd", "cfg", "algo", "off_policy.yaml")).read()
    assert re.search(r"^#.*prioritized", text, re.M)


def test_ppo_ignores_the_key():
    from pql_amd.replay.prioritized_replay import per_cfg
    assert per_cfg(_cfg("ppo_algo").algo) is None


def _script(name):
    return load_script(f"scripts/{name}.py", name)


def test_pql_learners_refuse_prioritized_replay():
    from pql_amd.algo.pql_p_learner import PQLPLearner
    from pql_amd.algo.pql_v_learner import PQLVLearner
    cfg = _cfg("pql_algo", "algo.per.enabled=True")
    for make in (lambda: PQLVLearner((8,), 2, cfg), lambda: PQLPLearner((8,), 2, cfg), lambda: _script("train_pql").main(cfg)):
        with pytest.raises(ValueError, match=r"algo\.per\.enabled=True.*train_baselines\.py"):
            make()


def test_resume_mismatch_names_both_values():
    from pql_amd.utils import checkpoint as CK
    off, on = CK.structure(_cfg("ddpg_algo"), 8, 2), CK.structure(_cfg("ddpg_algo", "algo.per.enabled=True"), 8, 2)
    assert off["algo.per.enabled"] is False and off["algo.per.alpha"] is None and on["algo.per.enabled"] is True and on["algo.per.alpha"] == 0.6
    with pytest.raises(ValueError, match=r"algo\.per\.enabled=False .*algo\.per\.enabled=True"):
        CK.check_structure(on, off)
    with pytest.raises(ValueError, match=r"algo\.per\.enabled=True .*algo\.per\.enabled=False"):
        CK.check_structure(off, on)
    other = CK.structure(_cfg("ddpg_algo", "algo.per.enabled=True", "algo.per.alpha=1.0"), 8, 2)
    with pytest.raises(ValueError, match=r"algo\.per\.alpha=1\.0 .*algo\.per\.alpha=0\.6"):
        CK.check_structure(on, other)
    CK.check_structure(on, CK.structure(_cfg("ddpg_algo", "algo.per.enabled=True", "algo.per.beta0=0.7", "algo.per.eps=1.0e-3"), 8, 2))
    # a checkpoint from before the keys existed was written with uniform replay; alpha does not count while it is off
    old = {k: v for k, v in off.items() if not k.startswith("algo.per.")}
    CK.check_structure(old, off)
    with pytest.raises(ValueError, match=r"algo\.per\.enabled"):
        CK.check_structure(old, on)
    CK.check_structure(off, CK.structure(_cfg("ddpg_algo", "algo.per.alpha=1.0"), 8, 2))


@pytest.mark.parametrize("beta0,iters", [(0.4, 100000), (0.4, 7), (0.0, 3), (1.0, 5), (0.123, 1)])
def test_beta_schedule(beta0, iters):
    from pql_amd.algo.ac_base import per_beta
    assert per_beta(beta0, iters, 0) == beta0
    seq = [per_beta(beta0, iters, c) for c in range(iters + 1)] if iters < 100 else [per_beta(beta0, iters, c) for c in (0, 1, iters // 2, iters - 1, iters)]
    assert all(a <= b for a, b in zip(seq, seq[1:])) and all(beta0 <= x <= 1.0 for x in seq)
    assert per_beta(beta0, iters, iters) == 1.0 and per_beta(beta0, iters, iters + 1) == 1.0 and per_beta(beta0, iters, 10 * iters) == 1.0
    if iters % 2 == 0:
        assert abs(per_beta(beta0, iters, iters // 2) - (beta0 + 1.0) / 2) < 1e-12
