"""Prioritized replay in the PQL V-learner (`algo.per.refresh=run`) without a GPU: the config key, who refuses what, the
checkpoint structure, and the declaration and argument errors of `pqlk_per_sample_steps`."""
import ctypes as C
import os
import re

import pytest

from support import cfg_of as _cfg
from task_cases import load_script

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_NULL, E_SHAPE, E_RANGE = 1, 2, 3
ON = ("algo.per.enabled=True",)
RUN = ON + ("algo.per.refresh=run",)


def _script(name):
    return load_script(f"scripts/{name}.py", name)


@pytest.mark.parametrize("algo", ["ddpg_algo", "sac_algo", "crossq_algo", "pql_algo"])
def test_refresh_defaults_to_step_and_composes(algo):
    from pql_amd.replay.prioritized_replay import per_cfg, per_refresh
    assert _cfg(algo).algo.per.refresh == "step"
    assert per_refresh(per_cfg(_cfg(algo, *ON).algo)) == "step"
    assert per_refresh(per_cfg(_cfg(algo, *RUN).algo)) == "run"
    assert per_refresh({"enabled": True}) == "step"                       # a block without the key
    with pytest.raises(ValueError, match=r"algo\.per\.refresh must be step or run"):
        per_refresh(per_cfg(_cfg(algo, *ON, "algo.per.refresh=sometimes").algo))
    text = open(os.path.join(ROOT, "pql_amd", "cfg", "algo", "off_policy.yaml")).read()
    assert re.search(r"^#\s*refresh: step", text, re.M) and re.search(r"^#\s*run\s*=", text, re.M)


@pytest.mark.parametrize("algo,module,cls", [("ddpg_algo", "pql_amd.algo.ddpg", "AgentDDPG"), ("sac_algo", "pql_amd.algo.sac", "AgentSAC"),
                                             ("crossq_algo", "pql_amd.algo.crossq", "AgentCrossQ")])
def test_baselines_refuse_run(algo, module, cls):
    """Before anything is allocated: the environment is never looked at."""
    import importlib
    from pql_amd.algo.learner import check_per_refresh
    with pytest.raises(ValueError, match=r"algo\.per\.refresh=run cannot run in algo=\w+.*algo\.per\.refresh=step"):
        getattr(importlib.import_module(module), cls)(env=None, cfg=_cfg(algo, *RUN))
    check_per_refresh(_cfg(algo, *ON), "x")                               # step: accepted
    check_per_refresh(_cfg(algo, "algo.per.refresh=run"), "x")            # the key alone, replay uniform: nothing to refuse


def _pql_makers(cfg):
    from pql_amd.algo.pql_p_learner import PQLPLearner
    from pql_amd.algo.pql_v_learner import PQLVLearner
    return {"PQLVLearner": lambda: PQLVLearner((8,), 2, cfg), "PQLPLearner": lambda: PQLPLearner((8,), 2, cfg),
            "scripts/train_pql.py": lambda: _script("train_pql").main(cfg)}


def test_pql_refuses_step_with_the_old_message_and_a_pointer():
    for extra in (ON, ON + ("algo.per.refresh=step",)):
        for name, make in _pql_makers(_cfg("pql_algo", *extra)).items():
            with pytest.raises(ValueError, match=r"algo\.per\.enabled=True cannot run in " + re.escape(name)
                               + r".*does not change between hand-offs.*train_baselines\.py.*algo\.per\.refresh=run"):
                make()


def test_pql_accepts_run():
    """`check_critic_class` lets the three PQL components pass; without a GPU the learners then stop at their device check, which
    comes after every refusal."""
    from pql_amd import _lib as L
    from pql_amd.algo.critics import check_critic_class
    cfg = _cfg("pql_algo", *RUN)
    for name in ("scripts/train_pql.py", "PQLVLearner", "PQLPLearner"):
        check_critic_class(cfg, name)
    import torch
    if not torch.cuda.is_available():
        makers = _pql_makers(cfg)
        for name in ("PQLVLearner", "PQLPLearner"):
            with pytest.raises(L.PqlkError, match="needs an MI355X"):
                makers[name]()


def test_v_learner_refuses_c51_and_data_parallel_before_allocating():
    from pql_amd.algo.pql_p_learner import PQLPLearner
    from pql_amd.algo.pql_v_learner import PQLVLearner
    with pytest.raises(ValueError, match=r"algo\.distl=True.*algo\.per\.enabled=True.*algo\.per\.refresh=run.*C51"):
        PQLVLearner((8,), 2, _cfg("pql_algo", *RUN, "algo.distl=True"))
    group = object()   # never used: the refusal comes first
    with pytest.raises(ValueError, match=r"algo\.per\.enabled=True.*algo\.per\.refresh=run.*process group"):
        PQLVLearner((8,), 2, _cfg("pql_algo", *RUN), process_group=group)
    with pytest.raises(ValueError, match=r"algo\.graph_rng=True.*algo\.per\.enabled=True"):
        PQLVLearner((8,), 2, _cfg("pql_algo", *RUN, "algo.graph_rng=True"))
    # the P-learner samples observations only: it accepts the key and ignores it, C51 or not (it fails later, at its device check or not at all)
    from pql_amd import _lib as L
    try:
        PQLPLearner((8,), 2, _cfg("pql_algo", *RUN, "algo.distl=True"))
    except L.PqlkError as e:
        assert "needs an MI355X" in str(e)


def test_structure_carries_refresh():
    from pql_amd.utils import checkpoint as CK
    off = CK.structure(_cfg("pql_algo"), 8, 2)
    step, run = CK.structure(_cfg("ddpg_algo", *ON), 8, 2), CK.structure(_cfg("pql_algo", *RUN), 8, 2)
    assert off["algo.per.refresh"] is None and step["algo.per.refresh"] == "step" and run["algo.per.refresh"] == "run"
    assert CK.structure(_cfg("pql_algo", "algo.per.refresh=run"), 8, 2)["algo.per.refresh"] is None   # counts only when it is on
    with pytest.raises(ValueError, match=r"algo\.per\.refresh='step' .*algo\.per\.refresh='run'"):
        CK.check_structure(run, {**run, "algo.per.refresh": "step"})
    with pytest.raises(ValueError, match=r"algo\.per\.refresh='run' .*algo\.per\.refresh='step'"):
        CK.check_structure({**run, "algo.per.refresh": "step"}, run)
    CK.check_structure(run, dict(run))
    # a checkpoint from before the key existed: prioritized means refreshed every step, uniform means nothing
    old_on = {k: v for k, v in step.items() if k != "algo.per.refresh"}
    CK.check_structure(old_on, step)
    with pytest.raises(ValueError, match=r"algo\.per\.refresh='run' .*algo\.per\.refresh='step'"):
        CK.check_structure({**old_on, **{k: run[k] for k in run if k not in ("algo.per.refresh",)}}, run)
    old_off = {k: v for k, v in off.items() if not k.startswith("algo.per.")}
    CK.check_structure(old_off, off)


def test_entry_is_declared_exported_and_bound():
    from pql_amd import _lib as L
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pqlk.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+pqlk_per_sample_steps\s*\(([^)]*)\)", hdr)
    assert m, "pqlk_per_sample_steps is not declared in include/pqlk.h"
    args = [re.sub(r"\s+", " ", a.strip()) for a in m.group(1).split(",")]
    assert args == ["const float* tree", "int64_t capacity", "const int64_t* r", "int64_t b", "int64_t steps", "int64_t n_valid", "float beta",
                    "int64_t* idx_out", "float* w_out", "float* wmax_out", "pqlk_stream_t stream"]
    assert hasattr(C.CDLL(os.fspath(L.LIB_FILE)), "pqlk_per_sample_steps")
    P, I64 = C.c_void_p, C.c_int64
    assert L.PROTOTYPES["pqlk_per_sample_steps"] == (C.c_int, [P, I64, P, I64, I64, I64, C.c_float, P, P, P, P])
    from pql_amd.replay.prioritized_replay import PrioritizedReplayBuffer
    assert callable(PrioritizedReplayBuffer.draw_steps)


def test_argument_errors_are_codes():
    """0x1000 stands in for a device pointer: validation comes before any launch and never dereferences it."""
    from pql_amd import _lib as L
    P = C.c_void_p(0x1000)
    # (tree, capacity, r, b, steps, n_valid, beta, idx_out, w_out, wmax_out, stream)
    call = lambda tree=P, cap=100, r=P, b=8, steps=3, n=50, idx=P, w=P, wmax=P: L.lib.pqlk_per_sample_steps(  # noqa: E731
        tree, cap, r, b, steps, n, 0.4, idx, w, wmax, None)
    assert call(tree=None) == E_NULL and call(r=None) == E_NULL and call(idx=None) == E_NULL and call(w=None) == E_NULL
    assert call(wmax=None) == E_NULL
    assert call(b=0) == E_SHAPE and call(b=-1) == E_SHAPE and call(steps=0) == E_SHAPE and call(n=0) == E_SHAPE and call(n=-5) == E_SHAPE
    assert call(cap=0) == E_SHAPE and call(steps=65536) == E_SHAPE
    assert call(n=101) == E_RANGE and call(cap=49) == E_RANGE
