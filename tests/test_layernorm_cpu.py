"""The LayerNorm twin critic without a GPU: host argument errors of the three entries, their prototypes, the module's state_dict
against the torch twin, the refusals, and DoubleQBatchNorm's keys and arena size after the move to the shared base."""
import os
import re

import numpy as np
import pytest
import torch
from torch import nn

from support import cfg_of as _cfg
from task_cases import load_script

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_NULL, E_SHAPE = 1, 2


def _twin(in_dim, hidden):
    class Net(nn.Module):
        def __init__(self):
            super().__init__()
            dims, layers = [in_dim, *hidden], []
            for i, o in zip(dims[:-1], dims[1:]):
                layers += [nn.Linear(i, o), nn.LayerNorm(o, eps=1e-5), nn.ELU()]
            self.net = nn.Sequential(*layers, nn.Linear(dims[-1], 1))

    class Twin(nn.Module):
        def __init__(self):
            super().__init__()
            self.net_q1, self.net_q2 = Net(), Net()

    return Twin()


def test_prototypes_declared_and_bound():
    from pql_amd import _lib as L
    text = open(os.path.join(ROOT, "include", "pqlk.h")).read()
    for name in ("pqlk_ln_scratch_floats", "pqlk_ln_elu_forward", "pqlk_ln_elu_backward"):
        assert re.search(rf"\b{name}\s*\(", text), name
        assert name in L.PROTOTYPES and hasattr(L.lib, name)
    chunks = int(re.search(r"#define\s+PQLK_LN_CHUNKS\s+(\d+)", text).group(1))
    assert L.lib.pqlk_ln_scratch_floats(130) == 2 * chunks * 130
    assert L.lib.pqlk_ln_scratch_floats(0) == 0


def test_host_argument_errors():
    """NULL pointers, m <= 0, cols <= 0, ld < cols are refused on the host, before any launch (so this runs without a GPU)."""
    from pql_amd import _lib as L
    p = L.ptr(torch.zeros(64))      # a valid host address: never dereferenced, the shape checks come first or no launch happens
    fwd, bwd = L.lib.pqlk_ln_elu_forward, L.lib.pqlk_ln_elu_backward
    ok_f = [p, 8, 2, 8, p, p, 1e-5, p, p, p, None]             # z ld m cols gamma beta eps y mean rstd stream
    for i in (0, 4, 5, 7, 8, 9):
        a = list(ok_f); a[i] = None
        assert fwd(*a) == E_NULL, i
    for i, v in ((2, 0), (2, -1), (3, 0), (3, -4), (1, 7)):
        a = list(ok_f); a[i] = v
        assert fwd(*a) == E_SHAPE, (i, v)
    ok_b = [p, p, p, 8, 2, 8, p, p, p, p, p, p, p, None]       # dy y z ld m cols mean rstd gamma dz dgamma dbeta scratch stream
    for i in (0, 1, 2, 6, 7, 8, 9):
        a = list(ok_b); a[i] = None
        assert bwd(*a) == E_NULL, i
    a = list(ok_b); a[12] = None
    assert bwd(*a) == E_NULL                                   # parameter gradients wanted, no scratch
    for i, v in ((4, 0), (4, -1), (5, 0), (5, -4), (3, 7)):
        a = list(ok_b); a[i] = v
        assert bwd(*a) == E_SHAPE, (i, v)
        a[10] = a[11] = a[12] = None                           # the shape is checked whether or not gradients are wanted
        assert bwd(*a) == E_SHAPE, (i, v)


@pytest.mark.parametrize("O,A,hidden", [(8, 2, None), (11, 3, [40, 24])])
def test_state_dict_round_trip_with_torch_twin(O, A, hidden):
    from pql_amd.models.layernorm import DoubleQLayerNorm
    from pql_amd.models.mlp import HIDDEN_DEFAULT
    q = DoubleQLayerNorm((O,), A, hidden_layers=hidden)
    twin = _twin(O + A, list(hidden or HIDDEN_DEFAULT))
    assert list(q.named_buffers()) == [] and [k for k, _ in q.named_parameters()] == ["arena"]
    sd = q.state_dict()
    assert list(sd.keys()) == list(twin.state_dict().keys())
    twin.load_state_dict(sd, strict=True)
    # fresh norms are (1, 0); the pad entries of the arena are zero
    assert all(bool((v == 1).all()) for k, v in sd.items() if re.search(r"\.(1|4|7)\.weight$", k))
    assert q.num_params() == sum(p.numel() for p in twin.parameters())
    assert int((q.arena.data != 0).sum()) <= q.num_params() < q.arena.numel()
    with torch.no_grad():
        for p_ in twin.parameters():
            p_.uniform_(-1, 1)
    q.load_state_dict(twin.state_dict(), strict=True)
    back = q.state_dict()
    assert all(torch.equal(back[k], v) for k, v in twin.state_dict().items())
    missing = dict(twin.state_dict()); del missing["net_q2.net.1.bias"]
    with pytest.raises(RuntimeError, match="net_q2.net.1.bias"):
        q.load_state_dict(missing, strict=True)


def test_deepcopy_gets_its_own_empty_workspace():
    from copy import deepcopy
    from pql_amd.models.layernorm import DoubleQLayerNorm
    q = DoubleQLayerNorm((8,), 2, hidden_layers=[32])
    q._ws[64] = {"dev": "stand-in"}
    t = deepcopy(q)
    assert t._ws == {} and q._ws != {} and torch.equal(t.arena, q.arena) and t.arena.data_ptr() != q.arena.data_ptr()


def test_batchnorm_critic_keys_and_arena_unchanged():
    """DoubleQBatchNorm after the move to the shared base: the key list (46 keys, in order) and the arena / buffer sizes it had."""
    import hashlib
    from pql_amd.models.batchnorm import DoubleQBatchNorm
    q = DoubleQBatchNorm((8,), 2)
    keys = list(q.state_dict().keys())
    assert len(keys) == 46 and hashlib.sha256("\n".join(keys).encode()).hexdigest()[:16] == "dca5ab68d42ddea2"
    assert keys[:7] == ["net_q1.net.0.weight", "net_q1.net.0.bias", "net_q1.net.1.weight", "net_q1.net.1.bias", "net_q1.net.3.weight",
                        "net_q1.net.3.bias", "net_q1.net.4.weight"]
    assert keys[28:31] == ["net_q1.net.1.running_mean", "net_q1.net.1.running_var", "net_q1.net.1.num_batches_tracked"]
    assert (q.arena.numel(), q.stats.numel(), q.num_batches_tracked.numel()) == (366144, 3584, 6)
    big = DoubleQBatchNorm((88,), 16, hidden_layers=[512, 512, 256])
    assert (big.arena.numel(), big.stats.numel()) == (925760, 5120)
    assert sorted(k for k, _ in q.named_buffers()) == ["num_batches_tracked", "stats"]


# --------------------------------------------------------------------------- refusals: before anything is allocated (env = None)
def _script(name):
    return load_script(f"scripts/{name}.py", name)


def test_pql_learners_refuse_the_layernorm_critic():
    from pql_amd.algo.pql_p_learner import PQLPLearner
    from pql_amd.algo.pql_v_learner import PQLVLearner
    cfg = _cfg("pql_algo", "algo.cri_class=DoubleQLayerNorm")
    for make in (lambda: PQLVLearner((8,), 2, cfg), lambda: PQLPLearner((8,), 2, cfg), lambda: _script("train_pql").main(cfg)):
        with pytest.raises(ValueError, match=r"algo\.cri_class=DoubleQLayerNorm.*ddpg_algo.*sac_algo"):
            make()


@pytest.mark.parametrize("algo", ["ddpg_algo", "sac_algo"])
def test_distl_refused_with_the_layernorm_critic(algo):
    from pql_amd.algo.ddpg import AgentDDPG
    from pql_amd.algo.sac import AgentSAC
    cfg = _cfg(algo, "algo.cri_class=DoubleQLayerNorm", "algo.distl=True")
    with pytest.raises(ValueError, match=r"algo\.distl"):
        (AgentDDPG if algo == "ddpg_algo" else AgentSAC)(None, cfg)


@pytest.mark.parametrize("cri", ["DoubleQLayerNorm", "DoubleQ"])
def test_crossq_refuses_other_critics(cri):
    from pql_amd.algo.crossq import AgentCrossQ
    with pytest.raises(ValueError, match=rf"algo\.cri_class=DoubleQBatchNorm.*{cri}"):
        AgentCrossQ(None, _cfg("crossq_algo", f"algo.cri_class={cri}"))


def test_resume_mismatch_names_both_classes():
    from pql_amd.utils import checkpoint as CK
    saved = CK.structure(_cfg("ddpg_algo", "algo.cri_class=DoubleQLayerNorm"), 8, 2)
    have = CK.structure(_cfg("ddpg_algo"), 8, 2)
    assert saved["algo.cri_class"] == "DoubleQLayerNorm"
    with pytest.raises(ValueError, match=r"algo\.cri_class='DoubleQ' .*algo\.cri_class='DoubleQLayerNorm'"):
        CK.check_structure(saved, have)


def test_configs_show_the_key_and_keep_their_defaults():
    for name in ("ddpg_algo", "sac_algo"):
        text = open(os.path.join(ROOT, "pql_amd", "cfg", "algo", f"{name}.yaml")).read()
        assert re.search(r"#.*cri_class.*DoubleQLayerNorm", text), name
        assert _cfg(name).algo.cri_class == "DoubleQ"
    from pql_amd.models import model_name_to_path
    assert "DoubleQLayerNorm" in model_name_to_path and "NormTwinQ" in model_name_to_path
