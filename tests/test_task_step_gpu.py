"""The shared step template (pql_amd/csrc/taskstep.h) for both tasks at the shapes where its column decode can go wrong and that
the tasks' own four-shape tests do not reach.  Run with `pytest -m gpu`."""
import pytest
import torch

import task_cases as tc

pytestmark = pytest.mark.gpu


# one env, O = 3 A, scalar stores | exactly one full tile, O = 3 A, 16-byte stores | a one-row second tile and a wrapping global env id
@pytest.mark.parametrize("n,O,A,off", [(1, 3, 1, 0), (256, 12, 4, 0), (257, 12, 4, 2 ** 32 - 100)])
@pytest.mark.parametrize("kind", ["pointmass", "swingup"])
def test_task_step_equals_torch_definition_at_the_template_edges(kind, n, O, A, off):
    """The HIP step vs `_step_torch` on the same device, episode_length = 5: observations, rewards, dones, truncations and all five
    state tensors bit-equal after each of 12 steps.  (No coverage counters: one env cannot meet them.)"""
    from pql_amd.envs.synthetic import TASK_ENVS
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    dev = torch.device("cuda:0")
    a = TASK_ENVS[kind](n, O, A, device=dev, seed=1234, episode_length=5, env_offset=off)
    b = TASK_ENVS[kind](n, O, A, device=dev, seed=1234, episode_length=5, env_offset=off)
    assert torch.equal(a.reset(), b.reset())
    for act in tc.task_actions(n, A, 12):
        act = act.to(dev)
        oa, ra, da, ia = a.step(act)                 # the HIP launch
        ob, rb, db, ib = b._step_torch(act)          # the definition
        assert torch.equal(oa, ob) and torch.equal(ra, rb) and torch.equal(da, db)
        assert torch.equal(ia["TimeLimit.truncated"], ib["TimeLimit.truncated"])
        for name in (*a._STATE, "k", "ep"):
            assert torch.equal(getattr(a, name), getattr(b, name)), name
