"""`HashResetVecEnv` (pql_amd/envs/base.py) carries a task it has never seen: a toy third task written here on top of it, in torch
only, gets hash resets, sharding of the env axis and the state round trip from the base's code alone."""
import numpy as np
import pytest
import torch

from pql_amd.envs.base import HashResetVecEnv
from task_cases import u_np

F = np.float32


class DriftVecEnv(HashResetVecEnv):
    """x' = x + 0.1 a, reward = -mean |x'|, no terminal; y keeps the clamped action, z the start.  obs = [x | y | z | 0 ...]."""
    _STATE = ("x", "y", "z")
    _LAYOUT = "[x | y | z | 0 ...]"
    _EPISODE_LENGTH = 5

    def _reset_values(self, ep):
        x0 = 2.0 * self._uniform(ep, 21) - 1.0
        return x0, torch.zeros_like(x0), x0

    def _advance(self, a):
        x = self.x + 0.1 * a
        return (x, a, self.z), -(self._sum_in_order(x.abs()) * self.inv_a), None


def _acts(n, A, steps):
    g = torch.Generator().manual_seed(0)
    return [3.0 * (2.0 * torch.rand((n, A), generator=g) - 1.0) for _ in range(steps)]


def _same(p, q):
    return all(torch.equal(a, b) for a, b in zip(p[:3], q[:3])) and torch.equal(p[3]["TimeLimit.truncated"], q[3]["TimeLimit.truncated"])


def test_a_toy_task_runs_on_the_base_alone():
    mk = lambda n, off: DriftVecEnv(n, 7, 2, device="cpu", seed=9, env_offset=off)   # noqa: E731
    full, shards = mk(12, 3), [mk(5, 3), mk(7, 8)]
    assert full.max_episode_length == 5 and full.observation_space.shape == (7,) and full.action_space.shape == (2,)
    # reset = the plain-integer hash
    obs = full.reset()
    want = np.zeros((12, 7), dtype=np.float32)
    for i in range(12):
        for j in range(2):
            want[i, j] = want[i, 4 + j] = F(2.0) * u_np(9, 3 + i, 0, 21, j) - F(1.0)
    assert torch.equal(obs, torch.from_numpy(want))
    assert torch.equal(obs, torch.cat([s.reset() for s in shards]))
    # two shards reproduce slices of the global env over 12 steps (two resets on the way); the state travels after step 7
    acts, fresh = _acts(12, 2, 12), mk(12, 3)
    for t, act in enumerate(acts):
        x_prev, z_prev = full.x.clone(), full.z.clone()
        out = full.step(act)
        parts = [s.step(a) for s, a in zip(shards, (act[:5], act[5:]))]
        assert _same(out, tuple(torch.cat([p[i] for p in parts]) for i in range(3)) + ({"TimeLimit.truncated": torch.cat(
            [p[3]["TimeLimit.truncated"] for p in parts])},))
        assert torch.equal(out[2], out[3]["TimeLimit.truncated"]) and bool(out[2].all()) == ((t + 1) % 5 == 0) == bool(out[2].any())
        if not out[2].any():                                         # the toy transition itself, where no reset hides it
            assert torch.equal(out[0][:, :2], x_prev + 0.1 * act.clamp(-1.0, 1.0)) and torch.equal(out[0][:, 2:4], act.clamp(-1.0, 1.0))
            assert torch.equal(out[1], -(out[0][:, :2].abs().sum(1) * F(0.5)))
        else:
            assert torch.equal(out[0][:, :2], full.z) and not torch.equal(full.z, z_prev)
        if t == 6:
            state = full.state_dict()
            assert set(state) == {"x", "y", "z", "k", "ep", "seed", "num_envs", "env_offset"}
            fresh.load_state_dict(state)
        elif t > 6:
            assert _same(out, fresh.step(act))
    assert torch.equal(full.ep, torch.full((12,), 2, dtype=torch.int32)) and torch.equal(full.k, torch.full((12,), 2, dtype=torch.int32))
    for name in ("x", "y", "z", "k", "ep"):
        assert torch.equal(getattr(full, name), getattr(fresh, name)), name
        assert torch.equal(getattr(full, name), torch.cat([getattr(s, name) for s in shards])), name
    # the base's errors carry the task's own name and layout
    with pytest.raises(ValueError, match=r"DriftVecEnv: obs = \[x \| y \| z \| 0 \.\.\.\] needs obs_dim >= 3 \* act_dim"):
        DriftVecEnv(4, 5, 2, device="cpu")
    with pytest.raises(ValueError, match="DriftVecEnv.load_state_dict: env_offset=4"):
        mk(12, 4).load_state_dict(state)
