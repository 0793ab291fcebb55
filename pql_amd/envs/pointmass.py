"""PointMass: a learnable vectorised task with the env contract of `SyntheticVecEnv` (pql_amd/envs/synthetic.py).

A damped point mass in A dimensions is pushed towards a goal:

    a   = clamp(action, -1, 1)
    v'  = 0.8 v + 0.2 a
    x'  = x + 0.25 v'
    k'  = k + 1
    d2  = (1/A) sum_j (x'_j - g_j)^2                  summed in index order j = 0 .. A-1
    oob = any_j |x'_j| > 1.5
    reward    = -d2 - 0.01 (1/A) sum_j a_j^2 - (1 if oob else 0)
    truncated = k' >= episode_length and not oob
    done      = oob or truncated
    info channels (`info_channels=True`): dist2 = d2, oob = 1.0 if oob else 0.0

Every written operation is one fp32 rounding (no fused multiply-add), and nothing is transcendental, so the HIP step
(`pqlk_pointmass_step`, pql_amd/csrc/pointmass.hip) is bit-equal to `_step_torch`, which is the definition and the CPU /
`PQL_SYNTH_TORCH` form.  Everything but the transition and the reset draw is `HashResetVecEnv`
(pql_amd/envs/base.py).  Envs that are done advance their episode index and are reset before the step returns (Isaac-Gym
style): the `next_obs` of a done transition is the first observation of the new episode, and
`info["TimeLimit.truncated"]` says which of the dones were time limits.

Resets are a pure function of (seed, global env id, episode index): x_j = 2 u(e, ep, 11, j) - 1, g_j = 2 u(e, ep, 12, j) - 1
with the hash-based uniform of the synthetic env (the episode index in the place of the step), v = 0, k = 0 -- so
data-parallel shards reproduce slices of the global env.  obs = [x | v | g | 0 ... 0]; obs_dim >= 3 act_dim.
"""
from __future__ import annotations

import torch

from pql_amd.envs.base import HashResetVecEnv

STREAM_X, STREAM_G = 11, 12
OOB = 1.5


class PointMassVecEnv(HashResetVecEnv):
    """The task's part of a hash-reset env (pql_amd/envs/base.py holds the rest)."""
    _STATE = ("x", "v", "g")
    _ENTRY = "pqlk_pointmass_step"
    _LAYOUT = "[x | v | g | 0 ...]"
    _EPISODE_LENGTH = 64
    info_keys = ("dist2", "oob")   # of the step just taken: the reward's own d2, and 1.0 where the step left the box

    def _reset_values(self, ep):
        """(x, v, g) at the start of episode `ep` (N,) of every env."""
        x0 = 2.0 * self._uniform(ep, STREAM_X) - 1.0
        return x0, torch.zeros_like(x0), 2.0 * self._uniform(ep, STREAM_G) - 1.0

    def _advance(self, a):
        v = 0.8 * self.v + 0.2 * a
        x = self.x + 0.25 * v
        diff = x - self.g
        d2 = self._sum_in_order(diff * diff) * self.inv_a
        a2 = self._sum_in_order(a * a) * self.inv_a
        oob = (x.abs() > OOB).any(dim=1)
        if self.info_channels:
            self._info_step = (d2, oob.to(torch.float32))
        return (x, v, self.g), -d2 - 0.01 * a2 - oob.to(torch.float32), oob


# ---- yardsticks: two hand-written controllers that bracket what a learner can reach -------------------
def zero_policy(env):
    """a = 0: the mass stays where the reset put it."""
    return lambda obs: torch.zeros((obs.shape[0], env.act_dim), dtype=torch.float32, device=obs.device)


def pd_policy(env):
    """a = clamp(4 (g - x) - 4 v, -1, 1), read off the observation."""
    A = env.act_dim
    return lambda obs: (4.0 * (obs[:, 2 * A:3 * A] - obs[:, :A]) - 4.0 * obs[:, A:2 * A]).clamp(-1.0, 1.0)


@torch.no_grad()
def episode_return(env, policy):
    """Mean over the envs of the return of ONE episode each, from `env.reset()` to the env's first done, under
    `policy(obs) -> action` (a python float: this synchronises)."""
    obs = env.reset()
    ret = torch.zeros(env.num_envs, dtype=torch.float32, device=obs.device)
    alive = torch.ones(env.num_envs, dtype=torch.bool, device=obs.device)
    for _ in range(env.max_episode_length):
        obs, reward, done, _ = env.step(policy(obs))
        ret += reward * alive
        alive &= ~done
    return float(ret.mean())
