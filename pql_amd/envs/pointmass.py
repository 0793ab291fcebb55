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

Every written operation is one fp32 rounding (no fused multiply-add), and nothing is transcendental, so the HIP step
(`pqlk_pointmass_step`, pql_amd/csrc/pointmass.hip) is bit-equal to `_step_torch`, which is the definition and the CPU /
`PQL_SYNTH_TORCH` form.  Envs that are done advance their episode index and are reset before the step returns (Isaac-Gym
style): the `next_obs` of a done transition is the first observation of the new episode, and
`info["TimeLimit.truncated"]` says which of the dones were time limits.

Resets are a pure function of (seed, global env id, episode index): x_j = 2 u(e, ep, 11, j) - 1, g_j = 2 u(e, ep, 12, j) - 1
with the hash-based uniform of the synthetic env (the episode index in the place of the step), v = 0, k = 0 -- so
data-parallel shards reproduce slices of the global env.  obs = [x | v | g | 0 ... 0]; obs_dim >= 3 act_dim.
"""
from __future__ import annotations

import os
from types import SimpleNamespace

import numpy as np
import torch

from pql_amd.envs.synthetic import _hash32

STREAM_X, STREAM_G = 11, 12
OOB = 1.5


class PointMassVecEnv:
    def __init__(self, num_envs, obs_dim, act_dim, device="cuda", seed=42, episode_length=64, env_offset=0):
        self.num_envs, self.obs_dim, self.act_dim = int(num_envs), int(obs_dim), int(act_dim)
        if self.act_dim <= 0 or self.obs_dim < 3 * self.act_dim:
            raise ValueError(f"PointMassVecEnv: obs = [x | v | g | 0 ...] needs obs_dim >= 3 * act_dim, got obs_dim={self.obs_dim}, "
                             f"act_dim={self.act_dim}")
        self.device = torch.device(device)
        self.seed = int(seed)
        self.max_episode_length = int(episode_length)
        self.observation_space = SimpleNamespace(shape=(self.obs_dim,))
        self.action_space = SimpleNamespace(shape=(self.act_dim,))
        self.env_offset = int(env_offset)
        self.env_ids = torch.arange(self.num_envs, device=self.device, dtype=torch.int64) + self.env_offset
        self.inv_a = float(np.float32(1.0) / np.float32(self.act_dim))   # the fp32 constant 1.0f / A, in both forms
        n, A, dev = self.num_envs, self.act_dim, self.device
        self.x = torch.zeros((n, A), dtype=torch.float32, device=dev)
        self.v = torch.zeros((n, A), dtype=torch.float32, device=dev)
        self.g = torch.zeros((n, A), dtype=torch.float32, device=dev)
        self.k = torch.zeros(n, dtype=torch.int32, device=dev)
        self.ep = torch.zeros(n, dtype=torch.int32, device=dev)
        self._start(self.ep)

    # ---- resets ------------------------------------------------------------------------------------
    def _uniform(self, ep, stream):
        """(N, A) uniforms in (0, 1]: `SyntheticVecEnv._uniform` with the per-env episode index in the place of the step."""
        col = torch.arange(self.act_dim, device=self.device, dtype=torch.int64)
        key = _hash32(self.env_ids * 0x9E3779B1 + ((self.seed * 0x85EBCA77) & 0xFFFFFFFF) + (ep.to(torch.int64) & 0xFFFFFFFF) * 0xC2B2AE3D
                      + stream * 0x27D4EB2F)
        h = _hash32(key.unsqueeze(1) * 0x165667B1 + col.unsqueeze(0) * 0x9E3779B1 + 0x5BD1E995)
        return (h.to(torch.float32) + 0.5) * (1.0 / 4294967296.0)

    def _reset_values(self, ep):
        """(x, g) at the start of episode `ep` (N,) of every env."""
        return 2.0 * self._uniform(ep, STREAM_X) - 1.0, 2.0 * self._uniform(ep, STREAM_G) - 1.0

    def _start(self, ep):
        x0, g0 = self._reset_values(ep)
        self.x.copy_(x0)
        self.g.copy_(g0)
        self.v.zero_()
        self.k.zero_()

    def _observe(self):
        obs = torch.zeros((self.num_envs, self.obs_dim), dtype=torch.float32, device=self.device)
        A = self.act_dim
        obs[:, :A], obs[:, A:2 * A], obs[:, 2 * A:3 * A] = self.x, self.v, self.g
        return obs

    @torch.no_grad()
    def reset(self):
        """Every env back to the start of its episode 0."""
        self.ep.zero_()
        self._start(self.ep)
        return self._observe()

    # ---- state -------------------------------------------------------------------------------------
    _STATE = ("x", "v", "g", "k", "ep")

    def state_dict(self):
        """Everything the next transitions depend on besides the constructor arguments."""
        out = {name: getattr(self, name).detach().clone() for name in self._STATE}
        out.update(seed=self.seed, num_envs=self.num_envs, env_offset=self.env_offset)
        return out

    def load_state_dict(self, state):
        for key in ("seed", "num_envs", "env_offset"):
            if int(state[key]) != getattr(self, key):
                raise ValueError(f"{type(self).__name__}.load_state_dict: {key}={getattr(self, key)} but the state was saved with {int(state[key])}")
        for name in self._STATE:
            mine = getattr(self, name)
            if tuple(state[name].shape) != tuple(mine.shape):
                raise ValueError(f"{type(self).__name__}.load_state_dict: {name} has shape {tuple(mine.shape)} but the state holds {tuple(state[name].shape)}")
            mine.copy_(state[name].to(self.device, mine.dtype))

    # ---- step --------------------------------------------------------------------------------------
    @torch.no_grad()
    def step(self, action):
        if self.device.type == "cuda" and not os.environ.get("PQL_SYNTH_TORCH"):   # one HIP launch instead of ~40 torch launches
            return self._step_hip(action)
        return self._step_torch(action)

    @staticmethod
    def _sum_in_order(t):
        """Row sums of (N, A) taken column by column, j = 0 .. A-1 (torch's own `.sum(1)` reorders)."""
        s = t[:, 0]
        for j in range(1, t.shape[1]):
            s = s + t[:, j]
        return s

    def _step_torch(self, action):
        a = action.to(torch.float32).clamp(-1.0, 1.0)
        v = 0.8 * self.v + 0.2 * a
        x = self.x + 0.25 * v
        k = self.k + 1
        diff = x - self.g
        d2 = self._sum_in_order(diff * diff) * self.inv_a
        a2 = self._sum_in_order(a * a) * self.inv_a
        oob = (x.abs() > OOB).any(dim=1)
        reward = -d2 - 0.01 * a2 - oob.to(torch.float32)
        truncated = (k >= self.max_episode_length) & ~oob
        done = oob | truncated
        # auto-reset of the finished envs: next episode's start, drawn from the hash
        ep = self.ep + done.to(torch.int32)
        x0, g0 = self._reset_values(ep)
        d = done.unsqueeze(1)
        self.x = torch.where(d, x0, x)
        self.g = torch.where(d, g0, self.g)
        self.v = torch.where(d, torch.zeros_like(v), v)
        self.k = torch.where(done, torch.zeros_like(k), k)
        self.ep = ep
        return self._observe(), reward, done, {"TimeLimit.truncated": truncated}

    def _step_hip(self, action):
        """Same transition as `_step_torch`, one launch (`pqlk_pointmass_step`, include/pqlk.h): state updated in place."""
        from pql_amd import _lib as L
        n, dev = self.num_envs, self.device
        next_obs = torch.empty((n, self.obs_dim), dtype=torch.float32, device=dev)
        reward = torch.empty(n, dtype=torch.float32, device=dev)
        done = torch.empty(n, dtype=torch.bool, device=dev)
        truncated = torch.empty(n, dtype=torch.bool, device=dev)
        act = action.to(dev, torch.float32).contiguous()
        if tuple(act.shape) != (n, self.act_dim):
            raise ValueError(f"PointMassVecEnv.step: action has shape {tuple(act.shape)}, expected {(n, self.act_dim)}")
        with torch.cuda.device(dev):
            L.check(L.lib.pqlk_pointmass_step(n, self.obs_dim, self.act_dim, self.seed & 0xFFFFFFFF, self.env_offset & 0xFFFFFFFF,
                                              self.max_episode_length, L.ptr(act), L.ptr(self.x), L.ptr(self.v), L.ptr(self.g),
                                              L.ptr(self.k), L.ptr(self.ep), L.ptr(next_obs), L.ptr(reward), L.ptr(done),
                                              L.ptr(truncated), L.stream(dev)))
        return next_obs, reward, done, {"TimeLimit.truncated": truncated}


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
