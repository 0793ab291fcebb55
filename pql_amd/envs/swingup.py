"""SwingUp: a nonlinear, under-actuated learnable vectorised task with the env contract of `PointMassVecEnv`
(pql_amd/envs/pointmass.py).

A independent torque-limited pendulums per env, one per action column.  Joint j is held as (c, s) = (cos, sin) of its angle from
upright and its angular velocity w; gravity (15 sin) beats the torque (6 a), so the pendulum has to be swung up:

    rot(c, s, d):                                  rotate (c, s) by the angle d, |d| <= 0.5
        d2 = d d
        cd = 1 - d2 (0.5 - d2 C4)                  C4 = 0.041666668  (1/24)
        sd = d (1 - d2 (S3 - d2 S5))               S3 = 0.16666667, S5 = 0.008333334
        cn = c cd - s sd ;  sn = s cd + c sd
        m  = 1.5 - 0.5 (cn cn + sn sn)             one Newton step back to the unit circle
        return cn m, sn m

    a   = clamp(action, -1, 1)
    w'  = clamp(w + 0.05 (15 s + 6 a), -8, 8)
    (c', s') = rot(c, s, 0.05 w')
    cost_j = ((1 - c') + 0.01 (w' w')) + 0.01 (a a)
    reward    = -(0.05 ((sum_j cost_j) (1/A)))     summed in index order j = 0 .. A-1
    k'  = k + 1 ;  truncated = k' >= episode_length ;  done = truncated

There is no terminal: the speed is clamped instead (an episode that can be ended early is ended on purpose by a learner that finds
hanging more expensive than the end).  A pendulum at rest hanging costs 0.05 * 2 = 0.1 per step, so with gamma = 0.99 the
discounted return of doing nothing is about -10: the default C51 support [-10, 10] holds it.

No transcendental function, no division, no square root, and every written operation is one fp32 rounding (no fused multiply-add),
so the HIP step (`pqlk_swingup_step`, pql_amd/csrc/swingup.hip) is bit-equal to `_step_torch`, which is the definition and the
CPU / `PQL_SYNTH_TORCH` form.  Envs that are done advance their episode index and are reset before the step returns: the
`next_obs` of a done transition is the first observation of the new episode, and `info["TimeLimit.truncated"]` equals done.

Resets are a pure function of (seed, global env id, episode index), with the hash-based uniform u of the synthetic env (the episode
index in the place of the step): d = 0.5 (2 u(e, ep, 13, j) - 1), (c, s) = rot applied 4 times to (-1, 0) with that d (up to
+-2 rad away from hanging), w = 2 u(e, ep, 14, j) - 1, k = 0 -- so data-parallel shards reproduce slices of the global env.
obs = [c | s | 0.125 w | 0 ... 0]; obs_dim >= 3 act_dim.
"""
from __future__ import annotations

import os
from types import SimpleNamespace

import numpy as np
import torch

from pql_amd.envs.pointmass import PointMassVecEnv, episode_return  # noqa: F401  (the yardsticks' measure is PointMass's)

STREAM_TH, STREAM_W = 13, 14
C4, S3, S5 = 0.041666668, 0.16666667, 0.008333334
W_MAX = 8.0


def _rot(c, s, d):
    """(c, s) rotated by d (|d| <= 0.5), one fp32 rounding per written operation."""
    d2 = d * d
    cd = 1.0 - d2 * (0.5 - d2 * C4)
    sd = d * (1.0 - d2 * (S3 - d2 * S5))
    cn = c * cd - s * sd
    sn = s * cd + c * sd
    m = 1.5 - 0.5 * (cn * cn + sn * sn)
    return cn * m, sn * m


class SwingUpVecEnv:
    def __init__(self, num_envs, obs_dim, act_dim, device="cuda", seed=42, episode_length=128, env_offset=0):
        self.num_envs, self.obs_dim, self.act_dim = int(num_envs), int(obs_dim), int(act_dim)
        if self.act_dim <= 0 or self.obs_dim < 3 * self.act_dim:
            raise ValueError(f"SwingUpVecEnv: obs = [c | s | w / 8 | 0 ...] needs obs_dim >= 3 * act_dim, got obs_dim={self.obs_dim}, "
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
        self.c = torch.zeros((n, A), dtype=torch.float32, device=dev)
        self.s = torch.zeros((n, A), dtype=torch.float32, device=dev)
        self.w = torch.zeros((n, A), dtype=torch.float32, device=dev)
        self.k = torch.zeros(n, dtype=torch.int32, device=dev)
        self.ep = torch.zeros(n, dtype=torch.int32, device=dev)
        self._start(self.ep)

    # ---- resets ------------------------------------------------------------------------------------
    _uniform = PointMassVecEnv._uniform   # (N, A) uniforms in (0, 1] keyed by (seed, global env id, episode, stream, column)

    def _reset_values(self, ep):
        """(c, s, w) at the start of episode `ep` (N,) of every env."""
        d = 0.5 * (2.0 * self._uniform(ep, STREAM_TH) - 1.0)
        c, s = torch.full_like(d, -1.0), torch.zeros_like(d)
        for _ in range(4):
            c, s = _rot(c, s, d)
        return c, s, 2.0 * self._uniform(ep, STREAM_W) - 1.0

    def _start(self, ep):
        c0, s0, w0 = self._reset_values(ep)
        self.c.copy_(c0)
        self.s.copy_(s0)
        self.w.copy_(w0)
        self.k.zero_()

    def _observe(self):
        obs = torch.zeros((self.num_envs, self.obs_dim), dtype=torch.float32, device=self.device)
        A = self.act_dim
        obs[:, :A], obs[:, A:2 * A], obs[:, 2 * A:3 * A] = self.c, self.s, 0.125 * self.w
        return obs

    @torch.no_grad()
    def reset(self):
        """Every env back to the start of its episode 0."""
        self.ep.zero_()
        self._start(self.ep)
        return self._observe()

    # ---- state -------------------------------------------------------------------------------------
    _STATE = ("c", "s", "w", "k", "ep")

    state_dict, load_state_dict = PointMassVecEnv.state_dict, PointMassVecEnv.load_state_dict   # over _STATE, same mismatch errors

    # ---- step --------------------------------------------------------------------------------------
    @torch.no_grad()
    def step(self, action):
        if self.device.type == "cuda" and not os.environ.get("PQL_SYNTH_TORCH"):   # one HIP launch instead of ~200 torch launches
            return self._step_hip(action)
        return self._step_torch(action)

    _sum_in_order = staticmethod(PointMassVecEnv._sum_in_order)

    def _step_torch(self, action):
        a = action.to(torch.float32).clamp(-1.0, 1.0)
        w = (self.w + 0.05 * (15.0 * self.s + 6.0 * a)).clamp(-W_MAX, W_MAX)
        c, s = _rot(self.c, self.s, 0.05 * w)
        cost = ((1.0 - c) + 0.01 * (w * w)) + 0.01 * (a * a)
        reward = -(0.05 * (self._sum_in_order(cost) * self.inv_a))
        k = self.k + 1
        truncated = k >= self.max_episode_length
        done = truncated.clone()
        # auto-reset of the finished envs: next episode's start, drawn from the hash
        ep = self.ep + done.to(torch.int32)
        c0, s0, w0 = self._reset_values(ep)
        d = done.unsqueeze(1)
        self.c = torch.where(d, c0, c)
        self.s = torch.where(d, s0, s)
        self.w = torch.where(d, w0, w)
        self.k = torch.where(done, torch.zeros_like(k), k)
        self.ep = ep
        return self._observe(), reward, done, {"TimeLimit.truncated": truncated}

    def _step_hip(self, action):
        """Same transition as `_step_torch`, one launch (`pqlk_swingup_step`, include/pqlk.h): state updated in place."""
        from pql_amd import _lib as L
        n, dev = self.num_envs, self.device
        next_obs = torch.empty((n, self.obs_dim), dtype=torch.float32, device=dev)
        reward = torch.empty(n, dtype=torch.float32, device=dev)
        done = torch.empty(n, dtype=torch.bool, device=dev)
        truncated = torch.empty(n, dtype=torch.bool, device=dev)
        act = action.to(dev, torch.float32).contiguous()
        if tuple(act.shape) != (n, self.act_dim):
            raise ValueError(f"SwingUpVecEnv.step: action has shape {tuple(act.shape)}, expected {(n, self.act_dim)}")
        with torch.cuda.device(dev):
            L.check(L.lib.pqlk_swingup_step(n, self.obs_dim, self.act_dim, self.seed & 0xFFFFFFFF, self.env_offset & 0xFFFFFFFF,
                                            self.max_episode_length, L.ptr(act), L.ptr(self.c), L.ptr(self.s), L.ptr(self.w),
                                            L.ptr(self.k), L.ptr(self.ep), L.ptr(next_obs), L.ptr(reward), L.ptr(done),
                                            L.ptr(truncated), L.stream(dev)))
        return next_obs, reward, done, {"TimeLimit.truncated": truncated}


# ---- yardsticks: two hand-written controllers that bracket what a learner can reach -------------------
def zero_policy(env):
    """a = 0: the pendulum swings about hanging."""
    return lambda obs: torch.zeros((obs.shape[0], env.act_dim), dtype=torch.float32, device=obs.device)


def energy_policy(env):
    """Energy pumping, then a PD law near upright, read off the observation (w = 8 obs_w): with E = 0.5 w^2 + 15 (c - 1) (zero at rest
    upright), a = clamp(-(5 s + 1.5 w), -1, 1) where c > 0.9 and |w| < 2.5, and a = clamp(-E w, -1, 1) elsewhere."""
    A = env.act_dim

    def policy(obs):
        c, s, w = obs[:, :A], obs[:, A:2 * A], 8.0 * obs[:, 2 * A:3 * A]
        energy = 0.5 * w * w + 15.0 * (c - 1.0)
        near = (c > 0.9) & (w.abs() < 2.5)
        return torch.where(near, -(5.0 * s + 1.5 * w), -energy * w).clamp(-1.0, 1.0)
    return policy
