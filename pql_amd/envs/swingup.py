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
    info channels (`info_channels=True`): upright = (sum_j c'_j) (1/A), effort = (sum_j a_j a_j) (1/A), summed in index order

There is no terminal: the speed is clamped instead (an episode that can be ended early is ended on purpose by a learner that finds
hanging more expensive than the end).  A pendulum at rest hanging costs 0.05 * 2 = 0.1 per step, so with gamma = 0.99 the
discounted return of doing nothing is about -10: the default C51 support [-10, 10] holds it.

No transcendental function, no division, no square root, and every written operation is one fp32 rounding (no fused multiply-add),
so the HIP step (`pqlk_swingup_step`, pql_amd/csrc/swingup.hip) is bit-equal to `_step_torch`, which is the definition and the
CPU / `PQL_SYNTH_TORCH` form.  Everything but the transition, the reset draw and the observation blocks is `HashResetVecEnv`
(pql_amd/envs/base.py).  Envs that are done advance their episode index and are reset before the step returns: the
`next_obs` of a done transition is the first observation of the new episode, and `info["TimeLimit.truncated"]` equals done.

Resets are a pure function of (seed, global env id, episode index), with the hash-based uniform u of the synthetic env (the episode
index in the place of the step): d = 0.5 (2 u(e, ep, 13, j) - 1), (c, s) = rot applied 4 times to (-1, 0) with that d (up to
+-2 rad away from hanging), w = 2 u(e, ep, 14, j) - 1, k = 0 -- so data-parallel shards reproduce slices of the global env.
obs = [c | s | 0.125 w | 0 ... 0]; obs_dim >= 3 act_dim.
"""
from __future__ import annotations

import torch

from pql_amd.envs.base import HashResetVecEnv
from pql_amd.envs.pointmass import episode_return  # noqa: F401  (the yardsticks' measure is PointMass's)

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


class SwingUpVecEnv(HashResetVecEnv):
    """The task's part of a hash-reset env (pql_amd/envs/base.py holds the rest)."""
    _STATE = ("c", "s", "w")
    _ENTRY = "pqlk_swingup_step"
    _LAYOUT = "[c | s | w / 8 | 0 ...]"
    _EPISODE_LENGTH = 128
    info_keys = ("upright", "effort")   # of the step just taken: the means over the joints of c' and of a^2

    def _reset_values(self, ep):
        """(c, s, w) at the start of episode `ep` (N,) of every env."""
        d = 0.5 * (2.0 * self._uniform(ep, STREAM_TH) - 1.0)
        c, s = torch.full_like(d, -1.0), torch.zeros_like(d)
        for _ in range(4):
            c, s = _rot(c, s, d)
        return c, s, 2.0 * self._uniform(ep, STREAM_W) - 1.0

    def _obs_blocks(self):
        return self.c, self.s, 0.125 * self.w

    def _advance(self, a):
        w = (self.w + 0.05 * (15.0 * self.s + 6.0 * a)).clamp(-W_MAX, W_MAX)
        c, s = _rot(self.c, self.s, 0.05 * w)
        cost = ((1.0 - c) + 0.01 * (w * w)) + 0.01 * (a * a)
        if self.info_channels:
            self._info_step = (self._sum_in_order(c) * self.inv_a, self._sum_in_order(a * a) * self.inv_a)
        return (c, s, w), -(0.05 * (self._sum_in_order(cost) * self.inv_a)), None   # no terminal: every done is a time limit


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
