"""Reacher: a coupled learnable vectorised task with the env contract of `PointMassVecEnv` (pql_amd/envs/pointmass.py).

A planar arm of A links of length 1 / A per env, one joint per action column; its tip has to reach the fixed point (0.6, 0).
Joint j is held as (c, s) = (cos, sin) of its angle relative to link j - 1 (joint 0: relative to the world x axis) and its angular
velocity w.  The joint dynamics are per joint, but the reward and two observation columns go through the forward kinematics of the
whole chain, so -- unlike PointMass and SwingUp -- the best action of a joint depends on all the others:

    rot(c, s, d):                                  `_rot` of pql_amd/envs/swingup.py, unchanged; |d| <= 0.5

    a   = clamp(action, -1, 1)
    w'  = clamp(0.9 w + 0.3 a, -3, 3)
    (c', s') = rot(c, s, 0.05 w')                  |0.05 w'| <= 0.15

    tip(c, s):  C = c_0, S = s_0, x = C, y = S
                for j = 1 .. A-1:  (C, S) = (C c_j - S s_j, S c_j + C s_j)  (both from the old C, S);  x = x + C;  y = y + S
                ex = x (1/A) - 0.6 ;  ey = y (1/A)

    (ex, ey) = tip(c', s') ;  d2 = ex ex + ey ey
    cost   = (d2 + 0.01 ((sum_j w'_j w'_j) (1/A))) + 0.01 ((sum_j a_j a_j) (1/A))     sums in index order j = 0 .. A-1
    reward = -(0.05 cost)
    k'  = k + 1 ;  truncated = k' >= episode_length ;  done = truncated
    info channels (`info_channels=True`): tip_dist2 = d2, effort = (sum_j a_j a_j) (1/A), reached = 1.0 where d2 < 0.01 else 0.0

There is no terminal and no gravity: the speed is clamped, and every done is a time limit.  The goal is fixed; a uniformly random
first-joint angle is the same problem as a random goal direction.  Doing nothing costs 0.02 to 0.045 per step on average (R_zero =
-1.34 at (88, 16) and -2.88 at (8, 2) over 64 steps), so with gamma = 0.99 its discounted return is about -2 to -5: the default C51
support [-10, 10] holds it.

No transcendental function, no division, no square root, and every written operation is one fp32 rounding (no fused multiply-add),
so the HIP step (`pqlk_reacher_step`, pql_amd/csrc/reacher.hip) is bit-equal to `_step_torch`, which is the definition and the
CPU / `PQL_SYNTH_TORCH` form.  Everything but the transition, the reset draw and the observation is `HashResetVecEnv`
(pql_amd/envs/base.py).  Envs that are done advance their episode index and are reset before the step returns: the `next_obs` of a
done transition is the first observation of the new episode, and `info["TimeLimit.truncated"]` equals done.

Resets are a pure function of (seed, global env id, episode index), with the hash-based uniform u of the synthetic env (the episode
index in the place of the step): d = 0.5 (2 u(e, ep, 15, j) - 1), (c, s) = rot applied 6 times to (1, 0) with that d (up to +-3
rad), w = 0.5 (2 u(e, ep, 16, j) - 1), k = 0 -- so data-parallel shards reproduce slices of the global env.
obs = [c | s | 0.25 w | ex | ey | 0 ... 0] with (ex, ey) = tip of the state the row describes (after a reset: of the new episode);
obs_dim >= 3 act_dim + 2.
"""
from __future__ import annotations

import torch

from pql_amd.envs.base import HashResetVecEnv
from pql_amd.envs.pointmass import episode_return  # noqa: F401  (the yardsticks' measure is PointMass's)
from pql_amd.envs.swingup import _rot

STREAM_TH, STREAM_W = 15, 16
W_MAX = 3.0
GOAL_X = 0.6
REACHED_D2 = 0.01


def _chain(c, s):
    """[(C_j, S_j)], j = 0 .. A-1: the direction of link j, the angle sum by the addition theorems, both from the old C, S."""
    C, S = c[:, 0], s[:, 0]
    out = [(C, S)]
    for j in range(1, c.shape[1]):
        C, S = C * c[:, j] - S * s[:, j], S * c[:, j] + C * s[:, j]
        out.append((C, S))
    return out


def _tip(c, s, inv_a):
    """(ex, ey): the tip of the chain minus the goal, the link directions summed in index order."""
    links = _chain(c, s)
    x, y = links[0]
    for C, S in links[1:]:
        x, y = x + C, y + S
    return x * inv_a - GOAL_X, y * inv_a


class ReacherVecEnv(HashResetVecEnv):
    """The task's part of a hash-reset env (pql_amd/envs/base.py holds the rest)."""
    _STATE = ("c", "s", "w")
    _ENTRY = "pqlk_reacher_step"
    _LAYOUT = "[c | s | w / 4 | ex | ey | 0 ...]"
    _EPISODE_LENGTH = 64
    info_keys = ("tip_dist2", "effort", "reached")   # of the step just taken: d2, the mean of a^2, and 1.0 where d2 < 0.01

    def __init__(self, num_envs, obs_dim, act_dim, *args, **kwargs):
        if int(act_dim) <= 0 or int(obs_dim) < 3 * int(act_dim) + 2:   # (before anything touches the device)
            raise ValueError(f"{type(self).__name__}: obs = {self._LAYOUT} needs obs_dim >= 3 * act_dim + 2, got obs_dim={int(obs_dim)}, "
                             f"act_dim={int(act_dim)}")
        super().__init__(num_envs, obs_dim, act_dim, *args, **kwargs)

    def _reset_values(self, ep):
        """(c, s, w) at the start of episode `ep` (N,) of every env."""
        d = 0.5 * (2.0 * self._uniform(ep, STREAM_TH) - 1.0)
        c, s = torch.ones_like(d), torch.zeros_like(d)
        for _ in range(6):
            c, s = _rot(c, s, d)
        return c, s, 0.5 * (2.0 * self._uniform(ep, STREAM_W) - 1.0)

    def _obs_blocks(self):
        return self.c, self.s, 0.25 * self.w

    def _observe(self):
        obs = super()._observe()
        A = self.act_dim
        obs[:, 3 * A], obs[:, 3 * A + 1] = _tip(self.c, self.s, self.inv_a)
        return obs

    def _advance(self, a):
        w = (0.9 * self.w + 0.3 * a).clamp(-W_MAX, W_MAX)
        c, s = _rot(self.c, self.s, 0.05 * w)
        ex, ey = _tip(c, s, self.inv_a)
        d2 = ex * ex + ey * ey
        effort = self._sum_in_order(a * a) * self.inv_a
        cost = (d2 + 0.01 * (self._sum_in_order(w * w) * self.inv_a)) + 0.01 * effort
        if self.info_channels:
            self._info_step = (d2, effort, (d2 < REACHED_D2).to(torch.float32))
        return (c, s, w), -(0.05 * cost), None   # no terminal: every done is a time limit


# ---- yardsticks: two hand-written controllers that bracket what a learner can reach -------------------
def zero_policy(env):
    """a = 0: the arm coasts to rest where the reset put it."""
    return lambda obs: torch.zeros((obs.shape[0], env.act_dim), dtype=torch.float32, device=obs.device)


def jacobian_policy(env):
    """A Jacobian-transpose law read off the observation (w = 4 obs_w): with (tx_j, ty_j) = sum_{i >= j} (C_i, S_i) / A the vector from
    joint j to the tip, g_j = ex (-ty_j) + ey tx_j is the derivative of d2 / 2 by joint j's angle, and
    a = clamp(-8 A g - w, -1, 1)."""
    A = env.act_dim

    def policy(obs):
        c, s, w = obs[:, :A], obs[:, A:2 * A], 4.0 * obs[:, 2 * A:3 * A]
        ex, ey = obs[:, 3 * A:3 * A + 1], obs[:, 3 * A + 1:3 * A + 2]
        links = _chain(c, s)
        C, S = torch.stack([l[0] for l in links], 1), torch.stack([l[1] for l in links], 1)
        tx = C.flip(1).cumsum(1).flip(1) / A
        ty = S.flip(1).cumsum(1).flip(1) / A
        g = ex * (-ty) + ey * tx
        return (-8.0 * A * g - w).clamp(-1.0, 1.0)
    return policy
