"""What the vectorised envs share: the counter-based hash, the constructor fields and saved-state header of every env
(`VecEnvBase`), and the whole of a hash-reset task but the task itself (`HashResetVecEnv`: PointMass, SwingUp).

A hash-reset task holds three (N, A) float32 state tensors, a step count `k` and an episode index `ep` per env.  Envs that are
done advance their episode index and are reset before the step returns (Isaac-Gym style): the `next_obs` of a done transition is
the first observation of the new episode, and `info["TimeLimit.truncated"]` says which of the dones were time limits.  Resets are
a pure function of (seed, global env id, episode index) through `_uniform`, so data-parallel shards reproduce slices of the global
env.  obs = [the three state blocks | 0 ... 0]; obs_dim >= 3 act_dim.

A new task states
  * `_STATE` (the three attribute names, in the order of its entry point's arguments), `_ENTRY` (the `pqlk_*_step` of its
    csrc/<task>.hip, a task struct for `k_task_step` of csrc/taskstep.h), `_LAYOUT` (the observation row, for the shape error) and
    `_EPISODE_LENGTH` (the default);
  * `_reset_values(ep)`: the three state tensors at the start of episode `ep` (N,);
  * `_advance(a)`: the clamped action (N, A) -> (the three new state tensors, reward (N,), terminal mask (N,) or None);
  * `_obs_blocks()` where an observation block is not the state tensor itself;
  * `info_keys`: the names of its per-env float32 info channels, in the order of the task struct's `inf[]`; with
    `info_channels=True`, `_advance` also leaves their values in `self._info_step` (a tuple of (N,) tensors).

Info channels (`info_channels=True`; `create_task_env` asks for them exactly when `cfg.info_track_keys` is set): the values belong to
the step just taken -- for an env that finishes, they are taken before its reset -- and `step` adds `{key: (N,) row}` to the info
dict, beside `"TimeLimit.truncated"`.  The HIP step writes them from the same launch (the `_info` entry: a channel-major
(n_info, N) block).  They are derived from the state, so `state_dict` does not hold them.
`_step_torch` is the definition and the CPU / `PQL_SYNTH_TORCH` form; every written operation is one fp32 rounding, which is what
lets the HIP step be bit-equal to it.
"""
from __future__ import annotations

import os
from types import SimpleNamespace

import numpy as np
import torch

_M = 0xFFFFFFFF


def _hash32(x):
    """xorshift-multiply avalanche on int64 tensors holding 32-bit values."""
    x = x & _M
    x = ((x ^ (x >> 16)) * 0x7FEB352D) & _M
    x = ((x ^ (x >> 15)) * 0x846CA68B) & _M
    return x ^ (x >> 16)


class VecEnvBase:
    """The env contract's attributes and the header every saved env state carries."""

    def __init__(self, num_envs, obs_dim, act_dim, device, seed, episode_length, env_offset):
        self.num_envs, self.obs_dim, self.act_dim = int(num_envs), int(obs_dim), int(act_dim)
        self.device = torch.device(device)
        self.seed = int(seed)
        self.max_episode_length = int(episode_length)
        self.observation_space = SimpleNamespace(shape=(self.obs_dim,))
        self.action_space = SimpleNamespace(shape=(self.act_dim,))
        self.env_offset = int(env_offset)
        self.env_ids = torch.arange(self.num_envs, device=self.device, dtype=torch.int64) + self.env_offset

    def _header(self):
        return {"seed": self.seed, "num_envs": self.num_envs, "env_offset": self.env_offset}

    def _check_header(self, state):
        for key in ("seed", "num_envs", "env_offset"):
            if int(state[key]) != getattr(self, key):
                raise ValueError(f"{type(self).__name__}.load_state_dict: {key}={getattr(self, key)} but the state was saved with {int(state[key])}")


class HashResetVecEnv(VecEnvBase):
    _STATE = ()
    _ENTRY = None
    _LAYOUT = ""
    _EPISODE_LENGTH = 64
    info_keys = ()

    def __init__(self, num_envs, obs_dim, act_dim, device="cuda", seed=42, episode_length=None, env_offset=0, info_channels=False):
        if int(act_dim) <= 0 or int(obs_dim) < 3 * int(act_dim):   # (before anything touches the device)
            raise ValueError(f"{type(self).__name__}: obs = {self._LAYOUT} needs obs_dim >= 3 * act_dim, got obs_dim={int(obs_dim)}, "
                             f"act_dim={int(act_dim)}")
        super().__init__(num_envs, obs_dim, act_dim, device, seed, self._EPISODE_LENGTH if episode_length is None else episode_length,
                         env_offset)
        self.info_channels = bool(info_channels) and len(self.info_keys) > 0
        self._info_step = None
        self.inv_a = float(np.float32(1.0) / np.float32(self.act_dim))   # the fp32 constant 1.0f / A, in both forms
        n, A, dev = self.num_envs, self.act_dim, self.device
        for name in self._STATE:
            setattr(self, name, torch.zeros((n, A), dtype=torch.float32, device=dev))
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

    def _start(self, ep):
        for name, start in zip(self._STATE, self._reset_values(ep)):
            getattr(self, name).copy_(start)
        self.k.zero_()

    def _obs_blocks(self):
        return tuple(getattr(self, name) for name in self._STATE)

    def _observe(self):
        obs = torch.zeros((self.num_envs, self.obs_dim), dtype=torch.float32, device=self.device)
        A = self.act_dim
        obs[:, :A], obs[:, A:2 * A], obs[:, 2 * A:3 * A] = self._obs_blocks()
        return obs

    @torch.no_grad()
    def reset(self):
        """Every env back to the start of its episode 0."""
        self.ep.zero_()
        self._start(self.ep)
        return self._observe()

    # ---- state -------------------------------------------------------------------------------------
    def state_dict(self):
        """Everything the next transitions depend on besides the constructor arguments."""
        out = {name: getattr(self, name).detach().clone() for name in (*self._STATE, "k", "ep")}
        out.update(self._header())
        return out

    def load_state_dict(self, state):
        self._check_header(state)
        for name in (*self._STATE, "k", "ep"):
            mine = getattr(self, name)
            if tuple(state[name].shape) != tuple(mine.shape):
                raise ValueError(f"{type(self).__name__}.load_state_dict: {name} has shape {tuple(mine.shape)} but the state holds {tuple(state[name].shape)}")
            mine.copy_(state[name].to(self.device, mine.dtype))

    # ---- step --------------------------------------------------------------------------------------
    @torch.no_grad()
    def step(self, action):
        if self.device.type == "cuda" and not os.environ.get("PQL_SYNTH_TORCH"):   # one HIP launch instead of tens of torch launches
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
        new, reward, terminal = self._advance(action.to(torch.float32).clamp(-1.0, 1.0))
        k = self.k + 1
        truncated = k >= self.max_episode_length
        if terminal is None:
            done = truncated.clone()
        else:
            truncated = truncated & ~terminal
            done = terminal | truncated
        # auto-reset of the finished envs: next episode's start, drawn from the hash
        ep = self.ep + done.to(torch.int32)
        d = done.unsqueeze(1)
        for name, start, now in zip(self._STATE, self._reset_values(ep), new):
            setattr(self, name, torch.where(d, start, now))
        self.k = torch.where(done, torch.zeros_like(k), k)
        self.ep = ep
        info = {"TimeLimit.truncated": truncated}
        if self.info_channels:
            info.update(zip(self.info_keys, self._info_step))
        return self._observe(), reward, done, info

    def _step_hip(self, action):
        """Same transition as `_step_torch`, one launch (`_ENTRY`, include/pqlk.h): state updated in place."""
        from pql_amd import _lib as L
        n, dev = self.num_envs, self.device
        next_obs = torch.empty((n, self.obs_dim), dtype=torch.float32, device=dev)
        reward = torch.empty(n, dtype=torch.float32, device=dev)
        done = torch.empty(n, dtype=torch.bool, device=dev)
        truncated = torch.empty(n, dtype=torch.bool, device=dev)
        act = action.to(dev, torch.float32).contiguous()
        if tuple(act.shape) != (n, self.act_dim):
            raise ValueError(f"{type(self).__name__}.step: action has shape {tuple(act.shape)}, expected {(n, self.act_dim)}")
        entry, extra, info = self._ENTRY, (), {"TimeLimit.truncated": truncated}
        if self.info_channels:   # the same launch, plus one coalesced row per channel
            block = torch.empty((len(self.info_keys), n), dtype=torch.float32, device=dev)
            entry, extra = self._ENTRY + "_info", (L.ptr(block),)
            info.update(zip(self.info_keys, block.unbind(0)))
        with torch.cuda.device(dev):
            L.check(getattr(L.lib, entry)(n, self.obs_dim, self.act_dim, self.seed & 0xFFFFFFFF, self.env_offset & 0xFFFFFFFF,
                                          self.max_episode_length, L.ptr(act), *(L.ptr(getattr(self, name)) for name in self._STATE),
                                          L.ptr(self.k), L.ptr(self.ep), L.ptr(next_obs), L.ptr(reward), L.ptr(done),
                                          L.ptr(truncated), *extra, L.stream(dev)))
        return next_obs, reward, done, info
