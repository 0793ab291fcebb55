"""Reacher task, torch definition (pql_amd/envs/reacher.py `_step_torch`) on the CPU: the whole transition against an independent
recomputation in numpy float32 scalars (one rounding per written operation, the resets from `task_cases.u_np`), the info channels,
the tip columns across a reset, sharding of the env axis, the state round trip, the config surface, the entry point's argument checks
and the yardstick controllers.  No kernel is launched here; tests/test_reacher_gpu.py holds the HIP step to this definition bit for
bit."""
import os
import re

import numpy as np
import pytest
import torch

import task_cases as tc
from pql_amd.envs.pointmass import PointMassVecEnv
from pql_amd.envs.pointmass import episode_return as pointmass_episode_return
from pql_amd.envs.reacher import ReacherVecEnv, episode_return, jacobian_policy, zero_policy
from pql_amd.envs.swingup import SwingUpVecEnv
from pql_amd.envs.synthetic import TASK_ENVS, TASK_SHAPES, SyntheticVecEnv, create_task_env
from pql_amd.utils.cfg import load_cfg
from task_cases import F, rot_np, tip_np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STREAM_TH, STREAM_W = 15, 16


# --------------------------------------------------------------------------- the definition, once more, in numpy scalars (rot_np, tip_np: tests/task_cases.py)
class ReacherNp:
    """The issue's definition on numpy float32 scalars, env by env and joint by joint (independent of the env's code)."""

    def __init__(self, n, O, A, seed, episode_length, env_offset=0):
        self.n, self.O, self.A, self.seed, self.L, self.off = n, O, A, seed, episode_length, env_offset
        self.c, self.s, self.w = (np.zeros((n, A), dtype=F) for _ in range(3))
        self.k, self.ep = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32)
        for i in range(n):
            self._reset(i, 0)

    def _reset(self, i, ep):
        e = (self.off + i) & 0xFFFFFFFF
        for j in range(self.A):
            d = F(0.5) * (F(2.0) * tc.u_np(self.seed, e, ep, STREAM_TH, j) - F(1.0))
            c, s = F(1.0), F(0.0)
            for _ in range(6):
                c, s = rot_np(c, s, d)
            self.c[i, j], self.s[i, j] = c, s
            self.w[i, j] = F(0.5) * (F(2.0) * tc.u_np(self.seed, e, ep, STREAM_W, j) - F(1.0))
        self.k[i] = 0

    def obs(self):
        A, out = self.A, np.zeros((self.n, self.O), dtype=F)
        out[:, :A], out[:, A:2 * A], out[:, 2 * A:3 * A] = self.c, self.s, F(0.25) * self.w
        for i in range(self.n):
            out[i, 3 * A], out[i, 3 * A + 1] = tip_np(self.c[i], self.s[i])
        return out

    def step(self, action):
        """-> obs, reward, done, truncated, (tip_dist2, effort, reached)"""
        A, inv_a = self.A, F(1.0) / F(self.A)
        reward, done = np.zeros(self.n, dtype=F), np.zeros(self.n, dtype=bool)
        chans = np.zeros((3, self.n), dtype=F)
        for i in range(self.n):
            w2 = eff = None
            for j in range(A):
                a = min(max(F(action[i, j]), F(-1.0)), F(1.0))
                w = min(max(F(0.9) * self.w[i, j] + F(0.3) * a, F(-3.0)), F(3.0))
                self.c[i, j], self.s[i, j] = rot_np(self.c[i, j], self.s[i, j], F(0.05) * w)
                self.w[i, j] = w
                w2 = w * w if j == 0 else w2 + w * w
                eff = a * a if j == 0 else eff + a * a
            ex, ey = tip_np(self.c[i], self.s[i])
            d2 = ex * ex + ey * ey
            cost = (d2 + F(0.01) * (w2 * inv_a)) + F(0.01) * (eff * inv_a)
            reward[i] = -(F(0.05) * cost)
            assert type(cost) is F and type(d2) is F
            chans[:, i] = d2, eff * inv_a, F(1.0) if d2 < F(0.01) else F(0.0)
            self.k[i] += 1
            if self.k[i] >= self.L:
                done[i] = True
                self.ep[i] += 1
                self._reset(i, int(self.ep[i]))
        return self.obs(), reward, done, done.copy(), chans


T = torch.from_numpy


def _assert_state(env, ref, where):
    for name in ("c", "s", "w", "k", "ep"):
        assert torch.equal(getattr(env, name), T(getattr(ref, name))), (where, name)


# --------------------------------------------------------------------------- the transition
@pytest.mark.parametrize("O,A", [(8, 2), (5, 1), (12, 3), (50, 16)])
def test_step_torch_equals_the_numpy_recomputation(O, A):
    """12 steps of `task_actions` at episode_length 5 (two resets per env), 9 envs at env_offset 3: observations (tip columns
    included), rewards, dones, truncations, the five state tensors and, on a twin env with info_channels, the three channels are
    bit-equal to `ReacherNp`; the plain env's info dict holds only the time-limit key and its other outputs equal the twin's."""
    n = 9
    mk = lambda **kw: ReacherVecEnv(n, O, A, device="cpu", seed=77, episode_length=5, env_offset=3, **kw)   # noqa: E731
    env, chan, ref = mk(), mk(info_channels=True), ReacherNp(n, O, A, 77, 5, env_offset=3)
    assert chan.info_channels and not env.info_channels
    assert torch.equal(env.reset(), T(ref.obs())) and torch.equal(chan.reset(), T(ref.obs()))
    _assert_state(env, ref, "reset")
    seen = dict(reached=0, missed=0, clamped=0)
    for t, act in enumerate(tc.task_actions(n, A, 12)):
        obs, rew, done, info = env.step(act)
        obs_c, rew_c, done_c, info_c = chan.step(act)
        want = ref.step(act.numpy())
        assert obs.dtype == torch.float32 and rew.dtype == torch.float32 and done.dtype == torch.bool
        assert torch.equal(obs, T(want[0])), (t, "obs")
        assert torch.equal(rew, T(want[1])), (t, "reward")
        assert torch.equal(done, T(want[2])) and torch.equal(info["TimeLimit.truncated"], T(want[3])), t
        _assert_state(env, ref, t)
        assert set(info) == {"TimeLimit.truncated"} and set(info_c) == {"TimeLimit.truncated", "tip_dist2", "effort", "reached"}
        assert torch.equal(obs_c, obs) and torch.equal(rew_c, rew) and torch.equal(done_c, done)
        assert torch.equal(info_c["TimeLimit.truncated"], info["TimeLimit.truncated"])
        _assert_state(chan, ref, t)
        for row, key in enumerate(ReacherVecEnv.info_keys):
            assert info_c[key].dtype == torch.float32 and torch.equal(info_c[key], T(want[4][row])), (t, key)
        assert torch.equal(obs[:, 3 * A + 2:], torch.zeros(n, O - 3 * A - 2))
        assert bool(done.all()) == (t % 5 == 4)
        seen["reached"] += int(want[4][2].sum()); seen["missed"] += int((want[4][2] == 0).sum())
        seen["clamped"] += int((act.abs() > 1).sum())
    assert int(env.ep.min()) == 2 and seen["missed"] > 0 and seen["clamped"] > 0
    assert "info" not in " ".join(env.state_dict()) and set(env.state_dict()) == set(chan.state_dict())


def test_reached_channel_and_speed_clamp():
    """Both values of `reached`, and the clamp of w from both sides, on states set by hand.  Env 0 is a two-link arm folded so that
    its tip is on the goal: link 0 at acos(0.6), joint 1 turned back by twice that (cos = 2 * 0.36 - 1 = -0.28, sin = -2 * 0.6 * 0.8).
    Env 1 is stretched away from the goal and spins faster than the dynamics ever get on their own (0.9 w + 0.3 a stays below 3 from
    below 3, so only a state put there meets the clamp); env 2 starts at +-2.9 and stays inside."""
    env = ReacherVecEnv(3, 8, 2, device="cpu", info_channels=True)
    env.c.copy_(torch.tensor([[0.6, -0.28], [-1.0, 1.0], [-1.0, 1.0]]))
    env.s.copy_(torch.tensor([[0.8, -0.96], [0.0, 0.0], [0.0, 0.0]]))
    env.w.copy_(torch.tensor([[0.0, 0.0], [3.5, -3.5], [2.9, -2.9]]))
    obs, rew, done, info = env.step(torch.tensor([[0.0, 0.0], [1.0, -1.0], [1.0, -1.0]]))
    assert info["reached"].tolist() == [1.0, 0.0, 0.0]
    assert float(info["tip_dist2"][0]) < 1e-10 and float(info["tip_dist2"][1]) > 2.0 and abs(float(rew[0])) < 1e-10
    assert info["effort"].tolist() == [0.0, 1.0, 1.0]
    assert torch.equal(env.w[1], torch.tensor([3.0, -3.0]))
    np.testing.assert_allclose(env.w[2].numpy(), [2.91, -2.91], rtol=0, atol=1e-6)
    assert torch.equal(obs[:, 4:6], 0.25 * env.w) and not done.any()


def test_tip_columns_follow_the_reset():
    """The tip columns of `reset()` and of a done transition's next_obs are the tip of the NEW episode's state."""
    n, O, A = 6, 11, 3
    env = ReacherVecEnv(n, O, A, device="cpu", seed=5, episode_length=3, env_offset=2)
    ref = ReacherNp(n, O, A, 5, 3, env_offset=2)
    obs = env.reset()
    for i in range(n):
        ex, ey = tip_np(ref.c[i], ref.s[i])
        assert float(obs[i, 3 * A]) == ex and float(obs[i, 3 * A + 1]) == ey
    acts = tc.task_actions(n, A, 3)
    for act in acts:
        before = (env.c.clone(), env.s.clone())
        obs, _, done, _ = env.step(act)
    assert done.all()
    fresh = ReacherNp(n, O, A, 5, 3, env_offset=2)
    for i in range(n):
        fresh._reset(i, 1)
        ex, ey = tip_np(fresh.c[i], fresh.s[i])
        assert float(obs[i, 3 * A]) == ex and float(obs[i, 3 * A + 1]) == ey
        assert torch.equal(env.c[i], T(fresh.c[i])) and not torch.equal(env.c[i], before[0][i])
    assert torch.equal(obs, env._observe())


def test_shards_reproduce_slices_of_the_global_env():
    full = ReacherVecEnv(64, 8, 2, device="cpu", seed=42, episode_length=5)
    part = ReacherVecEnv(5, 8, 2, device="cpu", seed=42, episode_length=5, env_offset=40)
    assert torch.equal(part.reset(), full.reset()[40:45])
    for act in tc.task_actions(64, 2, 12):
        fo, fr, fd, fi = full.step(act)
        po, pr, pd, pi = part.step(act[40:45])
        assert torch.equal(po, fo[40:45]) and torch.equal(pr, fr[40:45]) and torch.equal(pd, fd[40:45])
        assert torch.equal(pi["TimeLimit.truncated"], fi["TimeLimit.truncated"][40:45])
    for name in ("c", "s", "w", "k", "ep"):
        assert torch.equal(getattr(part, name), getattr(full, name)[40:45]), name
    assert int(full.ep.min()) == 2


def test_state_round_trip():
    mk = lambda **kw: ReacherVecEnv(16, 8, 2, device="cpu", **{**dict(seed=5, episode_length=6, env_offset=3), **kw})   # noqa: E731
    acts = tc.task_actions(16, 2, 20, seed=1)
    env = mk()
    env.reset()
    for a in acts[:9]:
        env.step(a)
    state = env.state_dict()
    assert set(state) == {"c", "s", "w", "k", "ep", "seed", "num_envs", "env_offset"}
    kept = {k: v.clone() for k, v in state.items() if torch.is_tensor(v)}
    fresh = mk()
    fresh.load_state_dict(state)
    for a in acts[9:]:
        want, got = env.step(a), fresh.step(a)
        for w, h in zip(want[:3], got[:3]):
            assert torch.equal(w, h)
        assert torch.equal(want[3]["TimeLimit.truncated"], got[3]["TimeLimit.truncated"])
    for name in ("c", "s", "w", "k", "ep"):
        assert torch.equal(getattr(env, name), getattr(fresh, name))
        assert torch.equal(state[name], kept[name]), "state_dict must hand out copies, not the live tensors"
    assert int(env.ep.max()) >= 2
    for kw in (dict(seed=6), dict(env_offset=4)):
        with pytest.raises(ValueError, match="ReacherVecEnv.load_state_dict"):
            mk(**kw).load_state_dict(state)
    with pytest.raises(ValueError, match="num_envs"):
        ReacherVecEnv(17, 8, 2, device="cpu", seed=5, episode_length=6, env_offset=3).load_state_dict(state)
    with pytest.raises(ValueError, match="shape"):
        mk().load_state_dict(dict(state, w=torch.zeros(16, 3)))


# --------------------------------------------------------------------------- the config surface
def test_config_surface():
    cfg = load_cfg(["task=reacher", "num_envs=8", "device=cpu"])
    assert dict(cfg.task) == dict(name="Reacher", kind="reacher", obs_dim=8, act_dim=2, episode_length=64)
    env = create_task_env(cfg)
    assert isinstance(env, ReacherVecEnv) and env.observation_space.shape == (8,) and env.action_space.shape == (2,)
    assert env.max_episode_length == 64 and env.num_envs == 8 and env.env_offset == 0 and env.seed == cfg.seed
    assert not env.info_channels and TASK_ENVS["reacher"] is ReacherVecEnv and list(TASK_ENVS)[-1] == "reacher"
    assert create_task_env(load_cfg(["task=reacher", "num_envs=4", "sim_device=cpu", "info_track_keys=[reached]", "info_track_step=[last]"])).info_channels
    big = create_task_env(load_cfg(["task=reacher", "task.obs_dim=88", "task.act_dim=16", "num_envs=8", "device=cpu"]), num_envs=5, env_offset=40)
    assert isinstance(big, ReacherVecEnv) and (big.obs_dim, big.act_dim, big.num_envs, big.env_offset) == (88, 16, 5, 40)
    for O, A in TASK_SHAPES.values():                               # every benchmarked shape fits
        assert ReacherVecEnv(2, O, A, device="cpu").reset().shape == (2, O)
    with pytest.raises(ValueError, match=r"ReacherVecEnv: obs = \[c \| s \| w / 4 \| ex \| ey \| 0 \.\.\.\] needs obs_dim >= 3 \* act_dim \+ 2, got obs_dim=7, act_dim=2"):
        create_task_env(load_cfg(["task=reacher", "task.obs_dim=7", "device=cpu"]))
    with pytest.raises(ValueError, match="obs_dim=7"):
        ReacherVecEnv(4, 7, 2, device="cuda:5")                     # raised before anything touches the device
    with pytest.raises(ValueError, match="obs_dim=47"):
        ReacherVecEnv(4, 47, 16, device="cpu")
    with pytest.raises(ValueError):
        ReacherVecEnv(4, 8, 0, device="cpu")
    ReacherVecEnv(4, 50, 16, device="cpu")                          # 3 A + 2 exactly
    with pytest.raises(ValueError, match="known kinds: .*swingup, reacher"):
        create_task_env(load_cfg(["task=reacher", "task.kind=pendulum", "device=cpu"]))
    with pytest.raises(ValueError, match="task=reacher"):
        load_cfg(["task=Reach", "device=cpu"])
    # what existed before builds what it built before
    assert type(create_task_env(load_cfg(["task=pointmass", "num_envs=8", "device=cpu"]))) is PointMassVecEnv
    assert type(create_task_env(load_cfg(["task=swingup", "num_envs=8", "device=cpu"]))) is SwingUpVecEnv
    for ov in (["task=AllegroHand"], ["task=ShadowHand"], ["task.name=Toy"], ["task=synthetic"], []):
        assert type(create_task_env(load_cfg([*ov, "num_envs=8", "device=cpu"]))) is SyntheticVecEnv
    from pql_amd.utils.common import preprocess_cfg
    cfg = load_cfg(["task=reacher", "algo=ddpg_algo", "device=cpu"])
    preprocess_cfg(cfg)
    assert cfg.algo.reward_scale == 1


def test_learning_tool_knows_the_task():
    lp = tc.load_script("tools/learn_pointmass.py", "learn_pointmass_re_cpu")
    tk = lp.TASKS["reacher"]
    assert tk["env"] is ReacherVecEnv and tk["episode_length"] == 64 and tk["ctrl_key"] == "R_ctrl"
    assert tk["zero"] is zero_policy and tk["ctrl"] is jacobian_policy
    assert lp.TASKS["pointmass"]["ctrl_key"] == "R_pd" and lp.TASKS["swingup"]["ctrl_key"] == "R_ctrl"
    ov = lp.overrides("ddpg", "small", 0, 10, "/nowhere", task="reacher")
    assert "task=reacher" in ov and "task.episode_length=64" in ov


# --------------------------------------------------------------------------- the entry point
def test_reacher_step_argument_checks():
    """PQLK_E_NULL / PQLK_E_SHAPE come back before anything is launched (0x1000 stands in for device memory)."""
    import ctypes as C
    from pql_amd import _lib as L
    P = C.c_void_p(0x1000)
    names = ("action", "c", "s", "w", "k", "ep", "next_obs", "reward", "done", "truncated")

    def step(n, O, A, null=None, entry="pqlk_reacher_step", info=()):
        ptrs = [None if name == null else P for name in names]
        return getattr(L.lib, entry)(n, O, A, 1, 0, 5, *ptrs, *info, None)

    for name in names:
        assert step(16, 8, 2, null=name) == 1, name                 # PQLK_E_NULL
        assert step(16, 8, 2, null=name, entry="pqlk_reacher_step_info", info=(P,)) == 1, name
    assert step(16, 8, 2, entry="pqlk_reacher_step_info", info=(None,)) == 1
    assert step(0, 8, 2) == 2 and step(-3, 8, 2) == 2 and step(16, 8, 0) == 2   # PQLK_E_SHAPE
    assert step(16, 7, 2) == 2 and step(16, 49, 16) == 2            # O = 3 A + 1: no room for the tip columns
    assert step(16, 7, 2, entry="pqlk_reacher_step_info", info=(P,)) == 2
    assert step(16, 2 ** 23, 2) == 2                                # a block's rows must index with 32-bit ints


def test_symbols_are_declared_exported_and_bound():
    import ctypes as C
    from pql_amd import _lib as L
    hdr = open(os.path.join(ROOT, "include", "pqlk.h")).read()
    want = ["n", "obs_dim", "act_dim", "seed", "env_offset", "episode_length", "action", "c", "s", "w", "k", "ep", "next_obs", "reward", "done",
            "truncated", "stream"]
    for entry, names in (("pqlk_reacher_step", want), ("pqlk_reacher_step_info", want[:-1] + ["info", "stream"])):
        decl = re.search(r"int %s\(([^;]*)\);" % entry, hdr)
        assert decl, f"include/pqlk.h does not declare {entry}"
        params = [p.strip() for p in decl.group(1).replace("\n", " ").split(",")]
        assert [p.split()[-1].lstrip("*") for p in params] == names
        res, args = L.PROTOTYPES[entry]
        assert res is C.c_int and len(args) == len(params)
        assert args[:6] == [C.c_int64, C.c_int32, C.c_int32, C.c_uint32, C.c_uint32, C.c_int32] and all(a is C.c_void_p for a in args[6:])
        fn = getattr(C.CDLL(os.fspath(L.LIB_FILE)), entry)          # AttributeError if the library does not export it
        assert fn is not None and getattr(L.lib, entry).argtypes == args
    assert re.search(r"reacher:\s+0 = tip_dist2.*\n.*2 = reached", hdr)
    mk = open(os.path.join(ROOT, "pql_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS\s*=.*\breacher\.hip\b", mk, re.M) and re.search(r"^SRCS\s*=.*\bswingup\.hip\b", mk, re.M)
    # the rotation is written once, in the header both task files include
    csrc = os.path.join(ROOT, "pql_amd", "csrc")
    for name in ("swingup.hip", "reacher.hip"):
        src = open(os.path.join(csrc, name)).read()
        assert '#include "rot.h"' in src and "0.041666668f" not in src and "#pragma clang fp contract(off)" in src, name
    assert "0.041666668f" in open(os.path.join(csrc, "rot.h")).read()


# --------------------------------------------------------------------------- the yardsticks
@pytest.mark.parametrize("O,A", [(8, 2), (88, 16)])
def test_controllers_bracket_the_task(O, A):
    """256 envs, seed 10000, episode_length 64.  The definition alone gives R_zero = -2.881 / -1.343 and R_ctrl = -0.534 / -0.215 at the
    two shapes: the controller closes 0.81 / 0.84 of |R_zero| where the bar is 0.5; a uniform random policy stays near the zero action;
    at (8, 2) 0.94 of the arms are within 0.1 of the goal on step 63 where the bar is 0.75."""
    assert episode_return is pointmass_episode_return               # the measure is PointMass's, not a copy
    env = ReacherVecEnv(256, O, A, device="cpu", seed=10_000, episode_length=64, info_channels=True)
    r_zero, r_ctrl = episode_return(env, zero_policy(env)), episode_return(env, jacobian_policy(env))
    g = torch.Generator().manual_seed(0)
    r_rand = episode_return(env, lambda obs: 2.0 * torch.rand((256, A), generator=g) - 1.0)
    obs, pol = env.reset(), jacobian_policy(env)
    worst = 0.0
    for _ in range(63):
        act = pol(obs)
        obs, _, done, info = env.step(act)
        worst = max(worst, float(((env.c * env.c + env.s * env.s) - 1.0).abs().max()))
        assert act.shape == (256, A) and float(act.abs().max()) <= 1.0 and not done.any()
    share = float(info["reached"].mean())
    print(f"reacher yardsticks ({O}, {A}): R_zero = {r_zero:.3f}, R_ctrl = {r_ctrl:.3f}, R_random = {r_rand:.3f}, reached = {share:.3f}, "
          f"worst |c^2 + s^2 - 1| = {worst:.2e}")
    assert r_ctrl - r_zero > 0.5 * abs(r_zero), (r_zero, r_ctrl)
    assert r_rand < r_ctrl
    assert worst <= 1e-6 and float(env.w.abs().max()) <= 3.0
    if (O, A) == (8, 2):
        assert share >= 0.75
    assert torch.equal(zero_policy(env)(obs), torch.zeros(256, A))
