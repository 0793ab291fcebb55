"""SwingUp task, torch definition (pql_amd/envs/swingup.py `_step_torch`) on the CPU: a known-answer step worked out in numpy float32
scalars, hash resets, sharding of the env axis, the invariants of the rotation (unit circle, speed clamp), the counters, the state
round trip, the yardstick controllers and the config surface.  No kernel is launched here; tests/test_swingup_gpu.py holds the HIP step
to this definition bit for bit."""
import os
import re

import numpy as np
import pytest
import torch

from pql_amd.envs.pointmass import PointMassVecEnv
from pql_amd.envs.pointmass import episode_return as pointmass_episode_return
from pql_amd.envs.swingup import SwingUpVecEnv, energy_policy, episode_return, zero_policy
from pql_amd.envs.synthetic import TASK_SHAPES, SyntheticVecEnv, create_task_env
from pql_amd.utils.cfg import load_cfg
from task_cases import u_np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
C4, S3, S5 = F(0.041666668), F(0.16666667), F(0.008333334)


def _env(n=4, O=8, A=2, **kw):
    return SwingUpVecEnv(n, O, A, device="cpu", **kw)


def rot_np(c, s, d):
    """The issue's rot in numpy float32 scalars, one rounding per written operation (independent of the env's code)."""
    d2 = d * d
    cd = F(1.0) - d2 * (F(0.5) - d2 * C4)
    sd = d * (F(1.0) - d2 * (S3 - d2 * S5))
    cn = c * cd - s * sd
    sn = s * cd + c * sd
    m = F(1.5) - F(0.5) * (cn * cn + sn * sn)
    return cn * m, sn * m


def _reset_obs(env, ep):
    """Start-of-episode observation recomputed from the hash: d = 0.5 (2 u_13 - 1), (c, s) = rot^4 (-1, 0), w = 2 u_14 - 1."""
    A = env.act_dim
    obs = np.zeros((env.num_envs, env.obs_dim), dtype=np.float32)
    for i in range(env.num_envs):
        e = env.env_offset + i
        for j in range(A):
            d = F(0.5) * (F(2.0) * u_np(env.seed, e, ep, 13, j) - F(1.0))
            c, s = F(-1.0), F(0.0)
            for _ in range(4):
                c, s = rot_np(c, s, d)
            obs[i, j], obs[i, A + j] = c, s
            obs[i, 2 * A + j] = F(0.125) * (F(2.0) * u_np(env.seed, e, ep, 14, j) - F(1.0))
    return torch.from_numpy(obs)


def test_known_answer_step():
    """Two envs, A = 2, O = 8.  Env 0: joints at (c, s, w) = (-1, 0, 0.5) and (0.6, 0.8, -7.9), a = (3, -0.25): a clamps to 1 in column
    0, and w' = -7.9 + 0.05 (12 - 1.5) = -7.375 stays inside.  Env 1: (0, 1, 7.9) and (0.8, -0.6, 0), a = (0.5, -2): w' = 7.9 + 0.05 (15
    + 3) = 8.8 clamps to 8, the other to -1 with w' = 0.05 (-9 - 6) = -0.75."""
    env = _env(n=2, episode_length=128)
    c0 = [[F(-1.0), F(0.6)], [F(0.0), F(0.8)]]
    s0 = [[F(0.0), F(0.8)], [F(1.0), F(-0.6)]]
    w0 = [[F(0.5), F(-7.9)], [F(7.9), F(0.0)]]
    act = [[F(3.0), F(-0.25)], [F(0.5), F(-2.0)]]
    env.c.copy_(torch.tensor(c0)); env.s.copy_(torch.tensor(s0)); env.w.copy_(torch.tensor(w0))
    obs, reward, done, info = env.step(torch.tensor(act))
    want_obs = np.zeros((2, 8), dtype=np.float32)
    want_r, want_w = [], np.zeros((2, 2), dtype=np.float32)
    for i in range(2):
        costs = []
        for j in range(2):
            a = min(max(act[i][j], F(-1.0)), F(1.0))
            w = w0[i][j] + F(0.05) * (F(15.0) * s0[i][j] + F(6.0) * a)
            w = min(max(w, F(-8.0)), F(8.0))
            c, s = rot_np(c0[i][j], s0[i][j], F(0.05) * w)
            costs.append(((F(1.0) - c) + F(0.01) * (w * w)) + F(0.01) * (a * a))
            want_obs[i, j], want_obs[i, 2 + j], want_obs[i, 4 + j], want_w[i, j] = c, s, F(0.125) * w, w
            assert type(w) is F and type(c) is F and type(costs[-1]) is F
        want_r.append(-(F(0.05) * ((costs[0] + costs[1]) * (F(1.0) / F(2.0)))))
    assert torch.equal(obs, torch.from_numpy(want_obs)), (obs, want_obs)
    assert torch.equal(reward, torch.tensor(want_r)), (reward, want_r)
    assert torch.equal(env.c, obs[:, 0:2]) and torch.equal(env.s, obs[:, 2:4]) and torch.equal(env.w, torch.from_numpy(want_w))
    # ... and against values worked out by hand: the speeds, and the angle advanced by 0.05 w' (double-precision trigonometry)
    np.testing.assert_allclose(env.w.numpy(), [[0.5 + 0.05 * 6.0, -7.375], [8.0, -0.75]], rtol=0, atol=1e-6)
    th0 = np.arctan2(np.array(s0, dtype=np.float64), np.array(c0, dtype=np.float64))
    th1 = th0 + 0.05 * env.w.numpy().astype(np.float64)
    np.testing.assert_allclose(obs[:, 0:2].numpy(), np.cos(th1), rtol=0, atol=2e-5)   # the degree-4 / 5 polynomials at |d| = 0.4:
    np.testing.assert_allclose(obs[:, 2:4].numpy(), np.sin(th1), rtol=0, atol=2e-5)   # remainders d^6 / 720 = 5.7e-6, d^7 / 5040 = 3.3e-7
    assert not done.any() and not info["TimeLimit.truncated"].any() and info["TimeLimit.truncated"].dtype == torch.bool
    assert torch.equal(env.k, torch.ones(2, dtype=torch.int32)) and torch.equal(env.ep, torch.zeros(2, dtype=torch.int32))
    assert obs.dtype == torch.float32 and reward.dtype == torch.float32 and done.dtype == torch.bool
    assert env.c.dtype == env.s.dtype == env.w.dtype == torch.float32 and env.k.dtype == env.ep.dtype == torch.int32


def test_reset_is_the_hash_of_seed_env_and_episode():
    env = _env(n=5, O=11, A=3, seed=7, env_offset=9)
    first = env._observe()                                          # construction starts episode 0 too
    obs = env.reset()
    assert torch.equal(obs, first) and torch.equal(obs, _reset_obs(env, 0))
    c, s, w = obs[:, :3], obs[:, 3:6], 8.0 * obs[:, 6:9]
    assert ((c * c + s * s) - 1.0).abs().max() <= 1e-6 and w.abs().max() <= 1.0
    assert c.max() < 0.417                                          # within 2 rad of hanging: cos(pi - 2) = 0.4161 at the most
    assert torch.equal(obs[:, 9:], torch.zeros(5, 2))               # zero tail
    assert c.unique().numel() == 15 and w.unique().numel() == 15    # every env and column its own draw
    # an episode's start depends on (seed, global env id, episode) alone: not on the env count, the offset split or the path there
    other = SwingUpVecEnv(3, 11, 3, device="cpu", seed=7, env_offset=11, episode_length=2)
    assert torch.equal(other.reset(), obs[2:5])
    g = torch.Generator().manual_seed(0)
    for _ in range(4):                                              # two episodes of whatever actions: episode 2 starts the same
        nobs, _, done, _ = other.step(2.0 * torch.rand((3, 3), generator=g) - 1.0)
    assert done.all() and torch.equal(other.ep, torch.full((3,), 2, dtype=torch.int32))
    assert torch.equal(nobs, _reset_obs(other, 2)) and not torch.equal(nobs, _reset_obs(other, 1))
    assert not torch.equal(SwingUpVecEnv(5, 11, 3, device="cpu", seed=8, env_offset=9).reset(), obs)


def test_counters_and_truncation():
    """done == truncated on every step; k counts the steps of the episode, ep the episodes; the next_obs of a done transition is the
    new episode's first observation."""
    env = _env(n=6, seed=3, episode_length=3)
    env.reset()
    g = torch.Generator().manual_seed(2)
    for t in range(1, 10):
        obs, reward, done, info = env.step(3.0 * (2.0 * torch.rand((6, 2), generator=g) - 1.0))
        assert torch.equal(done, info["TimeLimit.truncated"]) and done.dtype == torch.bool
        assert bool(done.all()) == (t % 3 == 0) and bool(done.any()) == (t % 3 == 0)
        assert torch.equal(env.k, torch.full((6,), t % 3, dtype=torch.int32))
        assert torch.equal(env.ep, torch.full((6,), t // 3, dtype=torch.int32))
        if t % 3 == 0:
            assert torch.equal(obs, _reset_obs(env, t // 3))
        assert (reward <= 0).all()


def test_shards_reproduce_slices_of_the_global_env():
    mk = lambda n, off: SwingUpVecEnv(n, 7, 2, device="cpu", seed=42, episode_length=4, env_offset=off)   # noqa: E731
    full, shards = mk(64, 0), [mk(32, 0), mk(32, 32)]
    assert torch.equal(full.reset(), torch.cat([s.reset() for s in shards]))
    late = mk(40, 24)                                               # env_offset = k equals rows k: of the global env
    assert torch.equal(late.reset(), full._observe()[24:])
    g = torch.Generator().manual_seed(0)
    dones = 0
    for _ in range(10):
        act = 3.0 * (2.0 * torch.rand((64, 2), generator=g) - 1.0)
        fo, fr, fd, fi = full.step(act)
        parts = [s.step(act[i * 32:(i + 1) * 32]) for i, s in enumerate(shards)]
        assert torch.equal(fo, torch.cat([p[0] for p in parts])) and torch.equal(fr, torch.cat([p[1] for p in parts]))
        assert torch.equal(fd, torch.cat([p[2] for p in parts]))
        assert torch.equal(fi["TimeLimit.truncated"], torch.cat([p[3]["TimeLimit.truncated"] for p in parts]))
        lo, lr, ld, _ = late.step(act[24:])
        assert torch.equal(lo, fo[24:]) and torch.equal(lr, fr[24:]) and torch.equal(ld, fd[24:])
        dones += int(fd.sum())
    assert dones == 128 and int(full.ep.min()) == 2                 # the 10 steps did cross two resets
    assert torch.equal(full.ep, torch.cat([s.ep for s in shards])) and torch.equal(full.w[24:], late.w)


def test_rotation_stays_on_the_unit_circle_and_the_speed_clamped():
    """2000 steps of 3 U(-1, 1) actions at (64 envs, A = 2), episode length 128: |c^2 + s^2 - 1| <= 1e-6 throughout (a sanity margin on
    the Newton step: a float32 prototype gave 1.2e-7 after 5000 steps) and |w| <= 8 always."""
    env = _env(n=64, seed=11, episode_length=128)
    env.reset()
    g = torch.Generator().manual_seed(3)
    worst, fastest, clamped = 0.0, 0.0, 0
    for _ in range(2000):
        env.step(3.0 * (2.0 * torch.rand((64, 2), generator=g) - 1.0))
        worst = max(worst, float(((env.c * env.c + env.s * env.s) - 1.0).abs().max()))
        fastest = max(fastest, float(env.w.abs().max()))
        clamped += int((env.w.abs() == 8.0).sum())
    print(f"swingup: worst |c^2 + s^2 - 1| = {worst:.3e}, largest |w| = {fastest}, clamped joint-steps = {clamped}")
    assert worst <= 1e-6
    assert fastest <= 8.0
    # the clamp itself, where random torques do not reach it: a falling pendulum pushed on
    fall = _env(n=2, episode_length=128)
    fall.c.fill_(0.0); fall.s.fill_(1.0); fall.w.fill_(7.9)
    for _ in range(3):
        fall.step(torch.ones(2, 2))
        assert float(fall.w.abs().max()) <= 8.0
        assert float(((fall.c * fall.c + fall.s * fall.s) - 1.0).abs().max()) <= 1e-6
    fall2 = _env(n=2, episode_length=128)
    fall2.c.fill_(0.0); fall2.s.fill_(-1.0); fall2.w.fill_(-7.9)
    fall2.step(-torch.ones(2, 2))
    assert torch.equal(fall2.w, torch.full((2, 2), -8.0))


def test_state_round_trip():
    mk = lambda **kw: SwingUpVecEnv(16, 8, 2, device="cpu", **{**dict(seed=5, episode_length=6, env_offset=3), **kw})   # noqa: E731
    g = torch.Generator().manual_seed(1)
    acts = [3.0 * (2.0 * torch.rand((16, 2), generator=g) - 1.0) for _ in range(20)]
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
        with pytest.raises(ValueError, match="SwingUpVecEnv.load_state_dict"):
            mk(**kw).load_state_dict(state)
    with pytest.raises(ValueError, match="num_envs"):
        SwingUpVecEnv(17, 8, 2, device="cpu", seed=5, episode_length=6, env_offset=3).load_state_dict(state)
    bad = dict(state, w=torch.zeros(16, 3))
    with pytest.raises(ValueError, match="shape"):
        mk().load_state_dict(bad)


def test_controllers_bracket_the_task():
    """The yardsticks the learning test measures against, at 256 envs, (8, 2), seed 10000, length 128.  A float32 prototype of the same
    formulas with torch's own generator for the resets gave R_zero = -11.4 and R_energy = -2.3: the bars are R_energy > -4 and
    R_zero < -9, and a uniform random policy scores below the energy controller."""
    assert episode_return is pointmass_episode_return               # the measure is PointMass's, not a copy
    env = SwingUpVecEnv(256, 8, 2, device="cpu", seed=10_000, episode_length=128)
    r_zero, r_energy = episode_return(env, zero_policy(env)), episode_return(env, energy_policy(env))
    g = torch.Generator().manual_seed(0)
    r_rand = episode_return(env, lambda obs: 2.0 * torch.rand((256, 2), generator=g) - 1.0)
    print(f"swingup yardsticks: R_zero = {r_zero:.3f}, R_energy = {r_energy:.3f}, R_random = {r_rand:.3f}")
    assert r_energy > -4.0 and r_zero < -9.0, (r_zero, r_energy)
    assert r_rand < r_energy
    # the energy controller does swing up: after 96 steps every pendulum is upright
    obs = env.reset()
    pol = energy_policy(env)
    for _ in range(96):
        obs, _, _, _ = env.step(pol(obs))
    assert float(obs[:, :2].min()) > 0.9
    act = pol(obs)
    assert act.shape == (256, 2) and act.abs().max() <= 1.0
    assert torch.equal(zero_policy(env)(obs), torch.zeros(256, 2))


def test_config_surface():
    cfg = load_cfg(["task=swingup", "num_envs=8", "device=cpu"])
    assert dict(cfg.task) == dict(name="SwingUp", kind="swingup", obs_dim=8, act_dim=2, episode_length=128)
    env = create_task_env(cfg)
    assert isinstance(env, SwingUpVecEnv) and env.observation_space.shape == (8,) and env.action_space.shape == (2,)
    assert env.max_episode_length == 128 and env.num_envs == 8 and env.env_offset == 0 and env.seed == cfg.seed
    assert torch.equal(env.env_ids, torch.arange(8))
    big = create_task_env(load_cfg(["task=swingup", "task.obs_dim=88", "task.act_dim=16", "num_envs=8", "device=cpu"]), num_envs=5, env_offset=40)
    assert isinstance(big, SwingUpVecEnv) and (big.obs_dim, big.act_dim, big.num_envs, big.env_offset) == (88, 16, 5, 40)
    assert torch.equal(big.env_ids, torch.arange(40, 45))
    with pytest.raises(ValueError, match="obs_dim >= 3"):
        create_task_env(load_cfg(["task=swingup", "task.obs_dim=5", "task.act_dim=2", "device=cpu"]))
    with pytest.raises(ValueError):
        SwingUpVecEnv(4, 47, 16, device="cpu")
    for O, A in TASK_SHAPES.values():                               # every benchmarked shape fits
        assert SwingUpVecEnv(2, O, A, device="cpu").reset().shape == (2, O)
    # what existed before builds what it built before
    assert type(create_task_env(load_cfg(["task=pointmass", "num_envs=8", "device=cpu"]))) is PointMassVecEnv
    for ov in (["task=AllegroHand"], ["task=ShadowHand"], ["task.name=Toy"], ["task=synthetic"], []):
        assert type(create_task_env(load_cfg([*ov, "num_envs=8", "device=cpu"]))) is SyntheticVecEnv
    # the two messages that list what exists name the new kind; `pendulum` stays unknown
    with pytest.raises(ValueError, match="known kinds: .*swingup"):
        create_task_env(load_cfg(["task=swingup", "task.kind=pendulum", "device=cpu"]))
    with pytest.raises(ValueError, match="task=swingup"):
        load_cfg(["task=SwingDown", "device=cpu"])
    # reward_scale stays 1 on SwingUp
    from pql_amd.utils.common import preprocess_cfg
    cfg = load_cfg(["task=swingup", "algo=ddpg_algo", "device=cpu"])
    preprocess_cfg(cfg)
    assert cfg.algo.reward_scale == 1


def test_swingup_step_argument_checks():
    """PQLK_E_NULL / PQLK_E_SHAPE come back before anything is launched (0x1000 stands in for device memory)."""
    import ctypes as C
    from pql_amd import _lib as L
    P = C.c_void_p(0x1000)
    names = ("action", "c", "s", "w", "k", "ep", "next_obs", "reward", "done", "truncated")

    def step(n, O, A, null=None):
        ptrs = [None if name == null else P for name in names]
        return L.lib.pqlk_swingup_step(n, O, A, 1, 0, 5, *ptrs, None)

    for name in names:
        assert step(16, 8, 2, null=name) == 1, name                 # PQLK_E_NULL
    assert step(0, 8, 2) == 2 and step(-3, 8, 2) == 2 and step(16, 8, 0) == 2 and step(16, 5, 2) == 2   # PQLK_E_SHAPE
    assert step(16, 2 ** 23, 2) == 2                                # a block's rows must index with 32-bit ints
    assert L.lib.pqlk_strerror(1) and L.lib.pqlk_strerror(2)


def test_symbol_is_declared_exported_and_bound():
    import ctypes as C
    from pql_amd import _lib as L
    hdr = open(os.path.join(ROOT, "include", "pqlk.h")).read()
    decl = re.search(r"int pqlk_swingup_step\(([^;]*)\);", hdr)
    assert decl, "include/pqlk.h does not declare pqlk_swingup_step"
    params = [p.strip() for p in decl.group(1).replace("\n", " ").split(",")]
    assert [p.split()[-1].lstrip("*") for p in params] == ["n", "obs_dim", "act_dim", "seed", "env_offset", "episode_length", "action", "c", "s",
                                                           "w", "k", "ep", "next_obs", "reward", "done", "truncated", "stream"]
    res, args = L.PROTOTYPES["pqlk_swingup_step"]
    assert res is C.c_int and len(args) == len(params) == 17
    assert args[:6] == [C.c_int64, C.c_int32, C.c_int32, C.c_uint32, C.c_uint32, C.c_int32] and all(a is C.c_void_p for a in args[6:])
    fn = getattr(C.CDLL(os.fspath(L.LIB_FILE)), "pqlk_swingup_step")   # AttributeError if the library does not export it
    assert fn is not None and L.lib.pqlk_swingup_step.argtypes == args
    mk = open(os.path.join(ROOT, "pql_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS\s*=.*\bswingup\.hip\b", mk, re.M) and re.search(r"^SRCS\s*=.*\bpointmass\.hip\b", mk, re.M)
