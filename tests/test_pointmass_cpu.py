"""PointMass task, torch definition (pql_amd/envs/pointmass.py `_step_torch`) on the CPU: a known-answer vector, the two ways an
episode ends, the auto-reset, sharding of the env axis, the state round trip and the config surface.  No kernel is launched here;
tests/test_pointmass_gpu.py holds the HIP step to this definition bit for bit."""
import numpy as np
import pytest
import torch

from pql_amd.envs.pointmass import PointMassVecEnv, episode_return, pd_policy, zero_policy
from pql_amd.envs.synthetic import SyntheticVecEnv, create_task_env
from pql_amd.utils.cfg import load_cfg
from task_cases import u_np

F = np.float32


def _env(n=4, O=8, A=2, **kw):
    return PointMassVecEnv(n, O, A, device="cpu", **kw)


def _set(env, x=None, v=None, g=None):
    for name, val in (("x", x), ("v", v), ("g", g)):
        if val is not None:
            getattr(env, name).copy_(torch.tensor(val, dtype=torch.float32).expand_as(getattr(env, name)))


def _reset_obs(env, ep):
    """Start-of-episode observation recomputed from the hash with plain python integers: x = 2 u(e, ep, 11, j) - 1,
    g = 2 u(e, ep, 12, j) - 1, v = 0."""
    A = env.act_dim
    obs = np.zeros((env.num_envs, env.obs_dim), dtype=np.float32)
    for i in range(env.num_envs):
        e = env.env_offset + i
        for j in range(A):
            obs[i, j] = F(2.0) * u_np(env.seed, e, ep, 11, j) - F(1.0)
            obs[i, 2 * A + j] = F(2.0) * u_np(env.seed, e, ep, 12, j) - F(1.0)
    return torch.from_numpy(obs)


def test_known_answer_vector():
    """A = 2, O = 8; x = (0, 0.5), v = (0.1, -0.1), g = (1, 0), a = (1, -3) -> a clamps to (1, -1);
    v' = 0.8 v + 0.2 a = (0.28, -0.28); x' = x + 0.25 v' = (0.07, 0.43);
    d2 = ((0.07 - 1)^2 + 0.43^2) / 2 = (0.8649 + 0.1849) / 2 = 0.5249; action cost = 0.01 * (1 + 1) / 2 = 0.01; reward = -0.5349."""
    env = _env(n=3, episode_length=64)
    _set(env, x=[0.0, 0.5], v=[0.1, -0.1], g=[1.0, 0.0])
    obs, reward, done, info = env.step(torch.tensor([[1.0, -3.0]]).expand(3, 2))
    # the same operations, one fp32 rounding each, in numpy scalars
    a = [F(1.0), F(-1.0)]
    v1 = [F(0.8) * F(0.1) + F(0.2) * a[0], F(0.8) * F(-0.1) + F(0.2) * a[1]]
    x1 = [F(0.0) + F(0.25) * v1[0], F(0.5) + F(0.25) * v1[1]]
    d = [x1[0] - F(1.0), x1[1] - F(0.0)]
    d2 = (d[0] * d[0] + d[1] * d[1]) * (F(1.0) / F(2.0))
    a2 = (a[0] * a[0] + a[1] * a[1]) * (F(1.0) / F(2.0))
    want_r = -d2 - F(0.01) * a2 - F(0.0)
    want = torch.tensor([x1[0], x1[1], v1[0], v1[1], 1.0, 0.0, 0.0, 0.0], dtype=torch.float32)
    assert torch.equal(obs, want.expand(3, 8)), obs
    assert torch.equal(reward, torch.full((3,), float(want_r)))
    # ... and against the decimal values worked out above
    np.testing.assert_allclose(obs[0].numpy(), [0.07, 0.43, 0.28, -0.28, 1.0, 0.0, 0.0, 0.0], rtol=0, atol=1e-6)
    assert float(reward[0]) == pytest.approx(-0.5349, abs=1e-6)
    assert not done.any() and not info["TimeLimit.truncated"].any() and info["TimeLimit.truncated"].dtype == torch.bool
    assert torch.equal(env.k, torch.ones(3, dtype=torch.int32)) and torch.equal(env.ep, torch.zeros(3, dtype=torch.int32))
    assert obs.dtype == torch.float32 and reward.dtype == torch.float32 and done.dtype == torch.bool
    assert env.x.dtype == env.v.dtype == env.g.dtype == torch.float32 and env.k.dtype == env.ep.dtype == torch.int32


def test_reset_is_the_hash_of_seed_env_and_episode():
    env = _env(n=5, O=11, A=3, seed=7, env_offset=9)
    obs = env.reset()
    assert torch.equal(obs, _reset_obs(env, 0))
    assert obs[:, :3].abs().max() <= 1 and obs[:, 6:9].abs().max() <= 1 and torch.equal(obs[:, 3:6], torch.zeros(5, 3))
    assert torch.equal(obs[:, 9:], torch.zeros(5, 2))               # zero tail
    assert obs[:, :3].unique().numel() == 15                        # every env and column its own draw


def test_truncation_resets_into_the_next_episode():
    env = _env(n=6, seed=3, episode_length=3)
    env.reset()
    zero = torch.zeros(6, 2)
    for t in range(1, 4):
        obs, reward, done, info = env.step(zero)
        if t < 3:
            assert not done.any() and not info["TimeLimit.truncated"].any() and torch.equal(env.k, torch.full((6,), t, dtype=torch.int32))
    assert done.all() and info["TimeLimit.truncated"].all()
    assert torch.equal(env.ep, torch.ones(6, dtype=torch.int32)) and torch.equal(env.k, torch.zeros(6, dtype=torch.int32))
    assert torch.equal(obs, _reset_obs(env, 1))                     # next_obs of a done transition: the new episode's first observation
    assert not torch.equal(obs, _reset_obs(env, 0))
    for _ in range(3):
        obs, reward, done, info = env.step(zero)
    assert done.all() and torch.equal(obs, _reset_obs(env, 2))


def test_out_of_bounds_is_a_terminal_not_a_truncation():
    env = _env(n=2, episode_length=1)                                # the time limit is due in the same step: oob wins
    _set(env, x=[1.45, 0.0], v=[0.9, 0.0], g=[0.0, 0.0])
    obs, reward, done, info = env.step(torch.tensor([[1.0, 0.0]]).expand(2, 2))
    v1 = F(0.8) * F(0.9) + F(0.2) * F(1.0)
    x1 = F(1.45) + F(0.25) * v1                                      # 1.68 > 1.5
    assert x1 > 1.5
    d2 = (x1 * x1 + F(0.0)) * F(0.5)
    want = -d2 - F(0.01) * ((F(1.0) + F(0.0)) * F(0.5)) - F(1.0)
    assert done.all() and not info["TimeLimit.truncated"].any()
    assert torch.equal(reward, torch.full((2,), float(want))) and float(reward[0]) < -1.0 - 0.5 * 1.68 ** 2 + 1e-3
    assert torch.equal(env.ep, torch.ones(2, dtype=torch.int32)) and torch.equal(obs, _reset_obs(env, 1))
    env2 = _env(n=2, episode_length=5)
    _set(env2, x=[1.45, 0.0], v=[0.9, 0.0], g=[0.0, 0.0])
    _, r2, d2_, i2 = env2.step(torch.tensor([[-1.0, 0.0]]).expand(2, 2))   # braking: x' = 1.45 + 0.25 * 0.52 = 1.58 -> still out
    assert d2_.all() and not i2["TimeLimit.truncated"].any()
    env3 = _env(n=2, episode_length=5)
    _set(env3, x=[1.2, 0.0], v=[0.1, 0.0], g=[0.0, 0.0])
    _, r3, d3, _ = env3.step(torch.zeros(2, 2))
    assert not d3.any() and float(r3[0]) > -1.0                     # inside: no terminal, no penalty


def test_shards_reproduce_slices_of_the_global_env():
    mk = lambda n, off: PointMassVecEnv(n, 7, 2, device="cpu", seed=42, episode_length=4, env_offset=off)   # noqa: E731
    full, shards = mk(64, 0), [mk(32, 0), mk(32, 32)]
    o = full.reset()
    assert torch.equal(o, torch.cat([s.reset() for s in shards]))
    g = torch.Generator().manual_seed(0)
    dones = 0
    for _ in range(10):
        act = 3.0 * (2.0 * torch.rand((64, 2), generator=g) - 1.0)
        fo, fr, fd, fi = full.step(act)
        parts = [s.step(act[i * 32:(i + 1) * 32]) for i, s in enumerate(shards)]
        assert torch.equal(fo, torch.cat([p[0] for p in parts])) and torch.equal(fr, torch.cat([p[1] for p in parts]))
        assert torch.equal(fd, torch.cat([p[2] for p in parts]))
        assert torch.equal(fi["TimeLimit.truncated"], torch.cat([p[3]["TimeLimit.truncated"] for p in parts]))
        dones += int(fd.sum())
    assert dones >= 128 and int(full.ep.max()) >= 2                 # the 10 steps did cross resets
    assert torch.equal(full.ep, torch.cat([s.ep for s in shards]))


def test_state_round_trip():
    mk = lambda **kw: PointMassVecEnv(16, 8, 2, device="cpu", **{**dict(seed=5, episode_length=6, env_offset=3), **kw})   # noqa: E731
    g = torch.Generator().manual_seed(1)
    acts = [3.0 * (2.0 * torch.rand((16, 2), generator=g) - 1.0) for _ in range(20)]
    env = mk()
    env.reset()
    for a in acts[:9]:
        env.step(a)
    state = env.state_dict()
    kept = {k: v.clone() for k, v in state.items() if torch.is_tensor(v)}
    fresh = mk()
    fresh.load_state_dict(state)
    for a in acts[9:]:
        want, got = env.step(a), fresh.step(a)
        for w, h in zip(want[:3], got[:3]):
            assert torch.equal(w, h)
        assert torch.equal(want[3]["TimeLimit.truncated"], got[3]["TimeLimit.truncated"])
    for name in ("x", "v", "g", "k", "ep"):
        assert torch.equal(getattr(env, name), getattr(fresh, name))
        assert torch.equal(state[name], kept[name]), "state_dict must hand out copies, not the live tensors"
    assert int(env.ep.max()) >= 2
    for kw in (dict(seed=6), dict(env_offset=4)):
        with pytest.raises(ValueError):
            mk(**kw).load_state_dict(state)
    with pytest.raises(ValueError):
        PointMassVecEnv(17, 8, 2, device="cpu", seed=5, episode_length=6, env_offset=3).load_state_dict(state)


def test_config_surface():
    cfg = load_cfg(["task=pointmass", "num_envs=8", "device=cpu"])
    assert dict(cfg.task) == dict(name="PointMass", kind="pointmass", obs_dim=8, act_dim=2, episode_length=64)
    env = create_task_env(cfg)
    assert isinstance(env, PointMassVecEnv) and env.observation_space.shape == (8,) and env.action_space.shape == (2,)
    assert env.max_episode_length == 64 and env.num_envs == 8 and env.env_offset == 0 and env.seed == cfg.seed
    big = create_task_env(load_cfg(["task=pointmass", "task.obs_dim=88", "task.act_dim=16", "num_envs=8", "device=cpu"]), num_envs=5, env_offset=40)
    assert isinstance(big, PointMassVecEnv) and (big.obs_dim, big.act_dim, big.num_envs, big.env_offset) == (88, 16, 5, 40)
    with pytest.raises(ValueError):
        create_task_env(load_cfg(["task=pointmass", "task.obs_dim=5", "task.act_dim=2", "device=cpu"]))
    with pytest.raises(ValueError):
        PointMassVecEnv(4, 47, 16, device="cpu")
    from pql_amd.envs.synthetic import TASK_SHAPES
    for O, A in TASK_SHAPES.values():                               # every benchmarked shape fits
        assert PointMassVecEnv(2, O, A, device="cpu").reset().shape == (2, O)
    # what existed before keeps building the synthetic env
    for ov in (["task=AllegroHand"], ["task.name=Toy"], []):
        old = create_task_env(load_cfg([*ov, "num_envs=8", "device=cpu"]))
        assert type(old) is SyntheticVecEnv
    with pytest.raises(ValueError):
        create_task_env(load_cfg(["task=pointmass", "task.kind=pendulum", "device=cpu"]))
    # reward_scale stays 1 on PointMass (the reference's per-task table scales the Isaac tasks only)
    from pql_amd.utils.common import preprocess_cfg
    cfg = load_cfg(["task=pointmass", "algo=ddpg_algo", "device=cpu"])
    preprocess_cfg(cfg)
    assert cfg.algo.reward_scale == 1


def test_controllers_bracket_the_task():
    """Sanity of the yardsticks the learning test measures against: the PD controller beats doing nothing by a wide margin."""
    env = PointMassVecEnv(256, 8, 2, device="cpu", seed=10_000, episode_length=64)
    r_zero, r_pd = episode_return(env, zero_policy(env)), episode_return(env, pd_policy(env))
    assert r_pd > r_zero and r_pd > -6.0 and r_zero < -20.0, (r_zero, r_pd)
    g = torch.Generator().manual_seed(0)
    r_rand = episode_return(env, lambda obs: 2.0 * torch.rand((256, 2), generator=g) - 1.0)
    assert r_rand < r_pd


def test_pointmass_step_argument_checks():
    """PQLK_E_NULL / PQLK_E_SHAPE come back before anything is launched (0x1000 stands in for device memory)."""
    import ctypes as C
    from pql_amd import _lib as L
    P = C.c_void_p(0x1000)
    step = lambda n, O, A, act=P, trunc=P: L.lib.pqlk_pointmass_step(n, O, A, 1, 0, 5, act, P, P, P, P, P, P, P, P, trunc, None)   # noqa: E731
    assert step(16, 8, 2, act=None) == 1 and step(16, 8, 2, trunc=None) == 1
    assert step(0, 8, 2) == 2 and step(16, 8, 0) == 2 and step(16, 5, 2) == 2
