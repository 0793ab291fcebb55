"""What the tests of the hash-reset tasks share (tests/test_pointmass_*.py, tests/test_swingup_*.py, tests/test_task_*.py): the
counter-based uniform in plain python integers, the action generator, the recording env wrapper, the host recomputation of the
rollout's n-step rows and tracker windows, and the resume comparison.  Not collected as tests."""
import importlib.util
import os
from collections import deque

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


def load_script(path, name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, path))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def u_np(seed, e, ep, stream, j):
    """The counter-based uniform with plain python integers (independent of the envs' code)."""
    M = 0xFFFFFFFF

    def h32(x):
        x &= M
        x = ((x ^ (x >> 16)) * 0x7FEB352D) & M
        x = ((x ^ (x >> 15)) * 0x846CA68B) & M
        return x ^ (x >> 16)

    key = h32(e * 0x9E3779B1 + seed * 0x85EBCA77 + ep * 0xC2B2AE3D + stream * 0x27D4EB2F)
    h = h32(key * 0x165667B1 + j * 0x9E3779B1 + 0x5BD1E995)
    return (F(h) + F(0.5)) * F(1.0 / 4294967296.0)


def task_actions(n, A, steps, seed=0):
    """Per step (n, A): 3 U(-1, 1), so the action clamp is live; every fourth env pushes with a = +1 throughout (on PointMass some
    of them leave the box)."""
    g = torch.Generator().manual_seed(seed)
    acts = [3.0 * (2.0 * torch.rand((n, A), generator=g) - 1.0) for _ in range(steps)]
    for a in acts:
        a[::4] = 1.0
    return acts


class RecordingEnv:
    """Passes the env through and keeps every transition it returned."""

    def __init__(self, env):
        self.env, self.log, self.first_obs = env, [], None
        self.observation_space, self.action_space = env.observation_space, env.action_space
        self.max_episode_length, self.num_envs = env.max_episode_length, env.num_envs

    def reset(self):
        self.first_obs = self.env.reset()
        return self.first_obs

    def step(self, action):
        out = self.env.step(action)
        self.log.append(tuple(x.clone().cpu() for x in (action, out[0], out[1], out[2], out[3]["TimeLimit.truncated"])))
        return out


def check_rollout_nstep_rows(dev, task, env_cls, timeout, terminals, prepare=None):
    """`PQLActor.explore_env` on `task` through `create_task_env` (nstep 3, two calls of T = 8, episode_length 5, 32 envs): the
    emitted n-step rows equal `oracle.pql_ref_cpu.NStepRef` fed the very same transitions, bit for bit.  With handle_timeout a window
    that holds only a time limit carries done = 0 and bootstraps from the window's last next_obs (past the reset, as the reference
    does); without it the row is terminal and stops at the truncated step.  Episode windows equal a host recomputation.
    terminals: the task ends episodes early and both kinds of done must be seen; otherwise every done is a time limit and every
    episode is 5 steps long.  prepare(inner env): state edits after the actor's reset (the actor's obs is refreshed from them)."""
    import detdata as dd
    from oracle import pql_ref_cpu as ref
    from pql_amd.algo.pql_actor import PQLActor
    from pql_amd.envs.synthetic import create_task_env
    from pql_amd.models.mlp import TanhMLPPolicy
    from pql_amd.utils.cfg import load_cfg
    N, O, A, n, T, WIN = 32, 8, 2, 3, 8, 20
    cfg = load_cfg([f"task={task}", "task.episode_length=5", f"num_envs={N}", f"algo.tracker_len={WIN}", "algo.v_learner_gpu=0",
                    "algo.p_learner_gpu=0", "algo.num_gpus=1", "sim_device=cuda:0", "device=cuda:0", f"algo.nstep={n}",
                    f"algo.handle_timeout={timeout}"])
    inner = create_task_env(cfg)
    assert isinstance(inner, env_cls) and inner.max_episode_length == 5
    env = RecordingEnv(inner)
    actor = PQLActor(env, cfg)
    pol = TanhMLPPolicy((O,), A).to(dev)
    pol.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in dd.mlp_state(O, A, 17).items()})
    actor.set_actor(pol)
    actor.reset_agent()
    if prepare is not None:
        prepare(inner)
        actor.obs = inner._observe()

    ns = ref.NStepRef(O, A, N, n)
    ret_win, len_win = deque([0.0] * WIN, maxlen=WIN), deque([0.0] * WIN, maxlen=WIN)
    cur_ret, cur_len = torch.zeros(N), torch.zeros(N)
    g = torch.Generator().manual_seed(5)
    obs, cursor = actor.obs.cpu(), 0
    if prepare is None:
        assert torch.equal(obs, env.first_obs.cpu())
    trunc_only = terminal = 0
    for _call in range(2):
        draws = [torch.randn((N, A), generator=g) for _ in range(T)]
        p_data, v_data, steps = actor.explore_env(env, T, random=False, draws=[d.to(dev) for d in draws])
        torch.cuda.synchronize()
        sl = [torch.zeros((N, T, O)), torch.zeros((N, T, A)), torch.zeros((N, T, 1)), torch.zeros((N, T, O)), torch.zeros((N, T, 1))]
        raw_done, raw_trunc = torch.zeros((N, T), dtype=torch.bool), torch.zeros((N, T), dtype=torch.bool)
        for t in range(T):
            act, nobs, rew, done, trunc = env.log[cursor]; cursor += 1
            if not terminals:
                assert torch.equal(done, trunc)
            cur_ret += rew; cur_len += 1                                 # trackers see the env's own done (pql_actor.py:129-135)
            ret_win.extend(cur_ret[done].tolist()); len_win.extend(cur_len[done].tolist())
            cur_ret[done] = 0; cur_len[done] = 0
            d = (done & ~trunc) if timeout else done                     # handle_timeout (common.py:195-202)
            sl[0][:, t] = obs; sl[1][:, t] = act; sl[2][:, t, 0] = rew; sl[3][:, t] = nobs; sl[4][:, t, 0] = d.float()
            raw_done[:, t], raw_trunc[:, t] = done, trunc
            obs = nobs
        first_call = ns.count == 0
        want = ns.add(*sl)
        assert steps == T * N
        for name, got, exp in zip(("obs", "action", "reward", "next_obs", "done"), v_data, want):
            assert got.shape == exp.shape and torch.equal(got.cpu(), exp), name
        assert torch.equal(p_data.cpu(), want[0])
        # what the rows mean, read off the raw transitions (first call: block b of N rows is the window of steps b .. b + n - 1)
        if first_call:
            got_nobs, got_done = v_data[3].cpu().view(T - n + 1, N, O), v_data[4].cpu().view(T - n + 1, N)
            for b in range(T - n + 1):
                w_done, w_trunc = raw_done[:, b:b + n], raw_trunc[:, b:b + n]
                only_trunc = w_trunc.any(1) & ~(w_done & ~w_trunc).any(1)
                first = w_done.float().argmax(1)
                for e in torch.where(only_trunc)[0].tolist():
                    trunc_only += 1
                    if timeout:
                        assert got_done[b, e] == 0 and torch.equal(got_nobs[b, e], sl[3][e, b + n - 1])
                    else:
                        assert got_done[b, e] == 1 and torch.equal(got_nobs[b, e], sl[3][e, b + int(first[e])])
                for e in torch.where((w_done & ~w_trunc).any(1))[0].tolist():
                    terminal += 1
                    assert got_done[b, e] == 1
                if not terminals:
                    assert not timeout or not got_done[b].any()
        assert actor.return_tracker.mean() == pytest.approx(float(np.mean(ret_win)), rel=1e-5, abs=1e-7)
        assert actor.step_tracker.mean() == pytest.approx(float(np.mean(len_win)), rel=1e-6)
        assert torch.equal(actor.obs.cpu(), obs)
    assert trunc_only > 0 and cursor == 2 * T
    assert (terminal > 0) == terminals, (trunc_only, terminal)
    assert sum(x != 0 for x in len_win) == WIN                          # 32 envs hit the time limit in ONE step: more than the window holds
    if not terminals:
        assert set(len_win) == {5.0}


def check_ddpg_resume(tmp_path, task, module_name):
    """scripts/train_baselines.py on `task`: 6 iterations + checkpoint, then resumed (same process) to 12 == 12 uninterrupted: the
    env's episode state travels in the checkpoint."""
    tb = load_script("scripts/train_baselines.py", module_name)
    from pql_amd.utils.cfg import load_cfg
    N = 32
    base = ["algo=ddpg_algo", f"task={task}", "task.episode_length=5", f"num_envs={N}", "algo.batch_size=64", "algo.memory_size=4000",
            "algo.hidden_layers=[64, 64]"]
    upto = lambda iters: f"max_step={(32 + iters) * N - 1}"   # noqa: E731  (warm_up = 32 steps, then N env steps per iteration)
    a = tb.main(load_cfg(base + [upto(12)]))
    ck = tmp_path / "ck"
    b1 = tb.main(load_cfg(base + [upto(6), f"checkpoint.dir={ck}"]))
    assert (a["iters"], b1["iters"]) == (12, 6) and b1["actor_sha"] != a["actor_sha"]
    b2 = tb.main(load_cfg(base + [upto(12), f"resume={ck}"]))
    assert b2["resumed_from"]["global_steps"] == b1["global_steps"] and b2["resumed_from"]["actor_sha"] == b1["actor_sha"]
    for key in ("actor_sha", "critic_sha", "replay_sha", "global_steps", "iters", "train/critic_loss", "train/actor_loss", "train/return",
                "train/episode_length"):
        assert a[key] == b2[key], key


# --------------------------------------------------------------------------- the model: the reference's Tracker and its callers
class TrackerModel:
    """A deque of `max_len` zeros, `extend`, mean over all slots (what pql/utils/common.py's Tracker is), plus how many values it
    has been given, so that its content can be laid out like the device ring: value i of the deque sits in slot (count + i) % max_len."""

    def __init__(self, max_len):
        self.max_len, self.window, self.count = max_len, deque([0.0] * max_len, maxlen=max_len), 0

    def update(self, values):
        self.window.extend(values)
        self.count += len(values)

    def ring(self):
        return torch.from_numpy(np.roll(np.asarray(self.window, dtype=np.float32), self.count % self.max_len))

    def ptr(self):
        return self.count % self.max_len

    def mean(self):
        return float(self.ring().mean())   # fp32, summed in the ring's slot order like DeviceTracker.mean


class ModelTrackers:
    """update_tracker's info part (pql_actor.py:138-146, ac_base.py:88-101, evaluator.py:89-102) on the host, index lists and all."""

    def __init__(self, keys, steps, num_envs, window_len):
        self.keys, self.steps = list(keys), list(steps)
        self.trackers = [TrackerModel(window_len) for _ in keys]
        self.accs = [torch.zeros(num_envs, dtype=torch.float32) for _ in keys]

    def update(self, done, info):
        idx = torch.where(done.cpu())[0]
        for key, step, tr, acc in zip(self.keys, self.steps, self.trackers, self.accs):
            if key not in info:
                continue
            v = info[key].cpu().to(torch.float32)
            if step == "last":
                tr.update(v[idx].tolist())
            elif step in ("all-episode", "all"):
                acc += v
                tr.update(acc[idx].tolist())
                acc[idx] = 0
            elif step == "all-step":
                tr.update(v.tolist())
            else:
                raise AssertionError(step)


def assert_trackers_equal(got, want, where=""):
    """Windows (the discard slot left out), pointers, accumulators and means of an `InfoTrackers` against a `ModelTrackers`."""
    for i, key in enumerate(want.keys):
        t, m = got.trackers[i], want.trackers[i]
        assert torch.equal(t.ring[: t.max_len].cpu(), m.ring()), (where, key, "ring")
        assert int(t.ptr.item()) == m.ptr(), (where, key, "ptr")
        if got.accs[i] is not None:
            assert torch.equal(got.accs[i].cpu(), want.accs[i]), (where, key, "acc")
        assert float(t.ring[: t.max_len].cpu().mean()) == m.mean(), (where, key, "mean")


def scripted_steps(n, n_float, n_bool, seed=0, missing=()):
    """Six (done, info) steps: nobody finishes, everybody, then about 30 % scattered four times.  info holds float keys f0.., bool
    keys b0.. and one uint8 key u0; the keys in `missing` are absent on steps 1 and 3."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for t in range(6):
        done = torch.zeros(n, dtype=torch.bool) if t == 0 else torch.ones(n, dtype=torch.bool) if t == 1 else torch.rand(n, generator=g) < 0.3
        info = {f"f{i}": 4.0 * torch.rand(n, generator=g) - 1.0 for i in range(n_float)}
        info.update({f"b{i}": torch.rand(n, generator=g) < 0.4 for i in range(n_bool)})
        info["u0"] = (torch.rand(n, generator=g) < 0.5).to(torch.uint8)
        if t in (1, 3):
            for key in missing:
                del info[key]
        out.append((done, info))
    return out


def pointmass_channels_np(obs, act, A):
    """(dist2, oob) of the step that `act` (N, A) takes from the state in the observation rows `obs` = [x | v | g | 0 ...]: the
    formulas of pql_amd/envs/pointmass.py's docstring in numpy float32, one rounding per operation, sums in index order."""
    o = obs.cpu().numpy().astype(F)
    x, v, g = o[:, :A], o[:, A:2 * A], o[:, 2 * A:3 * A]
    a = np.clip(act.cpu().numpy().astype(F), F(-1), F(1))
    vn = F(0.8) * v + F(0.2) * a
    xn = x + F(0.25) * vn
    df = xn - g
    sq = df * df
    d2 = sq[:, 0]
    for j in range(1, A):
        d2 = d2 + sq[:, j]
    d2 = d2 * (F(1.0) / F(A))
    return torch.from_numpy(d2.astype(F)), torch.from_numpy((np.abs(xn) > F(1.5)).any(1))


def pointmass_infos_from_log(first_obs, log, A):
    """[(done, info)] of the transitions `task_cases.RecordingEnv` kept, the channels recomputed on the host."""
    out, obs = [], first_obs.cpu()
    for act, nobs, _rew, done, trunc in log:
        d2, oob = pointmass_channels_np(obs, act, A)
        assert torch.equal(oob, done & ~trunc)   # leaving the box is PointMass's only terminal
        out.append((done, {"dist2": d2, "oob": oob.to(torch.float32), "TimeLimit.truncated": trunc}))
        obs = nobs
    return out


C4, S3, S5 = F(0.041666668), F(0.16666667), F(0.008333334)
# --------------------------------------------------------------------------- the definition, once more, in numpy scalars
def rot_np(c, s, d):
    d2 = d * d
    cd = F(1.0) - d2 * (F(0.5) - d2 * C4)
    sd = d * (F(1.0) - d2 * (S3 - d2 * S5))
    cn = c * cd - s * sd
    sn = s * cd + c * sd
    m = F(1.5) - F(0.5) * (cn * cn + sn * sn)
    return cn * m, sn * m


def tip_np(c, s):
    """(ex, ey) of one env's chain c, s (A,)."""
    A = len(c)
    C, S = c[0], s[0]
    x, y = C, S
    for j in range(1, A):
        C, S = C * c[j] - S * s[j], S * c[j] + C * s[j]
        x, y = x + C, y + S
    inv_a = F(1.0) / F(A)
    return x * inv_a - F(0.6), y * inv_a
