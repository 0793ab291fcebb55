"""SwingUp on the GPU: the one-launch HIP step against its torch definition (bit-equal), the rollout's n-step rows with real time-limit
truncations against the oracle's assembler, bit-exact resume of a DDPG run on the task, and a training run that improves a policy on a
task where neither the zero action nor a linear law does.  Run with `pytest -m gpu`."""
import importlib.util
import os
import sys
from collections import deque

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch.device("cuda:0")


@pytest.fixture(autouse=True)
def _keep_sigint():
    """The entry points' `main` installs a Ctrl+C handler (capture_keyboard_interrupt); here they run inside pytest's process."""
    import signal
    old = signal.getsignal(signal.SIGINT)
    yield
    signal.signal(signal.SIGINT, old)


def _load(path, name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, path))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# --------------------------------------------------------------------------- the kernel
def swingup_actions(n, A, steps, seed=0):
    """Per step (n, A): 3 U(-1, 1), so the action clamp is live; every fourth env pushes with a = +1 throughout."""
    g = torch.Generator().manual_seed(seed)
    acts = [3.0 * (2.0 * torch.rand((n, A), generator=g) - 1.0) for _ in range(steps)]
    for a in acts:
        a[::4] = 1.0
    return acts


@pytest.mark.parametrize("n,O,A,off", [(33, 8, 2, 7), (257, 88, 16, 0), (1024, 211, 20, 1024), (64, 6, 2, 0)])
def test_swingup_kernel_equals_torch_definition(dev, n, O, A, off):
    """`pqlk_swingup_step` vs `_step_torch` on the same device: observations, rewards, dones, truncations and every state tensor
    bit-equal after each of 12 steps with episode_length = 5 (every env is reset at least twice).  O = 6 = 3 A has no zero tail
    and O = 211 is no multiple of 4: both take the scalar store path (6 % 4 != 0 as well); 8 and 88 take the 16-byte one.  Every
    eighth env starts at w = +-7.9, so the speed clamp is met from both sides."""
    from pql_amd.envs.swingup import SwingUpVecEnv
    a = SwingUpVecEnv(n, O, A, device=dev, seed=1234, episode_length=5, env_offset=off)
    b = SwingUpVecEnv(n, O, A, device=dev, seed=1234, episode_length=5, env_offset=off)
    assert torch.equal(a.reset(), b.reset())
    for env in (a, b):
        env.w[::16] = 7.9
        env.w[8::16] = -7.9
    seen = dict(clamped=0, unclamped=0, truncated=0, running=0)
    for act in swingup_actions(n, A, 12):
        act = act.to(dev)
        oa, ra, da, ia = a.step(act)                 # the HIP launch
        ob, rb, db, ib = b._step_torch(act)          # the definition
        ta, tb = ia["TimeLimit.truncated"], ib["TimeLimit.truncated"]
        assert oa.dtype == torch.float32 and da.dtype == torch.bool and ta.dtype == torch.bool
        assert torch.equal(oa, ob) and torch.equal(ra, rb) and torch.equal(da, db) and torch.equal(ta, tb)
        assert torch.equal(da, ta)
        for name in ("c", "s", "w", "k", "ep"):
            assert torch.equal(getattr(a, name), getattr(b, name)), name
        assert torch.equal(oa[:, 3 * A:], torch.zeros((n, O - 3 * A), device=dev))
        assert float(a.w.abs().max()) <= 8.0
        running = ~da
        hit = (a.w.abs() == 8.0) & running.unsqueeze(1)          # (a reset env's w is a fresh draw in [-1, 1])
        seen["clamped"] += int(hit.sum())
        seen["unclamped"] += int(((a.w.abs() < 8.0) & running.unsqueeze(1)).sum())
        seen["truncated"] += int(ta.sum())
        seen["running"] += int(running.sum())
    assert min(seen.values()) > 0, f"the comparison did not see every kind of transition: {seen}"
    assert int(a.ep.min()) >= 2


# --------------------------------------------------------------------------- rollout integration
class _RecordingEnv:
    """Passes the env through and keeps every transition it returned (the wrapper idea of tests/test_pointmass_gpu.py)."""

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


@pytest.mark.parametrize("timeout", [True, False])
def test_rollout_nstep_rows_on_swingup(dev, timeout):
    """`PQLActor.explore_env` on SwingUp through `create_task_env` (nstep 3, two calls of T = 8, episode_length 5, 32 envs): the
    emitted n-step rows equal `oracle.pql_ref_cpu.NStepRef` fed the very same transitions, bit for bit.  Every done here is a time
    limit: with handle_timeout such a window carries done = 0 and bootstraps from the window's last next_obs; without it the row is
    terminal and stops at the truncated step.  Episode windows equal a host recomputation."""
    import detdata as dd
    from oracle import pql_ref_cpu as ref
    from pql_amd.algo.pql_actor import PQLActor
    from pql_amd.envs.swingup import SwingUpVecEnv
    from pql_amd.envs.synthetic import create_task_env
    from pql_amd.models.mlp import TanhMLPPolicy
    from pql_amd.utils.cfg import load_cfg
    N, O, A, n, T, WIN = 32, 8, 2, 3, 8, 20
    cfg = load_cfg(["task=swingup", "task.episode_length=5", f"num_envs={N}", f"algo.tracker_len={WIN}", "algo.v_learner_gpu=0",
                    "algo.p_learner_gpu=0", "algo.num_gpus=1", "sim_device=cuda:0", "device=cuda:0", f"algo.nstep={n}",
                    f"algo.handle_timeout={timeout}"])
    inner = create_task_env(cfg)
    assert isinstance(inner, SwingUpVecEnv) and inner.max_episode_length == 5
    env = _RecordingEnv(inner)
    actor = PQLActor(env, cfg)
    pol = TanhMLPPolicy((O,), A).to(dev)
    pol.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in dd.mlp_state(O, A, 17).items()})
    actor.set_actor(pol)
    actor.reset_agent()

    ns = ref.NStepRef(O, A, N, n)
    ret_win, len_win = deque([0.0] * WIN, maxlen=WIN), deque([0.0] * WIN, maxlen=WIN)
    cur_ret, cur_len = torch.zeros(N), torch.zeros(N)
    g = torch.Generator().manual_seed(5)
    obs, cursor = actor.obs.cpu(), 0
    assert torch.equal(obs, env.first_obs.cpu())
    trunc_only = 0
    for _call in range(2):
        draws = [torch.randn((N, A), generator=g) for _ in range(T)]
        p_data, v_data, steps = actor.explore_env(env, T, random=False, draws=[d.to(dev) for d in draws])
        torch.cuda.synchronize()
        sl = [torch.zeros((N, T, O)), torch.zeros((N, T, A)), torch.zeros((N, T, 1)), torch.zeros((N, T, O)), torch.zeros((N, T, 1))]
        raw_done = torch.zeros((N, T), dtype=torch.bool)
        for t in range(T):
            act, nobs, rew, done, trunc = env.log[cursor]; cursor += 1
            assert torch.equal(done, trunc)
            cur_ret += rew; cur_len += 1                                 # trackers see the env's own done
            ret_win.extend(cur_ret[done].tolist()); len_win.extend(cur_len[done].tolist())
            cur_ret[done] = 0; cur_len[done] = 0
            d = (done & ~trunc) if timeout else done                     # handle_timeout
            sl[0][:, t] = obs; sl[1][:, t] = act; sl[2][:, t, 0] = rew; sl[3][:, t] = nobs; sl[4][:, t, 0] = d.float()
            raw_done[:, t] = done
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
                w_done = raw_done[:, b:b + n]
                first = w_done.float().argmax(1)
                for e in torch.where(w_done.any(1))[0].tolist():
                    trunc_only += 1
                    if timeout:
                        assert got_done[b, e] == 0 and torch.equal(got_nobs[b, e], sl[3][e, b + n - 1])
                    else:
                        assert got_done[b, e] == 1 and torch.equal(got_nobs[b, e], sl[3][e, b + int(first[e])])
                assert not timeout or not got_done[b].any()
        assert actor.return_tracker.mean() == pytest.approx(float(np.mean(ret_win)), rel=1e-5, abs=1e-7)
        assert actor.step_tracker.mean() == pytest.approx(float(np.mean(len_win)), rel=1e-6)
        assert torch.equal(actor.obs.cpu(), obs)
    assert trunc_only > 0 and cursor == 2 * T
    assert sum(x != 0 for x in len_win) == WIN and set(len_win) == {5.0}    # 32 envs hit the time limit in ONE step: more than the window holds


# --------------------------------------------------------------------------- resume
def test_ddpg_resume_on_swingup_is_bit_exact(tmp_path):
    """scripts/train_baselines.py on SwingUp: 6 iterations + checkpoint, then resumed (same process) to 12 == 12 uninterrupted:
    the env's episode state (c, s, w, k, ep) travels in the checkpoint."""
    tb = _load("scripts/train_baselines.py", "train_baselines_su")
    from pql_amd.utils.cfg import load_cfg
    N = 32
    base = ["algo=ddpg_algo", "task=swingup", "task.episode_length=5", f"num_envs={N}", "algo.batch_size=64", "algo.memory_size=4000",
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


# --------------------------------------------------------------------------- it learns
# profiles/swingup_learning.json (tools/learn_pointmass.py --task swingup on an MI355X), DDPG at this shape, seeds 0..4, mean f by iteration
# count: 500: 0.494, 1000: 0.863, 2000: 0.972, 4000: 0.979, 8000: 0.998 -- 2000 is the smallest rung after which doubling adds less than
# 0.02 to the mean (it adds 0.007; from 1000 to 2000 it still adds 0.109).
# f of the five seeds at 2000 iterations: 0.9965, 0.9738, 0.9557, 0.9774, 0.9572.  The bar is half of the lowest: the yardsticks (zero
# action, energy controller) do not depend on any learner kernel, and the half covers seed-to-seed and box-to-box spread.
LEARN_ITERS = 2000      # rollout iterations (8 critic + 8 actor updates each); about 5 s on an MI355X
F_MIN = 0.5 * 0.9557


def test_ddpg_learns_swingup():
    """DDPG at (8, 2), 64 envs, batch 256, hidden [128, 128], episode_length 128, seed 0, 2000 iterations: the trained deterministic
    policy closes at least F_MIN of the gap between the zero action and the energy controller, both measured here on 256 evaluation
    envs.  Source of the bar: `runs` of profiles/swingup_learning.json, DDPG small, f of seeds 0-4 = 0.9965, 0.9738, 0.9557, 0.9774,
    0.9572; F_MIN = 0.5 x 0.9557 = 0.478."""
    lp = _load("tools/learn_pointmass.py", "learn_pointmass_su")
    r = lp.run("ddpg", "small", 0, LEARN_ITERS, task="swingup")
    print(f"swingup ddpg seed 0, {LEARN_ITERS} iterations: R={r['R']:.3f} R_zero={r['R_zero']:.3f} R_ctrl={r['R_ctrl']:.3f} f={r['f']:.4f} "
          f"wall={r['wall_s']}s")
    assert r["task"] == "swingup" and "R_pd" not in r
    assert r["R_ctrl"] > r["R_zero"]
    assert r["f"] >= F_MIN, r
