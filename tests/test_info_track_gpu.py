"""info_track_keys on the GPU: the `_info` step entries against the torch definition, `pqlk_rollout_info` against the torch form of
`InfoTrackers`, the rollout, the evaluator, resume and the training scripts with keys set.  Every comparison is between fp32 values
produced by the same operations in the same order, so it is exact.  Run with `pytest -m gpu`."""
import json
import os

import numpy as np
import pytest
import torch

import detdata as dd
import task_cases as tc
from support import dev  # noqa: F401
from task_cases import ModelTrackers, assert_trackers_equal, pointmass_infos_from_log, scripted_steps

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(autouse=True)
def _keep_sigint():
    """The entry points' `main` installs a Ctrl+C handler (capture_keyboard_interrupt); here they run inside pytest's process."""
    import signal
    old = signal.getsignal(signal.SIGINT)
    yield
    signal.signal(signal.SIGINT, old)


@pytest.fixture
def hip_launches(monkeypatch):
    """Counts the entries that went through `pqlk_rollout_info` and its launches."""
    from pql_amd import _lib as L
    from pql_amd.utils.info_track import InfoTrackers
    seen = dict(entries=0, launches=0)
    inner = InfoTrackers._update_hip

    def counting(self, done, entries):
        seen["entries"] += len(entries)
        seen["launches"] += -(-len(entries) // L.INFO_MAX_KEYS)
        return inner(self, done, entries)

    monkeypatch.setattr(InfoTrackers, "_update_hip", counting)
    return seen


# --------------------------------------------------------------------------- the step kernels
@pytest.mark.parametrize("n,O,A,off", [(33, 8, 2, 7), (257, 88, 16, 0), (1024, 211, 20, 1024)])
@pytest.mark.parametrize("kind", ["pointmass", "swingup"])
def test_step_info_kernel_equals_torch_definition(dev, kind, n, O, A, off):
    """`pqlk_<task>_step_info` vs `_step_torch` on the same device, 12 steps at episode_length = 5: the info block, observations,
    rewards, dones, truncations and every state tensor bit-equal; a twin env stepped through the plain entry stays bit-equal in
    everything but info.  The run sees every kind of transition the task has (SwingUp has no terminal)."""
    from pql_amd.envs.synthetic import TASK_ENVS
    mk = lambda **kw: TASK_ENVS[kind](n, O, A, device=dev, seed=1234, episode_length=5, env_offset=off, **kw)   # noqa: E731
    a, b, c = mk(info_channels=True), mk(info_channels=True), mk()
    assert torch.equal(a.reset(), b.reset()) and torch.equal(a.reset(), c.reset())
    seen = dict(terminal=0, truncated=0, running=0)
    for act in tc.task_actions(n, A, 12):
        act = act.to(dev)
        oa, ra, da, ia = a.step(act)                 # the HIP launch with INFO
        ob, rb, db, ib = b._step_torch(act)          # the definition
        oc, rc, dc, ic = c.step(act)                 # the HIP launch without
        assert set(ia) == set(ib) == {"TimeLimit.truncated", *a.info_keys} and set(ic) == {"TimeLimit.truncated"}
        block = torch.stack([ia[k] for k in a.info_keys])
        assert block.dtype == torch.float32 and ia[a.info_keys[1]].is_contiguous()
        assert torch.equal(block, torch.stack([ib[k] for k in a.info_keys])), [k for k in a.info_keys if not torch.equal(ia[k], ib[k])]
        ta = ia["TimeLimit.truncated"]
        for o, r, d, t, env in ((ob, rb, db, ib["TimeLimit.truncated"], b), (oc, rc, dc, ic["TimeLimit.truncated"], c)):
            assert torch.equal(oa, o) and torch.equal(ra, r) and torch.equal(da, d) and torch.equal(ta, t)
            for name in (*a._STATE, "k", "ep"):
                assert torch.equal(getattr(a, name), getattr(env, name)), name
        seen["terminal"] += int((da & ~ta).sum())
        seen["truncated"] += int(ta.sum())
        seen["running"] += int((~da).sum())
    if kind == "swingup":
        assert seen.pop("terminal") == 0
    assert min(seen.values()) > 0, f"the comparison did not see every kind of transition: {seen}"
    assert int(a.ep.min()) >= 2


# --------------------------------------------------------------------------- the info kernel
def _pair(keys, steps, n, window, dev):
    from pql_amd.utils.info_track import InfoTrackers
    return InfoTrackers(keys, steps, n, window, dev), InfoTrackers(keys, steps, n, window, dev)


def _run_pair(hip, ref, script, dev, n, window):
    """Feeds both forms the same steps; rings, pointers and accumulators bit-equal after every step.  The kernel never writes the
    discard slot behind the window (the torch form parks what it drops there)."""
    most = 0
    for t, (done, info) in enumerate(script):
        done, info = done.to(dev), {k: v.to(dev) for k, v in info.items()}
        hip.update(done, info)
        for i, key in enumerate(ref.keys):
            if key in info:
                ref._update_torch(i, done, info[key])
        for i, key in enumerate(ref.keys):
            a, b = hip.trackers[i], ref.trackers[i]
            assert torch.equal(a.ring[:window], b.ring[:window]), (t, key, hip.spellings[i], "ring")
            assert torch.equal(a.ptr, b.ptr) and 0 <= int(a.ptr) < window, (t, key, "ptr")
            assert float(a.ring[window]) == 0.0, (t, key, "discard slot")
            assert (hip.accs[i] is None) == (ref.accs[i] is None)
            assert hip.accs[i] is None or torch.equal(hip.accs[i], ref.accs[i]), (t, key, "acc")
        most = max(most, int(done.sum()))
    return most


@pytest.mark.parametrize("window", [7, 100])
@pytest.mark.parametrize("n", [33, 1025, 2500])   # less than one chunk of 1024 envs | one env past it | several chunks
def test_rollout_info_kernel_equals_torch_form(dev, hip_launches, n, window):
    """`pqlk_rollout_info` vs the torch form on the same device over six steps (nobody / everybody / about 30 % finish, so the
    pointers wrap): one key in every mode with a float32 and with a bool source, 8 keys in one launch (all four spellings, float32 /
    bool / uint8 sources, one key absent on two steps) and 9 keys in two.  At N = 2500 more episodes finish in one step than either
    window holds."""
    script = scripted_steps(n, 4, 2, seed=n + window, missing=("f3",))
    for mode in ("last", "all-episode", "all", "all-step"):
        for key in ("f0", "b0"):
            hip, ref = _pair([key], [mode], n, window, dev)
            _run_pair(hip, ref, script, dev, n, window)
    assert hip_launches == dict(entries=8 * 6, launches=8 * 6)
    keys8 = ["f0", "f1", "f1", "f2", "b0", "u0", "f3", "b1"]
    steps8 = ["last", "all-episode", "all", "all-step", "last", "all-episode", "last", "all-step"]
    hip_launches.update(entries=0, launches=0)
    most = _run_pair(*_pair(keys8, steps8, n, window, dev), script, dev, n, window)
    assert hip_launches == dict(entries=8 * 6 - 2, launches=6)       # one launch per step for all keys
    hip_launches.update(entries=0, launches=0)
    hip9, ref9 = _pair(keys8 + ["b0"], steps8 + ["all"], n, window, dev)
    _run_pair(hip9, ref9, script, dev, n, window)
    assert hip_launches == dict(entries=9 * 6 - 2, launches=4 * 2 + 2 * 1)   # 9 entries = 8 + 1; 8 on the two steps without f3
    assert most == n and (n < 2500 or sorted(int(d.sum()) for d, _ in script)[-2] > 100)
    # ... and the torch form is the one the deque model pins down (tests/test_info_track_cpu.py), here on the device
    want = ModelTrackers(keys8 + ["b0"], steps8 + ["all"], n, window)
    for done, info in script:
        want.update(done, info)
    assert_trackers_equal(hip9, want, "after six steps")


def test_rollout_info_takes_other_values_through_the_torch_form(dev, hip_launches):
    """What the kernel does not take (float64 values, a strided view, a float `done`) goes through the torch form, same result."""
    n, window = 33, 7
    script = scripted_steps(n, 2, 1, seed=1)
    hip, ref = _pair(["f0", "f1", "b0"], ["last", "all", "all-step"], n, window, dev)
    for done, info in script:
        done = done.to(dev)
        wide = torch.stack((info["f1"], info["f1"]), 1).to(dev)
        hip.update(done, {"f0": info["f0"].to(dev).double(), "f1": wide[:, 0], "b0": info["b0"].to(dev)})
        ref.update(done.float(), {k: v.to(dev) for k, v in info.items() if k != "u0"})
    assert hip_launches == dict(entries=6, launches=6)   # b0 alone on the first pair; nothing with a float done
    for a, b in zip(hip.trackers, ref.trackers):
        assert torch.equal(a.ring[:window], b.ring[:window]) and torch.equal(a.ptr, b.ptr)
    assert torch.equal(hip.accs[1], ref.accs[1])


# --------------------------------------------------------------------------- the rollout
KEYS = ["oob", "dist2", "TimeLimit.truncated", "dist2"]
STEPS = ["last", "all-episode", "last", "all-step"]
KEY_ARGS = [f"info_track_keys=[{', '.join(KEYS)}]", f"info_track_step=[{', '.join(STEPS)}]"]


def _policy(O, A, dev, seed=17):
    from pql_amd.models.mlp import TanhMLPPolicy
    pol = TanhMLPPolicy((O,), A).to(dev)
    pol.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in dd.mlp_state(O, A, seed).items()})
    return pol


def _leave_the_box(inner):
    inner.x[::4, 0], inner.v[::4, 0] = 1.4, 0.9       # as test_rollout_nstep_rows_with_real_truncations: out in the first step
    inner.x[1::8, 0], inner.v[1::8, 0] = 1.25, 0.9    # ... and some a step or two later, or not at all


def test_rollout_tracks_info_keys_without_touching_the_rest(dev, hip_launches, monkeypatch):
    """`PQLActor.explore_env` on PointMass, 32 envs, two calls of T = 8, episode_length 5, some envs prepared to leave the box: every
    info window equals a host recomputation from the transitions `task_cases.RecordingEnv` kept (32 envs hit the time limit in one
    step and the `all-step` entry brings 32 values every step: more than the window of 20 holds); slabs, n-step rows, return and length windows are bit-equal to a twin actor without
    keys; and an actor whose bookkeeping goes through `update_tracker` ends with the same windows: one update per env step and key
    whichever path ran."""
    from pql_amd.algo.pql_actor import PQLActor
    from pql_amd.envs.synthetic import create_task_env
    from pql_amd.utils.cfg import load_cfg
    N, O, A, T, WIN = 32, 8, 2, 8, 20
    base = ["task=pointmass", "task.episode_length=5", f"num_envs={N}", f"algo.tracker_len={WIN}", "algo.v_learner_gpu=0",
            "algo.p_learner_gpu=0", "algo.num_gpus=1", "sim_device=cuda:0", "device=cuda:0", "algo.nstep=3", "algo.handle_timeout=True"]

    def build(args, torch_bookkeeping=False):
        cfg = load_cfg(base + args)
        inner = create_task_env(cfg)
        env = tc.RecordingEnv(inner)
        actor = PQLActor(env, cfg)
        if torch_bookkeeping:
            monkeypatch.setattr(actor, "_bookkeep_hip", lambda *a, **k: False)
        actor.set_actor(_policy(O, A, dev))
        actor.reset_agent()
        _leave_the_box(inner)
        actor.obs = inner._observe()
        return actor, env, inner

    with_keys, env, inner = build(KEY_ARGS)
    plain, _, plain_inner = build([])
    by_torch, _, _ = build(KEY_ARGS, torch_bookkeeping=True)
    assert inner.info_channels and not plain_inner.info_channels and len(plain.info_trackers) == 0
    assert with_keys.info_trackers.window_len == WIN and with_keys.add_info_tracker_log({}) == {k: 0.0 for k in KEYS}
    assert plain.add_info_tracker_log({"x": 1}) == {"x": 1}
    want = ModelTrackers(KEYS, STEPS, N, WIN)
    g = torch.Generator().manual_seed(5)
    first_obs, cursor = with_keys.obs.clone(), 0
    for _call in range(2):
        draws = [torch.randn((N, A), generator=g).to(dev) for _ in range(T)]
        outs = [actor.explore_env(actor.env, T, random=False, draws=draws) for actor in (with_keys, plain, by_torch)]
        torch.cuda.synchronize()
        for other in outs[1:]:
            assert torch.equal(outs[0][0], other[0]) and outs[0][2] == other[2] == T * N
            for name, x, y in zip(("obs", "action", "reward", "next_obs", "done"), outs[0][1], other[1]):
                assert torch.equal(x, y), name
        for other in (plain, by_torch):
            for name, slab in with_keys._slabs[T].items():
                assert torch.equal(slab, other._slabs[T][name]), name
            for attr in ("return_tracker", "step_tracker"):
                mine, theirs = getattr(with_keys, attr), getattr(other, attr)
                assert torch.equal(mine.ring[:WIN], theirs.ring[:WIN]) and torch.equal(mine.ptr, theirs.ptr), attr
            assert torch.equal(with_keys.current_returns, other.current_returns)
        for done, info in pointmass_infos_from_log(first_obs if cursor == 0 else env.log[cursor - 1][1], env.log[cursor:cursor + T], A):
            want.update(done, info)
        cursor += T
        assert_trackers_equal(with_keys.info_trackers, want, f"call {_call}")
        assert_trackers_equal(by_torch.info_trackers, want, f"call {_call}, update_tracker path")
    assert hip_launches == dict(entries=2 * 2 * T * len(KEYS), launches=2 * 2 * T)   # one launch per env step for all four entries
    dones = torch.stack([d for _a, _o, _r, d, _t in env.log])
    truncs = torch.stack([t for _a, _o, _r, _d, t in env.log])
    assert int((dones & ~truncs).sum()) > 0 and int(truncs.sum()) > 0 and int((~dones).sum()) > 0   # terminal, truncated, running
    log = with_keys.add_info_tracker_log({})
    assert set(log) == {"oob", "dist2", "TimeLimit.truncated"} and 0 <= log["oob"] <= 1
    assert log["dist2"] == pytest.approx(want.trackers[3].mean(), rel=1e-6)   # (the device sums the window's 20 values in its own order)
    assert log["oob"] + log["TimeLimit.truncated"] <= 1.0 + 1e-6
    # the training state carries the windows: into a fresh actor, and not into one that tracks other keys
    st = with_keys.training_state()
    fresh, _, _ = build(KEY_ARGS)
    fresh.load_training_state(st)
    assert_trackers_equal(fresh.info_trackers, want, "restored")
    other, _, _ = build(["info_track_keys=[oob]", "info_track_step=[last]"])
    with pytest.raises(ValueError, match=r"'dist2'.*\['oob'\]"):
        other.load_training_state(st)
    plain_st = plain.training_state()
    assert "info_trackers" not in plain_st
    fresh.load_training_state(plain_st)   # a checkpoint without the entry: zeroed trackers
    assert all(float(t.ring.abs().sum()) == 0 for t in fresh.info_trackers.trackers)


def test_ppo_tracks_info_keys(dev, hip_launches):
    """`AgentPPO.explore_env` on PointMass with keys: the windows equal the host recomputation from the recorded transitions."""
    from pql_amd.algo.ppo import AgentPPO
    from pql_amd.envs.synthetic import create_task_env
    from pql_amd.utils.cfg import load_cfg
    N, A, T, WIN = 32, 2, 8, 20
    cfg = load_cfg(["algo=ppo_algo", "task=pointmass", "task.episode_length=5", f"num_envs={N}", f"algo.tracker_len={WIN}",
                    "sim_device=cuda:0", "device=cuda:0", "algo.hidden_layers=[64, 64]"] + KEY_ARGS)
    env = tc.RecordingEnv(create_task_env(cfg))
    agent = AgentPPO(env, cfg)
    first_obs = agent.reset_agent().clone()
    agent.explore_env(env, T)
    want = ModelTrackers(KEYS, STEPS, N, WIN)
    for done, info in pointmass_infos_from_log(first_obs, env.log, A):
        want.update(done, info)
    assert_trackers_equal(agent.info_trackers, want)
    assert hip_launches == dict(entries=T * len(KEYS), launches=T)
    assert set(agent.add_info_tracker_log({})) == set(KEYS) and float(agent.success_tracker.ring.abs().sum()) == 0


# --------------------------------------------------------------------------- the evaluator
def test_evaluator_reports_info_keys_from_zero_each_time(dev, tmp_path):
    """`Evaluator` (the in-process engine on its own stream) on PointMass with two keys: eval/<key> equals the host recomputation
    from the recorded transitions, and a second evaluation of the same policy reports the same numbers -- it does not see the first
    one's windows or partial sums (the reference would)."""
    from types import SimpleNamespace
    from pql_amd.envs.synthetic import create_task_env
    from pql_amd.utils.cfg import load_cfg
    from pql_amd.utils.evaluator import Evaluator
    n, O, A, EP = 48, 8, 2, 12
    keys, steps = ["dist2", "oob"], ["all-episode", "last"]
    cfg = load_cfg(["task=pointmass", f"task.episode_length={EP}", f"eval_num_envs={n}", "device=cuda:0", "eval_steps_per_poll=5",
                    "algo.obs_norm=False", f"info_track_keys=[{', '.join(keys)}]", f"info_track_step=[{', '.join(steps)}]"])
    rec = {}

    def make_env(c, num_envs=None):
        rec["env"] = tc.RecordingEnv(create_task_env(c, num_envs=num_envs))
        return rec["env"]

    ev = Evaluator(cfg, wandb_run=SimpleNamespace(dir=str(tmp_path)), create_task_env_func=make_env)
    actor = _policy(O, A, dev)
    actor.arena.data.mul_(40.0)   # saturated actions: some envs are pushed out of the box
    results = []
    for i in range(2):
        ev.eval_policy(actor, None, step=i)
        polls = 0
        while not ev.parent.poll():
            polls += 1
            assert polls < 100000
        results.append(ev.parent.recv())
    ev.close()
    env = rec["env"]
    assert len(env.log) == 2 * EP
    for r, result in enumerate(results):
        want = ModelTrackers(keys, steps, n, n)
        for done, info in pointmass_infos_from_log(env.first_obs, env.log[EP * r:EP * (r + 1)], A):
            want.update(done, info)
        for key, tr in zip(keys, want.trackers):
            assert result[f"eval/{key}"] == float(np.mean(tr.ring().numpy().astype(np.float64))), key
        assert set(result) == {"eval/return", "eval/episode_length", "eval/dist2", "eval/oob"}
    assert 0 <= results[0]["eval/oob"] <= 1 and results[0]["eval/dist2"] > 0
    assert results[0] == results[1]


# --------------------------------------------------------------------------- resume
def test_ddpg_resume_with_info_keys_is_bit_exact(tmp_path):
    """scripts/train_baselines.py, DDPG on PointMass with keys: 6 iterations + checkpoint + 6 resumed == 12 uninterrupted, on the
    info rings, pointers and accumulators as well as on what tests/task_cases.py's check_ddpg_resume compares."""
    tb = tc.load_script("scripts/train_baselines.py", "train_baselines_info")
    from pql_amd.utils.cfg import load_cfg
    N = 32
    base = ["algo=ddpg_algo", "task=pointmass", "task.episode_length=5", f"num_envs={N}", "algo.batch_size=64", "algo.memory_size=4000",
            "algo.hidden_layers=[64, 64]", "info_track_keys=[oob, dist2, dist2]", "info_track_step=[last, all-episode, all-step]"]
    upto = lambda iters: f"max_step={(32 + iters) * N - 1}"   # noqa: E731  (warm_up = 32 steps, then N env steps per iteration)
    kept = {}

    def keep(name):
        def on_finish(agent):
            torch.cuda.synchronize()
            kept[name] = agent.info_trackers.training_state()
        return on_finish

    a = tb.main(load_cfg(base + [upto(12)]), on_finish=keep("a"))
    ck = tmp_path / "ck"
    b1 = tb.main(load_cfg(base + [upto(6), f"checkpoint.dir={ck}"]), on_finish=keep("b1"))
    assert (a["iters"], b1["iters"]) == (12, 6) and b1["actor_sha"] != a["actor_sha"]
    b2 = tb.main(load_cfg(base + [upto(12), f"resume={ck}"]), on_finish=keep("b2"))
    assert b2["resumed_from"]["global_steps"] == b1["global_steps"]
    for key in ("actor_sha", "critic_sha", "replay_sha", "global_steps", "iters", "train/critic_loss", "train/actor_loss", "train/return",
                "train/episode_length"):
        assert a[key] == b2[key], key
    sa, sb, s1 = kept["a"], kept["b2"], kept["b1"]
    assert sa["keys"] == sb["keys"] == ["oob", "dist2", "dist2"]
    moved = False
    for i in range(3):
        assert torch.equal(sa["trackers"][i]["ring"][:-1], sb["trackers"][i]["ring"][:-1]) and torch.equal(sa["trackers"][i]["ptr"], sb["trackers"][i]["ptr"])
        assert (sa["accs"][i] is None) == (i != 1) and (sa["accs"][i] is None or torch.equal(sa["accs"][i], sb["accs"][i]))
        moved |= not torch.equal(sa["trackers"][i]["ring"][:-1], s1["trackers"][i]["ring"][:-1])
    assert moved and float(sa["accs"][1].abs().sum()) > 0   # the second half did change the windows, and sums were under way


# --------------------------------------------------------------------------- the training scripts
def _jsonl(path):
    return [json.loads(line) for line in open(path)]


SMALL = ["num_envs=64", "algo.batch_size=256", "algo.hidden_layers=[128, 128]", "algo.memory_size=20000", "task.episode_length=16"]


@pytest.mark.parametrize("task,keys,steps", [("pointmass", ["oob", "dist2", "TimeLimit.truncated"], ["last", "all-episode", "last"]),
                                             ("swingup", ["upright", "effort", "TimeLimit.truncated"], ["all-step", "all-episode", "last"])])
def test_train_pql_logs_info_keys(tmp_path, task, keys, steps):
    """scripts/train_pql.py for 48 iterations: the JSONL log carries each bare key (the rollout's windows) and eval/<key> (the
    evaluator's), within the ranges the channels have."""
    tp = tc.load_script("scripts/train_pql.py", f"train_pql_info_{task}")
    from pql_amd.utils.cfg import load_cfg
    log = tmp_path / "log.jsonl"
    cfg = load_cfg([f"task={task}", *SMALL, "algo.num_gpus=1", f"max_step={64 * (32 + 48) - 1}", f"logging.jsonl={log}", "eval_num_envs=32",
                    "algo.eval_freq=24", f"info_track_keys=[{', '.join(keys)}]", f"info_track_step=[{', '.join(steps)}]"])
    out = tp.main(cfg)
    assert out["rollout_iterations"] == 48
    rows = _jsonl(log)
    train, evals = [r for r in rows if "train/return" in r], [r for r in rows if "eval/return" in r]
    assert len(train) == 24 and len(evals) == 2
    for r in train:
        assert set(keys) <= set(r)
    for r in evals:
        assert {f"eval/{k}" for k in keys} <= set(r)
    for r, prefix in [(train[-1], ""), (evals[-1], "eval/")]:
        assert 0 <= r[prefix + "TimeLimit.truncated"] <= 1
        if task == "pointmass":
            assert 0 <= r[prefix + "oob"] <= 1 and r[prefix + "oob"] + r[prefix + "TimeLimit.truncated"] <= 1 + 1e-6
            assert r[prefix + "dist2"] > 0
        else:
            assert -1 <= r[prefix + "upright"] <= 1 and 0 <= r[prefix + "effort"] <= 16
    assert train[-1]["TimeLimit.truncated"] > 0   # episodes of 16 steps did finish within 80


@pytest.mark.parametrize("algo", ["ppo_algo", "sac_algo"])
def test_train_baselines_logs_info_keys(tmp_path, algo):
    """scripts/train_baselines.py (PPO through `AgentPPO`, SAC through `ActorCriticBase`) on PointMass with keys: every logged row
    carries the bare keys (this script has no evaluator, so no eval/<key>)."""
    tb = tc.load_script("scripts/train_baselines.py", f"train_baselines_info_{algo}")
    from pql_amd.utils.cfg import load_cfg
    log = tmp_path / "log.jsonl"
    iters, per_iter = (4, 64 * 16) if algo == "ppo_algo" else (48, 64)
    small = [x for x in SMALL if algo != "ppo_algo" or "memory_size" not in x]
    cfg = load_cfg([f"algo={algo}", "task=pointmass", *small, f"max_step={per_iter * iters + (0 if algo == 'ppo_algo' else 64 * 32) - 1}",
                    f"logging.jsonl={log}", "info_track_keys=[oob, dist2, TimeLimit.truncated]", "info_track_step=[last, all-episode, last]"])
    out = tb.main(cfg)
    assert out["iters"] == iters
    rows = _jsonl(log)
    assert len(rows) == iters // 2
    for r in rows:
        assert {"oob", "dist2", "TimeLimit.truncated", "train/return"} <= set(r)
    last = rows[-1]
    assert 0 <= last["oob"] <= 1 and 0 < last["TimeLimit.truncated"] <= 1 and last["oob"] + last["TimeLimit.truncated"] <= 1 + 1e-6
    assert last["dist2"] > 0
