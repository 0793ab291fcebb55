"""info_track_keys without a GPU: the tasks' info channels as `_step_torch` defines them, `InfoTrackers`' torch form against a deque
model of the reference's `Tracker` written here, the config errors, the C ABI of the new exports and the training state.

`TrackerModel`, `ModelTrackers` and `scripted_steps`, shared with tests/test_info_track_gpu.py, are in tests/task_cases.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from task_cases import ModelTrackers, assert_trackers_equal, pointmass_infos_from_log, scripted_steps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# --------------------------------------------------------------------------- channel definitions
def _pointmass_f64(pre, act, A):
    x, v, g = (t.double() for t in pre)
    a = act.double().clamp(-1, 1)
    vn = 0.8 * v + 0.2 * a
    xn = x + 0.25 * vn
    sq = (xn - g) ** 2
    return {"dist2": (sq.sum(1) / A, sq.sum(1) / A), "oob": ((xn.abs() > 1.5).any(1).double(), None), "edge": (xn.abs().max(1).values - 1.5).abs()}


def _swingup_f64(pre, act, A):
    c, s, w = (t.double() for t in pre)
    a = act.double().clamp(-1, 1)
    wn = (w + 0.05 * (15.0 * s + 6.0 * a)).clamp(-8, 8)
    d = 0.05 * wn
    d2 = d * d
    cd = 1.0 - d2 * (0.5 - d2 * 0.041666668)
    sd = d * (1.0 - d2 * (0.16666667 - d2 * 0.008333334))
    cn, sn = c * cd - s * sd, s * cd + c * sd
    cn = cn * (1.5 - 0.5 * (cn * cn + sn * sn))
    return {"upright": (cn.sum(1) / A, cn.abs().sum(1) / A), "effort": ((a * a).sum(1) / A, (a * a).sum(1) / A)}


@pytest.mark.parametrize("kind", ["pointmass", "swingup"])
def test_info_channels_are_what_the_step_computed(kind):
    """`_step_torch` with info_channels=True, 12 steps at episode_length = 5 (every env is reset at least twice): each channel equals
    a float64 recomputation from the recorded pre-step state and action within 1e-6 relative -- relative to the mean of the
    summands' magnitudes, which is the value itself for the sums of squares and the scale of the rounding errors for `upright`,
    whose terms cancel -- so the values belong to the step just taken and, for a finished env, are taken before its reset; `oob`
    equals done & ~truncated exactly.  Without info_channels the info dict has exactly the key it had."""
    import task_cases as tc
    from pql_amd.envs.synthetic import TASK_ENVS
    n, O, A = 37, 8, 2
    env = TASK_ENVS[kind](n, O, A, device="cpu", seed=1234, episode_length=5, info_channels=True)
    plain = TASK_ENVS[kind](n, O, A, device="cpu", seed=1234, episode_length=5)
    assert env.info_channels and not plain.info_channels and len(env.info_keys) == 2
    f64 = _pointmass_f64 if kind == "pointmass" else _swingup_f64
    assert torch.equal(env.reset(), plain.reset())
    finished = 0
    for act in tc.task_actions(n, A, 12):
        pre = tuple(getattr(env, name).clone() for name in env._STATE)
        obs, rew, done, info = env.step(act)
        obs_p, rew_p, done_p, info_p = plain.step(act)
        assert set(info_p) == {"TimeLimit.truncated"} and set(info) == {"TimeLimit.truncated", *env.info_keys}
        assert torch.equal(obs, obs_p) and torch.equal(rew, rew_p) and torch.equal(done, done_p)
        assert torch.equal(info["TimeLimit.truncated"], info_p["TimeLimit.truncated"])
        want = f64(pre, act, A)
        for key in env.info_keys:
            got = info[key]
            assert got.dtype == torch.float32 and got.shape == (n,)
            exp, scale = want[key]
            if scale is None:   # a flag: exact away from the threshold
                clear = want["edge"] > 1e-5
                assert torch.equal(got.double()[clear], exp[clear]), key
            else:
                assert bool(((got.double() - exp).abs() <= 1e-6 * scale).all()), (key, float(((got.double() - exp).abs() / scale).max()))
        if kind == "pointmass":
            assert torch.equal(info["oob"], (done & ~info["TimeLimit.truncated"]).to(torch.float32))
        else:
            assert bool((info["upright"].abs() <= 1.0 + 1e-6).all()) and bool((info["effort"] <= 1.0).all())
        finished += int(done.sum())
    assert finished >= 2 * n
    assert "info" not in " ".join(env.state_dict()) and set(env.state_dict()) == set(plain.state_dict())


def test_create_task_env_asks_for_channels_only_with_keys():
    from pql_amd.envs.synthetic import create_task_env
    from pql_amd.utils.cfg import load_cfg
    base = ["task=pointmass", "num_envs=4", "sim_device=cpu"]
    assert not create_task_env(load_cfg(base)).info_channels
    assert create_task_env(load_cfg(base + ["info_track_keys=oob", "info_track_step=[last]"])).info_channels
    create_task_env(load_cfg(["task.name=Toy", "num_envs=4", "sim_device=cpu", "info_track_keys=[TimeLimit.truncated]", "info_track_step=[last]"]))


# --------------------------------------------------------------------------- tracker semantics
@pytest.mark.parametrize("window", [7, 100])
def test_info_trackers_equal_the_deque_model(window):
    """N = 37, six scripted steps (none / all / scattered), all four mode spellings, bool and uint8 keys, a key missing on two steps;
    at window 7 the step where everybody finishes and every `all-step` update bring more values than the window holds.  Rings,
    pointers, accumulators and means equal the model after every step."""
    from pql_amd.utils.info_track import InfoTrackers
    n = 37
    keys = ["f0", "f1", "f1", "f2", "b0", "u0", "f3", "b1", "never"]
    steps = ["last", "all-episode", "all", "all-step", "last", "all-episode", "last", "all-step", "last"]
    got = InfoTrackers(keys, steps, n, window, "cpu")
    want = ModelTrackers(keys, steps, n, window)
    seen_none = seen_all = seen_more = False
    for t, (done, info) in enumerate(scripted_steps(n, 4, 2, seed=window, missing=("f3", "b0"))):
        got.update(done, info)
        want.update(done, info)
        assert_trackers_equal(got, want, f"step {t}")
        seen_none |= not bool(done.any())
        seen_all |= bool(done.all())
        seen_more |= int(done.sum()) > window
    assert seen_none and seen_all and seen_more == (window < n)
    assert want.trackers[-1].count == 0 and want.trackers[6].count < want.trackers[0].count   # never present / missing on some steps
    means = got.means()
    assert set(means) == set(keys) and means["f2"] == want.trackers[3].mean() and means["never"] == 0.0
    assert means["f1"] == want.trackers[2].mean()   # a key listed twice: the last entry of that name is the one reported


def test_info_trackers_string_key_and_log():
    from pql_amd.utils.info_track import InfoTrackers
    tr = InfoTrackers("oob", ["last"], 4, 3, "cpu")
    assert tr.keys == ["oob"] and len(tr) == 1
    tr.update(torch.tensor([True, False, True, False]), {"oob": torch.tensor([1.0, 1.0, 0.0, 1.0])})
    assert tr.add_to_log({"train/return": 0.0}) == {"train/return": 0.0, "oob": pytest.approx(1.0 / 3.0)}
    empty = InfoTrackers(None, None, 4, 3, "cpu")
    assert len(empty) == 0 and empty.means() == {}
    empty.update(torch.ones(4, dtype=torch.bool), {"oob": torch.ones(4)})


# --------------------------------------------------------------------------- config validation
def test_info_trackers_refuse_bad_configs():
    from pql_amd.envs.pointmass import PointMassVecEnv
    from pql_amd.utils.info_track import InfoTrackers
    mk = lambda keys, steps, **kw: InfoTrackers(keys, steps, 4, 3, "cpu", **kw)   # noqa: E731
    with pytest.raises(ValueError, match=r"info_track_keys.*\['oob', 'dist2'\].*info_track_step.*\['last'\]"):
        mk(["oob", "dist2"], ["last"])
    with pytest.raises(ValueError, match=r"info_track_step='sometimes'.*'dist2'"):
        mk(["oob", "dist2"], ["last", "sometimes"])
    with pytest.raises(ValueError, match=r"info_track_step=\['last'\].*info_track_keys"):
        mk(None, ["last"])
    with pytest.raises(ValueError, match=r"info_track_keys.*'upright'.*dist2, oob, TimeLimit\.truncated"):
        mk(["upright"], ["last"], offered=PointMassVecEnv.info_keys)
    mk(["oob", "TimeLimit.truncated"], ["last", "all"], offered=PointMassVecEnv.info_keys)
    mk(["anything"], ["all-step"])   # an env that declares nothing: accepted, stays at zero
    with pytest.raises(ValueError, match=r"info_track_keys.*'oob'.*\(4\)"):
        mk(["oob"], ["last"]).update(torch.ones(4, dtype=torch.bool), {"oob": torch.ones(5)})


def test_entry_points_take_the_keys_instead_of_refusing(tmp_path):
    """The evaluator's engine builds (and validates) its trackers where it is built, fresh ones per evaluation; the agents' guards
    are gone from the sources (their constructors need a GPU: tests/test_info_track_gpu.py)."""
    from types import SimpleNamespace
    from pql_amd.utils.cfg import load_cfg
    from pql_amd.utils.evaluator import RolloutEngine
    cfg = load_cfg(["task=pointmass", "task.episode_length=5", "eval_num_envs=6", "device=cpu", "sim_device=cpu",
                    "info_track_keys=[oob, dist2]", "info_track_step=[last, all-episode]"])
    run = SimpleNamespace(dir=str(tmp_path))
    eng = RolloutEngine(cfg, run)
    assert eng.env.info_channels
    policy = lambda obs: torch.ones((obs.shape[0], 2))   # noqa: E731
    job = eng.start(policy, None, None, 0)
    assert job.info_trackers.window_len == 6 and job.info_trackers is not eng.start(policy, None, None, 0).info_trackers
    cfg.info_track_step = ["last", "nope"]
    with pytest.raises(ValueError, match="info_track_step='nope'"):
        RolloutEngine(cfg, run)
    for path in ("pql_amd/algo/pql_actor.py", "pql_amd/algo/ppo.py", "pql_amd/utils/evaluator.py"):
        assert "NotImplementedError(\"info_track_keys" not in open(os.path.join(ROOT, path)).read(), path


def test_evaluation_on_cpu_reports_eval_keys_from_zero(tmp_path):
    """One whole evaluation through the engine's torch path: eval/<key> equals the model fed a host recomputation of the channels
    from the recorded transitions, and a second evaluation starts from zero (the reference carries its trackers over)."""
    from types import SimpleNamespace
    import task_cases as tc
    from pql_amd.envs.synthetic import create_task_env
    from pql_amd.utils.cfg import load_cfg
    from pql_amd.utils.evaluator import RolloutEngine
    n, A, keys, steps = 6, 2, ["oob", "dist2", "TimeLimit.truncated"], ["last", "all-episode", "last"]
    cfg = load_cfg(["task=pointmass", "task.episode_length=5", f"eval_num_envs={n}", "device=cpu", "sim_device=cpu",
                    f"info_track_keys=[{', '.join(keys)}]", f"info_track_step=[{', '.join(steps)}]", "algo.obs_norm=False"])
    rec = {}

    def make_env(c, num_envs=None):
        rec["env"] = tc.RecordingEnv(create_task_env(c, num_envs=num_envs))
        return rec["env"]

    eng = RolloutEngine(cfg, SimpleNamespace(dir=str(tmp_path)), create_task_env_func=make_env)
    policy = lambda obs: torch.ones((obs.shape[0], A))   # noqa: E731
    results = [eng.finish(eng.start(policy, None, None, i)) for i in range(2)]
    env = rec["env"]
    assert len(env.log) == 2 * 5
    for r, result in enumerate(results):
        want = ModelTrackers(keys, steps, n, n)
        for done, info in pointmass_infos_from_log(env.first_obs, env.log[5 * r:5 * r + 5], A):
            want.update(done, info)
        for key, tr in zip(keys, want.trackers):
            assert result[f"eval/{key}"] == float(np.mean(tr.ring().numpy().astype(np.float64))), key
        assert result["eval/dist2"] > 0 and result["eval/oob"] + result["eval/TimeLimit.truncated"] == 1.0
    assert results[0] == results[1]   # same reset, same policy: equal only because no window and no partial sum is carried over


# --------------------------------------------------------------------------- C ABI
def test_new_exports_are_declared_bound_and_check_their_arguments():
    from pql_amd import _lib as L
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pqlk.h")).read(), flags=re.S)
    raw = C.CDLL(os.fspath(L.LIB_FILE))
    for name in ("pqlk_pointmass_step_info", "pqlk_swingup_step_info", "pqlk_rollout_info"):
        assert re.search(rf"\bint {name}\s*\(", hdr) and name in L.PROTOTYPES and hasattr(raw, name), name
    assert L.PROTOTYPES["pqlk_pointmass_step_info"][1] == L.PROTOTYPES["pqlk_pointmass_step"][1][:-1] + [C.c_void_p, C.c_void_p]
    assert L.PROTOTYPES["pqlk_swingup_step_info"][1] == L.PROTOTYPES["pqlk_swingup_step"][1][:-1] + [C.c_void_p, C.c_void_p]
    assert C.sizeof(L.PqlInfoKey) == 40 and L.INFO_MAX_KEYS == int(re.search(r"#define PQLK_INFO_MAX_KEYS (\d+)", hdr).group(1)) == 8
    E_NULL, E_SHAPE, E_UNSUPPORTED = 1, 2, 5
    P = C.c_void_p(0x1000)   # stands in for a device pointer: argument validation never dereferences it
    for name in ("pqlk_pointmass_step_info", "pqlk_swingup_step_info"):
        step = lambda n, O, A, info: getattr(L.lib, name)(n, O, A, 1, 0, 5, P, P, P, P, P, P, P, P, P, P, info, None)  # noqa: E731
        assert step(16, 8, 2, None) == E_NULL
        assert step(0, 8, 2, P) == E_SHAPE and step(16, 5, 2, P) == E_SHAPE and step(16, 8, 0, P) == E_SHAPE
    assert L.lib.pqlk_pointmass_step(16, 8, 2, 1, 0, 5, P, P, P, P, P, P, P, P, P, None, None) == E_NULL   # the plain entry as before

    def keys(n, **bad):
        arr = (L.PqlInfoKey * n)()
        for k in arr:
            k.values = k.acc = k.ring = k.ring_ptr = 0x1000
            k.dtype, k.mode = L.INFO_F32, L.INFO_ALL_EPISODE
        for field, value in bad.items():
            setattr(arr[n - 1], field, value)
        return arr
    info = L.lib.pqlk_rollout_info
    assert info(16, None, 7, 1, keys(1), None) == E_NULL and info(16, P, 7, 1, None, None) == E_NULL
    for field in ("values", "acc", "ring", "ring_ptr"):
        assert info(16, P, 7, 2, keys(2, **{field: None}), None) == E_NULL, field
    assert info(0, P, 7, 1, keys(1), None) == E_SHAPE and info(16, P, 0, 1, keys(1), None) == E_SHAPE
    assert info(16, P, 7, 0, keys(1), None) == E_SHAPE and info(16, P, 7, 9, keys(9), None) == E_SHAPE
    assert info(16, P, 7, 1, keys(1, mode=3), None) == E_UNSUPPORTED and info(16, P, 7, 1, keys(1, dtype=2), None) == E_UNSUPPORTED


# --------------------------------------------------------------------------- training state
def test_info_trackers_training_state_round_trips_and_names_a_mismatch():
    from pql_amd.utils.info_track import InfoTrackers
    n, window = 37, 7
    keys, steps = ["f0", "f1", "b0"], ["last", "all", "all-step"]
    a = InfoTrackers(keys, steps, n, window, "cpu")
    script = scripted_steps(n, 2, 1, seed=3)
    for done, info in script[:4]:
        a.update(done, info)
    st = a.training_state()
    b = InfoTrackers(keys, ["last", "all-episode", "all-step"], n, window, "cpu")   # (`all` and `all-episode` are one mode)
    b.load_training_state(st)
    for done, info in script[4:]:
        a.update(done, info)
        b.update(done, info)
    for ta, tb, xa, xb in zip(a.trackers, b.trackers, a.accs, b.accs):
        assert torch.equal(ta.ring[:window], tb.ring[:window]) and torch.equal(ta.ptr, tb.ptr)
        assert xa is None or torch.equal(xa, xb)
    assert float(a.accs[1].abs().sum()) > 0 and int(a.trackers[0].ptr) != 0
    other = InfoTrackers(["f0", "b0"], ["last", "all-step"], n, window, "cpu")
    with pytest.raises(ValueError, match=r"\['f0', 'f1', 'b0'\].*\['f0', 'b0'\]"):
        other.load_training_state(st)
    with pytest.raises(ValueError, match="info_track_step"):
        InfoTrackers(keys, ["last", "all", "last"], n, window, "cpu").load_training_state(st)
    b.load_training_state(None)   # a checkpoint from before the keys were tracked
    assert all(float(t.ring.abs().sum()) == 0 and int(t.ptr) == 0 for t in b.trackers) and float(b.accs[1].abs().sum()) == 0
