"""Reacher on the GPU: the one-launch HIP step and its `_info` form against the torch definition (bit-equal, tip columns and the
three channels included), the rollout's n-step rows against the oracle's assembler, bit-exact resume of a DDPG run on the task, the
info windows of a DDPG run against a host recomputation, and a training run that improves a policy on a task whose action columns
interact.  Run with `pytest -m gpu`."""
import functools
import json
import os

import numpy as np
import pytest
import torch

import task_cases as tc
from support import dev  # noqa: F401
from task_cases import F, ModelTrackers, assert_trackers_equal, rot_np, tip_np

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(autouse=True)
def _keep_sigint():
    """The entry points' `main` installs a Ctrl+C handler (capture_keyboard_interrupt); here they run inside pytest's process."""
    import signal
    old = signal.getsignal(signal.SIGINT)
    yield
    signal.signal(signal.SIGINT, old)


# --------------------------------------------------------------------------- the kernels
@functools.lru_cache(maxsize=None)
def controlled_pose(A):
    """(c, s, w) of 64 arms of A links after 63 steps of `jacobian_policy` on the CPU: most of them rest with the tip at the goal."""
    from pql_amd.envs.reacher import ReacherVecEnv, jacobian_policy
    env = ReacherVecEnv(64, 3 * A + 2, A, device="cpu", seed=3, episode_length=64)
    obs, pol = env.reset(), jacobian_policy(env)
    for _ in range(63):
        obs, _, _, _ = env.step(pol(obs))
    return env.c.clone(), env.s.clone(), env.w.clone()


def prepare(env):
    """The start states the hash does not draw.  Envs 0, 16, .. start at w = 2.9 and envs 8, 24, .. at -2.9, just inside the speed
    limit; 0.9 w + 0.3 a stays below 3 from below 3, so nothing the dynamics reach meets the clamp itself: envs 6, 22, .. start at
    w = 3.9 and envs 14, 30, .. at -3.9, which the first step clamps to +-3 whatever the action.  Envs 1, 5, 9, .. start at a
    pose the Jacobian controller reached, so that `reached` = 1 is seen."""
    env.w[::16] = 2.9
    env.w[8::16] = -2.9
    env.w[6::16] = 3.9
    env.w[14::16] = -3.9
    rows = torch.arange(1, env.num_envs, 4)
    for mine, pose in zip((env.c, env.s, env.w), controlled_pose(env.act_dim)):
        mine[rows.to(env.device)] = pose[torch.arange(len(rows)) % 64].to(env.device)


CASES = [(1, 5, 1, 0),                   # one env, a one-link chain, scalar stores
         (33, 8, 2, 7),                  # a float4 that holds w0, w1, ex, ey
         (64, 12, 3, 0),                 # a float4 that holds w2, ex, ey, 0
         (257, 14, 4, 2 ** 32 - 100),    # O = 3 A + 2 exactly, a one-row second tile, an env id that wraps
         (256, 16, 4, 0),                # exactly one full tile, the tip columns in the last float4
         (257, 88, 16, 0),
         (1024, 211, 20, 1024)]


@pytest.mark.parametrize("n,O,A,off", CASES)
def test_reacher_kernels_equal_torch_definition(dev, n, O, A, off):
    """`pqlk_reacher_step` and `pqlk_reacher_step_info` vs `_step_torch` on the same device: observations (the tip columns included),
    rewards, dones, truncations and every state tensor bit-equal after each of 12 steps with episode_length = 5 (every env is reset at
    least twice), the (3, N) info block bit-equal to the torch channels, and the two entries bit-equal to each other in everything
    else.  With n >= 33 the run meets the speed clamp from both sides, unclamped, truncated and running transitions, and (A >= 2: a
    one-link arm's tip stays on the unit circle, 0.4 from the goal at best) both values of `reached`."""
    from pql_amd.envs.reacher import ReacherVecEnv
    mk = lambda **kw: ReacherVecEnv(n, O, A, device=dev, seed=1234, episode_length=5, env_offset=off, **kw)   # noqa: E731
    a, b, c = mk(), mk(info_channels=True), mk(info_channels=True)
    assert torch.equal(a.reset(), b.reset()) and torch.equal(a.reset(), c.reset())
    for env in (a, b, c):
        prepare(env)
    seen = dict(clamped_hi=0, clamped_lo=0, unclamped=0, truncated=0, running=0, reached=0, missed=0)
    for act in tc.task_actions(n, A, 12):
        act = act.to(dev)
        oa, ra, da, ia = a.step(act)                 # the HIP launch
        ob, rb, db, ib = b._step_torch(act)          # the definition
        oc, rc, dc, ic = c.step(act)                 # the HIP launch with INFO
        ta = ia["TimeLimit.truncated"]
        assert oa.dtype == torch.float32 and da.dtype == torch.bool and ta.dtype == torch.bool
        assert set(ia) == {"TimeLimit.truncated"} and set(ib) == set(ic) == {"TimeLimit.truncated", *a.info_keys}
        for o, r, d, t, env in ((ob, rb, db, ib["TimeLimit.truncated"], b), (oc, rc, dc, ic["TimeLimit.truncated"], c)):
            assert torch.equal(oa[:, :3 * A], o[:, :3 * A]), "state columns"
            assert torch.equal(oa[:, 3 * A:3 * A + 2], o[:, 3 * A:3 * A + 2]), "tip columns"
            assert torch.equal(oa, o) and torch.equal(ra, r) and torch.equal(da, d) and torch.equal(ta, t)
            for name in ("c", "s", "w", "k", "ep"):
                assert torch.equal(getattr(a, name), getattr(env, name)), name
        assert torch.equal(da, ta)
        block = torch.stack([ic[k] for k in a.info_keys])
        assert block.dtype == torch.float32 and block.shape == (3, n) and ic["reached"].is_contiguous()
        assert torch.equal(block, torch.stack([ib[k] for k in a.info_keys])), [k for k in a.info_keys if not torch.equal(ic[k], ib[k])]
        assert torch.equal(oa[:, 3 * A + 2:], torch.zeros((n, O - 3 * A - 2), device=dev))
        assert float(a.w.abs().max()) <= 3.0
        running = (~da).unsqueeze(1)                 # (a reset env's w is a fresh draw in [-0.5, 0.5])
        seen["clamped_hi"] += int(((a.w == 3.0) & running).sum())
        seen["clamped_lo"] += int(((a.w == -3.0) & running).sum())
        seen["unclamped"] += int(((a.w.abs() < 3.0) & running).sum())
        seen["truncated"] += int(ta.sum())
        seen["running"] += int((~da).sum())
        seen["reached"] += int((ic["reached"] == 1.0).sum())
        seen["missed"] += int((ic["reached"] == 0.0).sum())
    assert seen["reached"] + seen["missed"] == 12 * n
    if A < 2:
        assert seen.pop("reached") == 0
    if n < 33:
        for key in ("clamped_hi", "clamped_lo"):
            seen.pop(key)
    assert min(seen.values()) > 0, f"the comparison did not see every kind of transition: {seen}"
    assert int(a.ep.min()) >= 2


# --------------------------------------------------------------------------- rollout integration
@pytest.mark.parametrize("timeout", [True, False])
def test_rollout_nstep_rows_on_reacher(dev, timeout):
    """`PQLActor.explore_env` on Reacher through `create_task_env`: the emitted n-step rows equal `oracle.pql_ref_cpu.NStepRef` fed the
    very same transitions, bit for bit; every done is a time limit (tests/task_cases.py says what that means for either setting)."""
    from pql_amd.envs.reacher import ReacherVecEnv
    tc.check_rollout_nstep_rows(dev, "reacher", ReacherVecEnv, timeout, terminals=False)


# --------------------------------------------------------------------------- resume
def test_ddpg_resume_on_reacher_is_bit_exact(tmp_path):
    """scripts/train_baselines.py on Reacher: 6 iterations + checkpoint, then resumed (same process) to 12 == 12 uninterrupted: the
    env's episode state (c, s, w, k, ep) travels in the checkpoint."""
    tc.check_ddpg_resume(tmp_path, "reacher", "train_baselines_re")


# --------------------------------------------------------------------------- info windows
def reacher_infos_from_log(first_obs, log, A):
    """[(done, info)] of the transitions `task_cases.RecordingEnv` kept: the step is recomputed on the host in numpy float32 from the
    observation row in front of it (w = 4 obs_w, exact), one rounding per written operation; the recomputed reward has to be the
    recorded one bit for bit, so the channels are those of the very step the env took."""
    out, obs = [], first_obs.cpu()
    inv_a = F(1.0) / F(A)
    for act, nobs, rew, done, trunc in log:
        o = obs.numpy()
        c, s, w = o[:, :A], o[:, A:2 * A], F(4.0) * o[:, 2 * A:3 * A]
        a = np.clip(act.numpy().astype(F), F(-1.0), F(1.0))
        wn = np.clip(F(0.9) * w + F(0.3) * a, F(-3.0), F(3.0))
        cn, sn = rot_np(c, s, F(0.05) * wn)
        ex, ey = tip_np(cn.T, sn.T)
        d2 = ex * ex + ey * ey
        w2, eff = wn[:, 0] * wn[:, 0], a[:, 0] * a[:, 0]
        for j in range(1, A):
            w2, eff = w2 + wn[:, j] * wn[:, j], eff + a[:, j] * a[:, j]
        cost = (d2 + F(0.01) * (w2 * inv_a)) + F(0.01) * (eff * inv_a)
        assert cost.dtype == np.float32 and torch.equal(rew, torch.from_numpy(-(F(0.05) * cost)))
        assert torch.equal(done, trunc)
        out.append((done, {"tip_dist2": torch.from_numpy(d2), "reached": torch.from_numpy((d2 < F(0.01)).astype(F)), "TimeLimit.truncated": trunc}))
        obs = nobs
    return out


def test_train_baselines_tracks_reacher_info_keys(tmp_path, monkeypatch):
    """scripts/train_baselines.py, DDPG on Reacher with info_track_keys=[tip_dist2, reached], 32 envs, 12 iterations after the 32
    warm-up steps, episode_length 5: the windows the run ends with equal `ModelTrackers` fed a host recomputation of the two
    channels from the transitions a recording wrapper kept, and the last logged row (iteration 10: 43 env steps) carries that
    model's means."""
    tb = tc.load_script("scripts/train_baselines.py", "train_baselines_re_info")
    from pql_amd.utils.cfg import load_cfg
    N, A, WIN = 32, 2, 20
    keys, steps = ["tip_dist2", "reached"], ["all-episode", "last"]
    rec, kept = {}, {}
    inner_create = tb.create_task_env

    def recording(cfg, *args, **kw):
        rec["env"] = tc.RecordingEnv(inner_create(cfg, *args, **kw))
        return rec["env"]

    monkeypatch.setattr(tb, "create_task_env", recording)
    log = tmp_path / "log.jsonl"
    cfg = load_cfg(["algo=ddpg_algo", "task=reacher", "task.episode_length=5", f"num_envs={N}", "algo.batch_size=64", "algo.memory_size=4000",
                    "algo.hidden_layers=[64, 64]", f"algo.tracker_len={WIN}", f"max_step={(32 + 12) * N - 1}", f"logging.jsonl={log}",
                    f"info_track_keys=[{', '.join(keys)}]", f"info_track_step=[{', '.join(steps)}]"])

    def on_finish(agent):
        torch.cuda.synchronize()
        kept["trackers"] = agent.info_trackers

    out = tb.main(cfg, on_finish=on_finish)
    env = rec["env"]
    assert out["iters"] == 12 and len(env.log) == 32 + 12 and env.env.info_channels
    infos = reacher_infos_from_log(env.first_obs, env.log, A)
    want, at_log = ModelTrackers(keys, steps, N, WIN), None
    for t, (done, info) in enumerate(infos):
        want.update(done, info)
        if t == 32 + 11 - 1:                         # the state the row of iteration 10 was logged from
            at_log = {k: tr.mean() for k, tr in zip(keys, want.trackers)}
    assert_trackers_equal(kept["trackers"], want, "after 44 env steps")
    rows = [json.loads(line) for line in open(log)]
    assert len(rows) == 6 and all(set(keys) <= set(r) for r in rows)
    for key in keys:
        assert rows[-1][key] == pytest.approx(at_log[key], rel=1e-6), key   # (the device sums the window's 20 values in its own order)
    assert 0.0 <= rows[-1]["reached"] <= 1.0 and rows[-1]["tip_dist2"] > 0.0
    assert sum(int(d.sum()) for d, _ in infos) == 8 * N  # 44 steps of 5-step episodes: eight time limits per env


# --------------------------------------------------------------------------- it learns
# profiles/reacher_learning.json (tools/learn_pointmass.py --task reacher --curve 250,500,1000,2000,4000 on an MI355X), DDPG at this shape,
# seeds 0..4, mean f by iteration count: 250: 0.924, 500: 0.930, 1000: 0.971, 2000: 0.970, 4000: 0.972.  The project's rule
# (tests/test_swingup_gpu.py) takes the smallest rung after which doubling adds less than 0.02 to the mean: that is 250 (doubling adds
# 0.006).  The curve is not concave -- from 500 to 1000 it adds another 0.041, then nothing -- so 250 sits on a first shelf, 0.05 below
# the final plateau; the rule is applied as it stands, which also keeps the run under a second.
# f of the five seeds at 250 iterations: 0.9425, 0.8387, 0.9373, 0.9392, 0.9625.  The bar is half of the lowest: the yardsticks (zero
# action, Jacobian-transpose controller) do not depend on any learner kernel, and the half covers seed-to-seed and box-to-box spread.
LEARN_ITERS = 250       # rollout iterations (8 critic + 8 actor updates each); about 0.6 s on an MI355X
F_MIN = 0.5 * 0.8387


def test_ddpg_learns_reacher():
    """DDPG at (8, 2), 64 envs, batch 256, hidden [128, 128], episode_length 64, seed 0, 250 iterations: the trained deterministic
    policy closes at least F_MIN of the gap between the zero action and the Jacobian-transpose controller, both measured here on 256
    evaluation envs.  Source of the bar: `curve` of profiles/reacher_learning.json, f of seeds 0-4 at 250 iterations = 0.9425, 0.8387,
    0.9373, 0.9392, 0.9625; F_MIN = 0.5 x 0.8387 = 0.419."""
    lp =tc.load_script("tools/learn_pointmass.py", "learn_pointmass_re")
    r = lp.run("ddpg", "small", 0, LEARN_ITERS, task="reacher")
    print(f"reacher ddpg seed 0, {LEARN_ITERS} iterations: R={r['R']:.3f} R_zero={r['R_zero']:.3f} R_ctrl={r['R_ctrl']:.3f} f={r['f']:.4f} "
          f"wall={r['wall_s']}s")
    assert r["task"] == "reacher" and "R_pd" not in r
    assert r["R_ctrl"] > r["R_zero"]
    assert r["f"] >= F_MIN, r
