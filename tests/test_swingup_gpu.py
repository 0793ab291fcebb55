"""SwingUp on the GPU: the one-launch HIP step against its torch definition (bit-equal), the rollout's n-step rows with real time-limit
truncations against the oracle's assembler, bit-exact resume of a DDPG run on the task, and a training run that improves a policy on a
task where neither the zero action nor a linear law does.  Run with `pytest -m gpu`."""
import os

import pytest
import torch

import task_cases as tc
from support import dev  # noqa: F401

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(autouse=True)
def _keep_sigint():
    """The entry points' `main` installs a Ctrl+C handler (capture_keyboard_interrupt); here they run inside pytest's process."""
    import signal
    old = signal.getsignal(signal.SIGINT)
    yield
    signal.signal(signal.SIGINT, old)


# --------------------------------------------------------------------------- the kernel
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
    for act in tc.task_actions(n, A, 12):
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
@pytest.mark.parametrize("timeout", [True, False])
def test_rollout_nstep_rows_on_swingup(dev, timeout):
    """`PQLActor.explore_env` on SwingUp through `create_task_env` (nstep 3, two calls of T = 8, episode_length 5, 32 envs): the
    emitted n-step rows equal `oracle.pql_ref_cpu.NStepRef` fed the very same transitions, bit for bit.  Every done here is a time
    limit: with handle_timeout such a window carries done = 0 and bootstraps from the window's last next_obs; without it the row is
    terminal and stops at the truncated step.  Episode windows equal a host recomputation."""
    from pql_amd.envs.swingup import SwingUpVecEnv
    tc.check_rollout_nstep_rows(dev, "swingup", SwingUpVecEnv, timeout, terminals=False)


# --------------------------------------------------------------------------- resume
def test_ddpg_resume_on_swingup_is_bit_exact(tmp_path):
    """scripts/train_baselines.py on SwingUp: 6 iterations + checkpoint, then resumed (same process) to 12 == 12 uninterrupted:
    the env's episode state (c, s, w, k, ep) travels in the checkpoint."""
    tc.check_ddpg_resume(tmp_path, "swingup", "train_baselines_su")


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
    lp = tc.load_script("tools/learn_pointmass.py", "learn_pointmass_su")
    r = lp.run("ddpg", "small", 0, LEARN_ITERS, task="swingup")
    print(f"swingup ddpg seed 0, {LEARN_ITERS} iterations: R={r['R']:.3f} R_zero={r['R_zero']:.3f} R_ctrl={r['R_ctrl']:.3f} f={r['f']:.4f} "
          f"wall={r['wall_s']}s")
    assert r["task"] == "swingup" and "R_pd" not in r
    assert r["R_ctrl"] > r["R_zero"]
    assert r["f"] >= F_MIN, r
