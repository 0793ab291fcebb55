"""PointMass on the GPU: the one-launch HIP step against its torch definition (bit-equal), the rollout's n-step rows with REAL
time-limit truncations and terminals against the oracle's assembler, bit-exact resume of a DDPG run on the task, and the one thing no
other test in this tree observes: a training run that improves a policy.  Run with `pytest -m gpu`."""
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
def test_pointmass_kernel_equals_torch_definition(dev, n, O, A, off):
    """`pqlk_pointmass_step` vs `_step_torch` on the same device: observations, rewards, dones, truncations and every state tensor
    bit-equal after each of 12 steps with episode_length = 5 (every env is reset at least twice).  O = 6 = 3 A has no zero tail
    and O = 211 is no multiple of 4: both take the scalar store path (6 % 4 != 0 as well); 8 and 88 take the 16-byte one."""
    from pql_amd.envs.pointmass import PointMassVecEnv
    a = PointMassVecEnv(n, O, A, device=dev, seed=1234, episode_length=5, env_offset=off)
    b = PointMassVecEnv(n, O, A, device=dev, seed=1234, episode_length=5, env_offset=off)
    assert torch.equal(a.reset(), b.reset())
    seen = dict(oob=0, truncated=0, running=0)
    for act in tc.task_actions(n, A, 12):
        act = act.to(dev)
        oa, ra, da, ia = a.step(act)                 # the HIP launch
        ob, rb, db, ib = b._step_torch(act)          # the definition
        ta, tb = ia["TimeLimit.truncated"], ib["TimeLimit.truncated"]
        assert oa.dtype == torch.float32 and da.dtype == torch.bool and ta.dtype == torch.bool
        assert torch.equal(oa, ob) and torch.equal(ra, rb) and torch.equal(da, db) and torch.equal(ta, tb)
        for name in ("x", "v", "g", "k", "ep"):
            assert torch.equal(getattr(a, name), getattr(b, name)), name
        assert torch.equal(oa[:, 3 * A:], torch.zeros((n, O - 3 * A), device=dev))
        seen["oob"] += int((da & ~ta).sum())
        seen["truncated"] += int(ta.sum())
        seen["running"] += int((~da).sum())
    assert min(seen.values()) > 0, f"the comparison did not see every kind of transition: {seen}"
    assert int(a.ep.min()) >= 2


# --------------------------------------------------------------------------- rollout integration
@pytest.mark.parametrize("timeout", [True, False])
def test_rollout_nstep_rows_with_real_truncations(dev, timeout):
    """`PQLActor.explore_env` on PointMass (nstep 3, two calls of T = 8, episode_length 5, 32 envs): the emitted n-step rows equal
    `oracle.pql_ref_cpu.NStepRef` fed the very same transitions, bit for bit.  With handle_timeout a window that holds only a time
    limit carries done = 0 and bootstraps from the window's last next_obs (past the reset, as the reference does); without it the
    row is terminal and stops at the truncated step.  Episode windows equal a host recomputation."""
    from pql_amd.envs.pointmass import PointMassVecEnv

    def leave_the_box(inner):
        inner.x[::4, 0], inner.v[::4, 0] = 1.4, 0.9       # leave the box in the first step whatever the action (x' >= 1.4 + 0.25 * 0.52)
        inner.x[1::8, 0], inner.v[1::8, 0] = 1.25, 0.9    # ... and some a step or two later, or not at all: terminals inside the windows

    tc.check_rollout_nstep_rows(dev, "pointmass", PointMassVecEnv, timeout, terminals=True, prepare=leave_the_box)


# --------------------------------------------------------------------------- resume
def test_ddpg_resume_on_pointmass_is_bit_exact(tmp_path):
    """scripts/train_baselines.py on PointMass: 6 iterations + checkpoint, then resumed (same process) to 12 == 12 uninterrupted:
    the env's episode state (x, v, g, k, ep) travels in the checkpoint."""
    tc.check_ddpg_resume(tmp_path, "pointmass", "train_baselines_pm")


# --------------------------------------------------------------------------- it learns
# profiles/pointmass_learning.json (tools/learn_pointmass.py on an MI355X), DDPG at this shape, seeds 0..4, mean f by iteration count:
# 125: 0.862, 250: 0.893, 500: 0.936, 1000: 0.961, 2000: 0.971 -- the plateau is reached at 1000 (doubling again adds 0.01).
# f of the five seeds at 1000 iterations: 0.9653, 0.9661, 0.9571, 0.9688, 0.9469.  The bar is half of the lowest: the yardsticks (zero
# action, PD controller) do not depend on any learner kernel, and the half covers seed-to-seed and box-to-box spread.
LEARN_ITERS = 1000      # rollout iterations (8 critic + 8 actor updates each); about 2.2 s on an MI355X
F_MIN = 0.5 * 0.9469


def test_ddpg_learns_pointmass():
    """DDPG at (8, 2), 64 envs, batch 256, hidden [128, 128], episode_length 64, seed 0: the trained deterministic policy closes at
    least F_MIN of the gap between the zero action and the PD controller, both measured here on 256 evaluation envs."""
    lp = tc.load_script("tools/learn_pointmass.py", "learn_pointmass")
    r = lp.run("ddpg", "small", 0, LEARN_ITERS)
    print(f"pointmass ddpg seed 0, {LEARN_ITERS} iterations: R={r['R']:.3f} R_zero={r['R_zero']:.3f} R_pd={r['R_pd']:.3f} f={r['f']:.4f} "
          f"wall={r['wall_s']}s")
    assert r["R_pd"] > r["R_zero"]
    assert r["f"] >= F_MIN, r
