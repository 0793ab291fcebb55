"""PQL still learns PointMass when the V-learner's targets come from the bf16 forwards (`algo.target_dtype=bfloat16`).  `pytest -m gpu`."""
import importlib.util
import os

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEARN_ITERS = 1000
# profiles/pointmass_learning_bf16.json (tools/learn_pointmass.py --algos pql --override algo.target_dtype=bfloat16 --versus-default,
# seeds 0-4, 1000 iterations), PQL small with bf16 targets: f = 0.9685, 0.9405, 0.9724, 0.9608, 0.9487; the rule of DESIGN section 10 f7 / f8: half of the lowest
F_MIN_BF16 = 0.5 * 0.9405


def test_pql_learns_pointmass_with_bf16_targets():
    """PQL on PointMass small (obs 8, act 2, 64 envs, batch 256, hidden [128, 128], 1000 iterations, seed 0) with
    algo.target_dtype=bfloat16 closes at least F_MIN_BF16 = 0.5 x 0.9405 = 0.470 of the gap between the zero action and the PD controller.
    Source of the value: profiles/pointmass_learning_bf16.json, PQL small, bf16 targets, seeds 0-4: f = 0.9685, 0.9405, 0.9724, 0.9608, 0.9487; half of the lowest
    (the half covers seed-to-seed and box-to-box spread; the yardsticks depend on no learner kernel).  DESIGN section 10 f9."""
    spec = importlib.util.spec_from_file_location("learn_pointmass_bf16", os.path.join(ROOT, "tools", "learn_pointmass.py"))
    lp = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(lp)
    r = lp.run("pql", "small", 0, LEARN_ITERS, extra=("algo.target_dtype=bfloat16",))
    print(f"pointmass pql bf16 targets seed 0, {LEARN_ITERS} iterations: R={r['R']:.3f} R_zero={r['R_zero']:.3f} R_pd={r['R_pd']:.3f} "
          f"f={r['f']:.4f} wall={r['wall_s']}s")
    assert r["R_pd"] > r["R_zero"]
    assert r["f"] >= F_MIN_BF16, r
