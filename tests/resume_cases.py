"""What the save / resume tests share (tests/test_resume_gpu.py and the resume tests of the replay, prioritized-replay and TQC
families): the entry points, the Toy overrides, the child process that runs an entry point's `main` with its own timeout, and the
keys a resumed run must reproduce bit for bit.  Not collected as tests."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PQL = os.path.join(ROOT, "scripts", "train_pql.py")
BASELINES = os.path.join(ROOT, "scripts", "train_baselines.py")
TOY = ["task=Toy", "num_envs=64", "algo.batch_size=256", "algo.memory_size=20000"]
PQL_TOY = TOY + ["algo.num_gpus=1"]
CHILD = """
import importlib.util, json, sys
spec = importlib.util.spec_from_file_location("entry", sys.argv[1])
mod = importlib.util.module_from_spec(spec)
spec.loader.exec_module(mod)
from pql_amd.utils.cfg import load_cfg
out = mod.main(load_cfg(sys.argv[2:]))
sys.stdout.flush()
print("CHILD_RESULT " + json.dumps(out), flush=True)
"""
# what a resumed run must reproduce bit for bit (rollout_iterations is cumulative: the loop re-enters at the saved iter_t)
PQL_KEYS = ("critic_sha", "critic_target_sha", "actor_sha", "replay_sha", "obs_ring_sha", "rms_sha", "global_steps", "critic_updates",
            "actor_updates", "rollout_iterations", "critic_loss", "actor_loss")
BASELINE_KEYS = ("actor_sha", "critic_sha", "replay_sha", "global_steps", "iters", "train/critic_loss", "train/actor_loss", "train/return",
                 "train/episode_length")


def child(script, overrides, cwd, extra_env=None, timeout=300, check=True):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env.update(extra_env or {})
    r = subprocess.run([sys.executable, "-c", CHILD, script, *overrides], env=env, cwd=str(cwd), capture_output=True, text=True, timeout=timeout)
    if not check:
        return r
    assert r.returncode == 0, f"{overrides}\n{r.stderr[-4000:]}"
    lines = [l for l in r.stdout.splitlines() if l.startswith("CHILD_RESULT ")]
    assert len(lines) == 1, r.stdout[-2000:]
    out = json.loads(lines[0][len("CHILD_RESULT "):])
    out["_stderr"] = r.stderr
    return out


def same(a, b, keys):
    diff = {k: (a[k], b[k]) for k in keys if a[k] != b[k]}
    assert not diff, diff
