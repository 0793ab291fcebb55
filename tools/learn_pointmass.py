#!/usr/bin/env python3
"""Learning record on the learnable tasks -- PointMass (pql_amd/envs/pointmass.py), with `--task swingup` SwingUp
(pql_amd/envs/swingup.py), with `--task reacher` Reacher (pql_amd/envs/reacher.py): do the kernels, assembled into a training run,
improve a policy?

Runs the two entry points themselves -- `scripts/train_baselines.py` (DDPG; `--algos sac` / `tqc`: SAC and TQC) and the fixed-ratio loop of `scripts/train_pql.py` -- on
PointMass for a fixed number of rollout iterations, several seeds each, at two shapes:

    small  (obs 8, act 2):   64 envs, batch 256, hidden [128, 128]
    large  (obs 88, act 16): 1024 envs, batch 8192, the default hidden layers [512, 256, 128]

everything else at the defaults (nstep 3, gamma 0.99, tau 0.05, lr 5e-4, mixed exploration noise).  Per run it records the return of
the trained deterministic policy over one full episode on 256 fresh envs (R), the same for the zero action (R_zero) and for the PD
controller a = clamp(4 (g - x) - 4 v, -1, 1) (R_pd), the gap fraction f = (R - R_zero) / (R_pd - R_zero) and the wall time.
`--curve` adds DDPG (`--curve-algo pql`: PQL) at the small shape over a ladder of iteration counts (where does it plateau?).  With `--task swingup` the shapes
are the same, the episode length is 128 and the upper yardstick is the energy controller (`energy_policy`), recorded as R_ctrl.
With `--task reacher` the episode length is 64 and the upper yardstick is the Jacobian-transpose law (`jacobian_policy`), R_ctrl too.

    python tools/learn_pointmass.py --out profiles/pointmass_learning.json
    python tools/learn_pointmass.py --algos ddpg --shapes small --seeds 1 --iters 200      # a quick look
    python tools/learn_pointmass.py --override algo.replay_obs_dtype=float16 --out profiles/pointmass_learning_fp16.json
    python tools/learn_pointmass.py --algos pql --override algo.target_dtype=bfloat16 --versus-default --out profiles/pointmass_learning_bf16.json
    python tools/learn_pointmass.py --algos ddpg --shapes small --override algo.cri_class=DoubleQLayerNorm --versus-default --curve 125,250,500 --out profiles/pointmass_learning_ln.json
    python tools/learn_pointmass.py --task swingup --iters 2000 --curve 500,1000,2000,4000,8000 --out profiles/swingup_learning.json
    python tools/learn_pointmass.py --task swingup --iters 2000 --algos pql --shapes small --override algo.distl=True --out profiles/swingup_learning_distl.json
    python tools/learn_pointmass.py --task swingup --iters 2000 --algos pql --shapes small --override algo.per.enabled=True --override algo.per.refresh=run --versus-default --curve 250,500,1000 --curve-algo pql --out profiles/per_pql_learning.json
    python tools/learn_pointmass.py --task swingup --iters 2000 --algos pql --shapes small --override algo.cri_class=QuantileDoubleQ --versus algo.cri_class=QuantileDoubleQ --sweep algo.qr_drop=0,2,4 --out profiles/tqc_learning_swingup.json
    python tools/learn_pointmass.py --task swingup --iters 2000 --algos tqc --shapes small --versus-algo sac --sweep algo.qr_drop=0,2,5 --out profiles/tqc_sac_learning_swingup.json
    python tools/learn_pointmass.py --task reacher --curve 250,500,1000,2000,4000 --out profiles/reacher_learning.json
    python tools/learn_pointmass.py --task reacher --algos ddpg --shapes small --seeds 1 --iters 500     # a quick look at the coupled task
"""
import argparse
import importlib.util
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

from pql_amd.envs import reacher, swingup  # noqa: E402
from pql_amd.envs.pointmass import episode_return, pd_policy, zero_policy  # noqa: E402
from pql_amd.envs.synthetic import TASK_ENVS  # noqa: E402
from pql_amd.utils.cfg import load_cfg  # noqa: E402

EPISODE_LENGTH = 64
# task -> env class (the one `create_task_env` builds for that `task.kind`), episode length, (lower, upper) yardstick controllers and the
# record's key for the upper one
TASKS = {
    "pointmass": dict(env=TASK_ENVS["pointmass"], episode_length=EPISODE_LENGTH, zero=zero_policy, ctrl=pd_policy, ctrl_key="R_pd"),
    "swingup": dict(env=TASK_ENVS["swingup"], episode_length=128, zero=swingup.zero_policy, ctrl=swingup.energy_policy, ctrl_key="R_ctrl"),
    "reacher": dict(env=TASK_ENVS["reacher"], episode_length=64, zero=reacher.zero_policy, ctrl=reacher.jacobian_policy, ctrl_key="R_ctrl"),
}
EVAL_ENVS = 256
WARM_UP = 32   # algo.warm_up default: random-policy env steps in front of the first iteration
SHAPES = {
    "small": dict(obs_dim=8, act_dim=2, num_envs=64, batch=256, hidden=[128, 128]),
    "large": dict(obs_dim=88, act_dim=16, num_envs=1024, batch=8192, hidden=None),
}
ALGOS = {"ddpg": ("train_baselines.py", ["algo=ddpg_algo"]), "pql": ("train_pql.py", ["algo=pql_algo", "algo.num_gpus=1"]),
         "sac": ("train_baselines.py", ["algo=sac_algo"]), "tqc": ("train_baselines.py", ["algo=tqc_algo"])}
_SCRIPTS = {}


def script(name):
    if name not in _SCRIPTS:
        spec = importlib.util.spec_from_file_location(name[:-3], os.path.join(ROOT, "scripts", name))
        _SCRIPTS[name] = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(_SCRIPTS[name])
    return _SCRIPTS[name]


def overrides(algo, shape, seed, iters, run_dir, extra=(), task="pointmass"):
    sh = SHAPES[shape]
    n = sh["num_envs"]
    ov = [*ALGOS[algo][1], f"task={task}", f"task.obs_dim={sh['obs_dim']}", f"task.act_dim={sh['act_dim']}",
          f"task.episode_length={TASKS[task]['episode_length']}", f"num_envs={n}", f"algo.batch_size={sh['batch']}",
          f"algo.memory_size={(WARM_UP + iters + 8) * n}", f"seed={seed}", f"max_step={(WARM_UP + iters) * n - 1}", f"+logging.dir={run_dir}"]
    if sh["hidden"] is not None:
        ov.append(f"algo.hidden_layers={sh['hidden']}")
    return ov + list(extra)


def yardsticks(shape, seed, device="cuda:0", task="pointmass"):
    """(eval env, R_zero, R_pd or R_ctrl): 256 fresh envs (their seed is not the training env's) and the task's two hand-written
    controllers on them."""
    sh, tk = SHAPES[shape], TASKS[task]
    env = tk["env"](EVAL_ENVS, sh["obs_dim"], sh["act_dim"], device=device, seed=10_000 + seed, episode_length=tk["episode_length"])
    return env, episode_return(env, tk["zero"](env)), episode_return(env, tk["ctrl"](env))


def run(algo, shape, seed, iters, extra=(), task="pointmass"):
    """One training run through the entry point's own `main`; the policy is evaluated by its `on_finish` hook.
    extra: further config overrides, e.g. ("algo.replay_obs_dtype=float16",).  task: a key of TASKS; the upper yardstick's return is
    recorded as R_pd on PointMass and as R_ctrl on SwingUp and Reacher (a PointMass record has no `task` key, as before the tool knew two tasks)."""
    env, r_zero, r_pd = yardsticks(shape, seed, task=task)
    got = {}

    def evaluate(agent, *_learners):   # the baselines (DDPG, SAC, TQC): the agent; PQL: (rollout actor, V-learner, P-learner)
        agent.set_actor(agent.actor)   # the weights were stepped in place: refresh the rollout's packed copy
        got["R"] = episode_return(env, lambda obs: agent.get_actions(obs, sample=False))

    with tempfile.TemporaryDirectory() as run_dir:   # (the PQL loop's evaluator keeps its best model there)
        cfg = load_cfg(overrides(algo, shape, seed, iters, run_dir, extra, task))
        torch.cuda.synchronize()
        t0 = time.time()
        res = script(ALGOS[algo][0]).main(cfg, on_finish=evaluate)
        torch.cuda.synchronize()
        wall = time.time() - t0
    baseline = ALGOS[algo][0] == "train_baselines.py"   # the synchronous loop: update_times updates per iteration
    done_iters = res["iters"] if baseline else res["rollout_iterations"]
    assert done_iters == iters, (done_iters, iters)
    updates = iters * int(cfg.algo.update_times) if baseline else int(res["critic_updates"])
    return dict(**({"task": task} if task != "pointmass" else {}), algo=algo, shape=shape, seed=seed, iters=iters,
                **({"overrides": list(extra)} if extra else {}), critic_updates=updates, R=got["R"], R_zero=r_zero,
                **{TASKS[task]["ctrl_key"]: r_pd}, f=(got["R"] - r_zero) / (r_pd - r_zero), wall_s=round(wall, 2))


def env_step_time(env_cls=TASK_ENVS["pointmass"], num_envs=4096, obs_dim=88, act_dim=16, steps=2000, rounds=3, episode_length=EPISODE_LENGTH):
    """Microseconds per env step of `env_cls`'s one-launch HIP step and of its torch definition on the GPU (host clock around `steps`
    steps that end in a device synchronise; the two forms alternate, the best of `rounds` is kept; one warm-up round)."""
    mk = lambda: env_cls(num_envs, obs_dim, act_dim, device="cuda:0", seed=1, episode_length=episode_length)   # noqa: E731
    hip, ref = mk(), mk()
    act = 2.0 * torch.rand((num_envs, act_dim), device="cuda:0") - 1.0
    best = {"hip": float("inf"), "torch": float("inf")}
    for r in range(rounds + 1):
        for name, step in (("hip", hip.step), ("torch", ref._step_torch)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                step(act)
            torch.cuda.synchronize()
            if r > 0:
                best[name] = min(best[name], (time.perf_counter() - t0) / steps * 1e6)
    return dict(num_envs=num_envs, obs_dim=obs_dim, act_dim=act_dim, steps=steps, hip_us=round(best["hip"], 2), torch_us=round(best["torch"], 2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--task", default="pointmass", choices=sorted(TASKS))
    ap.add_argument("--algos", default="ddpg,pql")
    ap.add_argument("--shapes", default="small,large")
    ap.add_argument("--seeds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=1000, help="rollout iterations per run (8 critic updates each)")
    ap.add_argument("--curve", default=None, help="comma-separated iteration counts: --curve-algo (default DDPG) at the small shape, every seed, at each of them")
    ap.add_argument("--curve-algo", default="ddpg", choices=sorted(ALGOS), help="the algorithm of the --curve runs")
    ap.add_argument("--override", action="append", default=[], help="a further config override for every run (repeatable)")
    ap.add_argument("--versus-default", action="store_true", help="with --override: every run is preceded by the same run WITHOUT the "
                    "overrides (no `overrides` key in its record), so the two variants alternate inside one call")
    ap.add_argument("--versus", action="append", default=[], help="like --versus-default, but the preceding run takes THESE overrides "
                    "(repeatable): a baseline that is itself not the default")
    ap.add_argument("--versus-algo", default=None, choices=sorted(ALGOS), help="every seed's runs are preceded by ONE run of this algorithm "
                    "at the same shape and seed with the --versus overrides only (no --override, no --sweep): another algorithm as the baseline")
    ap.add_argument("--sweep", default=None, help="KEY=v1,v2,...: every run (and the run that precedes it) once per value, KEY=value "
                    "as a further override of the run itself")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sweep = [()] if a.sweep is None else [(f"{a.sweep.split('=', 1)[0]}={v}",) for v in a.sweep.split("=", 1)[1].split(",")]
    assert torch.cuda.is_available(), "learn_pointmass needs a GPU"
    tk = TASKS[a.task]
    out = dict(**({"task": a.task} if a.task != "pointmass" else {}), device=torch.cuda.get_device_name(0), torch=torch.__version__,
               episode_length=tk["episode_length"], eval_envs=EVAL_ENVS, shapes=SHAPES, overrides=list(a.override),
               env_step=env_step_time(tk["env"], episode_length=tk["episode_length"]), runs=[], curve=[])
    print(json.dumps(out["env_step"]), flush=True)

    def record(key, r):
        out[key].append(r)
        print(json.dumps(r), flush=True)
        if a.out:   # rewritten after every run: a run that is cut short still leaves what was measured
            with open(a.out, "w") as f:
                json.dump(out, f, indent=1)

    for algo in a.algos.split(","):
        for shape in a.shapes.split(","):
            for seed in range(a.seeds):
                if a.versus_algo:
                    record("runs", run(a.versus_algo, shape, seed, a.iters, tuple(a.versus), task=a.task))
                for sw in sweep:
                    if (a.versus_default or a.versus) and (a.override or sw):
                        record("runs", run(algo, shape, seed, a.iters, tuple(a.versus), task=a.task))
                    record("runs", run(algo, shape, seed, a.iters, tuple(a.override) + sw, task=a.task))
    for iters in ([int(x) for x in a.curve.split(",")] if a.curve else []):
        for seed in range(a.seeds):
            record("curve", run(a.curve_algo, "small", seed, iters, tuple(a.override), task=a.task))


if __name__ == "__main__":
    main()
