#!/usr/bin/env python3
"""Time the PPO baseline (AgentPPO on the HIP kernels) against a plain-torch eager PPO restated from the equations.

    python tools/bench_ppo.py                       # both shapes: default (4096 x 16, 4 epochs) and the AllegroHand preset (16384 x 8, 5 epochs)
    python tools/bench_ppo.py --shape default --iters 3 --out profiles/ppo_bench.json

Per shape: one rollout iteration (horizon_len env steps on the synthetic env, compute_adv included), compute_adv alone,
update_net, µs per minibatch (update_net / minibatches), kernel launches and the longest kernels of one minibatch (torch profiler),
minibatch time per dW batch-split count, achieved TFLOP/s of the minibatch MLP work and its fraction of the fp32-MFMA peak; then the
same update on the eager-torch PPO.
Timing: HIP events around each phase, after warm-up, median over --iters.
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch
import torch.nn as nn
from torch.distributions import Independent, Normal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_FP32_MFMA_TFLOPS = 157.3
SHAPES = {
    "default": dict(num_envs=4096, horizon=16, batch=32768, epochs=4),
    "allegro_preset": dict(num_envs=16384, horizon=8, batch=32768, epochs=5),
}
HIDDEN = (512, 256, 128)
SPLITS = (8, 16, 32, 64)


def mlp_flops(B, dims):
    """fwd + dW + dX of every layer but the first: 2 B sum(in*out) x (3 per layer, 2 for layer 1)."""
    macs = [a * b for a, b in zip(dims[:-1], dims[1:])]
    return 2.0 * B * (3 * sum(macs) - macs[0])


def timed(fn, iters):
    out = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) * 1e3)   # µs
    return statistics.median(out), out


def kernel_times(fn, top=8):
    """(launches, [(kernel, µs)] of the `top` longest kernels summed over one call of fn) from the torch profiler."""
    try:
        from torch.profiler import ProfilerActivity, profile
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        ev = [e for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA and "Memcpy" not in e.name
              and "Memset" not in e.name]
        per = {}
        for e in ev:
            per[e.name] = per.get(e.name, 0.0) + e.device_time
        rows = sorted(per.items(), key=lambda kv: -kv[1])[:top]
        return len(ev), [(n[:60], round(t, 1)) for n, t in rows], round(sum(per.values()), 1)
    except Exception as e:   # profiler unavailable: report it instead of numbers
        return f"n/a ({type(e).__name__})", [], None


class EagerPPO:
    """PPO update in plain torch: nn.Linear/ELU nets, Independent(Normal), clipped surrogate / value loss, clip_grad_norm_, AdamW."""

    def __init__(self, O, A, dev):
        def mlp(out):
            dims = [O, *HIDDEN, out]
            layers = []
            for i, (a, b) in enumerate(zip(dims[:-1], dims[1:])):
                layers.append(nn.Linear(a, b))
                if i < len(dims) - 2:
                    layers.append(nn.ELU())
            return nn.Sequential(*layers).to(dev)
        self.actor, self.critic = mlp(A), mlp(1)
        self.logstd = nn.Parameter(torch.zeros(A, device=dev))
        self.aopt = torch.optim.AdamW(list(self.actor.parameters()) + [self.logstd], 5e-4)
        self.copt = torch.optim.AdamW(self.critic.parameters(), 5e-4)

    def minibatch(self, obs, act, old, adv, ret, val, clip=0.2):
        mean = self.actor(obs)
        dist = Independent(Normal(mean, torch.exp(self.logstd.expand_as(mean))), 1)
        ratio = (dist.log_prob(act) - old).exp()
        adv = (adv - adv.mean()) / (adv.std() + 1e-8)
        al = torch.max(-adv * ratio, -adv * torch.clamp(ratio, 1 - clip, 1 + clip)).mean()
        v = self.critic(obs).view(-1)
        cl = 0.5 * torch.max((v - ret) ** 2, (val + torch.clamp(v - val, -clip, clip) - ret) ** 2).mean()
        for opt, loss in ((self.aopt, al), (self.copt, cl)):
            opt.zero_grad(set_to_none=True)
            loss.backward()
            nn.utils.clip_grad_norm_(opt.param_groups[0]["params"], 0.5)
            opt.step()


def bench_shape(name, sh, iters, overrides=()):
    from pql_amd.algo.ppo import AgentPPO
    from pql_amd.envs.synthetic import create_task_env
    from pql_amd.utils.cfg import load_cfg
    dev = torch.device("cuda:0")
    task = [] if any(o.lstrip("+").startswith(("task=", "task.name=")) for o in overrides) else ["task.name=AllegroHand"]
    cfg = load_cfg(["algo=ppo_algo", *task, f"num_envs={sh['num_envs']}", f"algo.horizon_len={sh['horizon']}",
                    f"algo.batch_size={sh['batch']}", f"algo.update_times={sh['epochs']}", "device=cuda:0", *overrides])
    env = create_task_env(cfg)
    O, A = env.observation_space.shape[0], env.action_space.shape[0]
    agent = AgentPPO(env, cfg)
    agent.reset_agent()
    rows = sh["num_envs"] * sh["horizon"]
    nmb = -(-rows // sh["batch"])
    holder = {}

    def rollout():
        holder["data"], _ = agent.explore_env(env, sh["horizon"])

    def adv():
        agent.compute_adv(agent._roll, agent.obs, agent.dones, gae=True, timeout=agent.timeout_info)

    def update():
        agent.update_net(holder["data"])

    rollout(); update(); torch.cuda.synchronize()   # warm-up: workspaces, code objects
    t_roll, _ = timed(rollout, iters)
    t_adv, _ = timed(adv, iters)
    t_upd, all_upd = timed(update, iters)
    idx = torch.randperm(rows, device=dev)[: sh["batch"]]
    launches, top_kernels, kernel_sum = kernel_times(lambda: agent.update_minibatch(holder["data"], idx, agent.aloss.numel()))
    # batch splits of the dW GEMMs at this minibatch size (default_splits caps at algo.dw_splits = 16, tuned at B = 8192)
    splits_us = {}
    for sp in SPLITS:
        agent.cfg.algo.dw_splits = sp
        agent.update_minibatch(holder["data"], idx, agent.aloss.numel())
        splits_us[sp] = round(timed(lambda: [agent.update_minibatch(holder["data"], idx, agent.aloss.numel()) for _ in range(4)],
                                    iters)[0] / 4, 1)
    agent.cfg.algo.dw_splits = 16
    per_mb = t_upd / (sh["epochs"] * nmb)
    flops = mlp_flops(sh["batch"], [O, *HIDDEN, A]) + mlp_flops(sh["batch"], [O, *HIDDEN, 1])
    tflops = flops / (per_mb * 1e-6) / 1e12

    eager = EagerPPO(O, A, dev)
    d = holder["data"]
    x = (d[0] - agent.obs_rms.mean) / torch.sqrt(agent.obs_rms.var + 1e-4)
    plan = [(s, min(s + sh["batch"], rows)) for s in range(0, rows, sh["batch"])]

    def eager_update():
        for _ in range(sh["epochs"]):
            p = torch.randperm(rows, device=dev)
            for s, e in plan:
                i = p[s:e]
                eager.minibatch(x[i], d[1][i], d[2][i], d[3][i], d[4][i], d[5][i])

    eager_update(); torch.cuda.synchronize()
    t_eager, _ = timed(eager_update, iters)
    return dict(shape=name, num_envs=sh["num_envs"], horizon=sh["horizon"], batch=sh["batch"], epochs=sh["epochs"], minibatches=nmb,
                obs_dim=O, act_dim=A, hidden=list(HIDDEN), iters=iters, rollout_iter_us=round(t_roll, 1), compute_adv_us=round(t_adv, 1),
                update_net_us=round(t_upd, 1), update_net_us_all=[round(v, 1) for v in all_upd], minibatch_us=round(per_mb, 1),
                launches_per_minibatch=launches, minibatch_kernel_us=kernel_sum, minibatch_top_kernels_us=top_kernels,
                minibatch_us_by_dw_splits=splits_us, minibatch_gflop=round(flops / 1e9, 2), achieved_tflops=round(tflops, 2),
                peak_fraction=round(tflops / PEAK_FP32_MFMA_TFLOPS, 3), eager_update_net_us=round(t_eager, 1),
                eager_minibatch_us=round(t_eager / (sh["epochs"] * nmb), 1), speedup_vs_eager=round(t_eager / t_upd, 2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", choices=["all", *SHAPES], default="all")
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--out", default=None, help="also write the result lines to this JSON file")
    ap.add_argument("overrides", nargs="*", help="config overrides, e.g. task=pointmass task.obs_dim=88 task.act_dim=16 "
                    "(default: the synthetic env with AllegroHand's shapes)")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_ppo needs a GPU"
    torch.manual_seed(0)
    np.random.seed(0)
    res = []
    for name, sh in SHAPES.items():
        if a.shape in ("all", name):
            r = bench_shape(name, sh, a.iters, a.overrides)
            print(json.dumps(r), flush=True)
            res.append(r)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(dict(device=torch.cuda.get_device_name(0), torch=torch.__version__, results=res), f, indent=1)


if __name__ == "__main__":
    main()
