#!/usr/bin/env python3
"""Timing of the one-launch forward of the residual LayerNorm critic (pql_amd/csrc/fwd_bro.hip) against the per-layer forward, and of
a DDPG update with `algo.bronet_fused_forward` on against off, on one MI355X.

ONE call, variants alternating inside every round after a warm-up round (deltas between variants come from the same process and the
same minutes):

  forward   at (obs 88, act 16), B = 8192, (critic_width, critic_blocks) = (512, 2) and (128, 1), on the same input and the same
            arena: the fused launch with stash, the fused launch without, and the per-layer forward (22 / 14 launches and a
            torch.stack); HIP events around `--launches` back-to-back forwards, median and min over the rounds.
  bf16      (`algo.critic_target_dtype=bfloat16`, pql_amd/csrc/fwd_bro_bf16.hip) in the same rounds, on the same input and arena: the
            bf16 no-stash forward, the pack launch alone, and the forward with the pack launch in front of it (what a target forward
            costs per update); compare them with fused_no_stash of the same call.
  update    `AgentDDPG.update_once` at the same sizes with `DoubleQBroNet`: the per-layer forward, `algo.bronet_fused_forward`, and the
            latter with `algo.critic_target_dtype=bfloat16`: host clock around `--updates` updates that end in a device synchronise.

    python tools/bench_bromlp.py --out profiles/bro_bf16_bench.json
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import torch  # noqa: E402

from bench_lnmlp import time_launches, time_updates  # noqa: E402
from pql_amd import _lib as L  # noqa: E402

O, A = 88, 16
SHAPES = {"default": (512, 2), "small": (128, 1)}   # critic_width, critic_blocks


def forward_variants(dev, batch):
    from pql_amd.models.bronet import DoubleQBroNet
    from pql_amd.models.mlp import pad_cols
    out = {}
    for name, (w, k) in SHAPES.items():
        per, fus = (DoubleQBroNet((O,), A, w, k, fused_forward=f).to(dev) for f in (False, True))
        fus.arena.data.copy_(per.arena.data)
        x = pad_cols(torch.randn((batch, O + A), device=dev), L.ld(O + A))
        out[(name, "fused_stash")] = lambda fus=fus, x=x: fus.forward_raw(x)
        out[(name, "fused_no_stash")] = lambda fus=fus, x=x: fus.forward_raw(x, stash=False)
        out[(name, "per_layer")] = lambda per=per, x=x: per.forward_raw(x)
        b16 = DoubleQBroNet((O,), A, w, k, fused_forward=True, target_dtype="bfloat16").to(dev)
        b16.arena.data.copy_(per.arena.data)
        b16.refresh()
        out[(name, "bf16_no_stash")] = lambda b16=b16, x=x: b16.forward_raw(x, stash=False)
        out[(name, "pack_bf16")] = lambda b16=b16: b16.refresh()
        out[(name, "bf16_no_stash_plus_pack")] = lambda b16=b16, x=x: b16.refresh().forward_raw(x, stash=False)
    return out


def make_agent(width, blocks, fused, batch, target_dtype="float32"):
    from pql_amd.algo.ddpg import AgentDDPG
    from pql_amd.envs.synthetic import create_task_env
    from pql_amd.replay.simple_replay import ReplayBuffer
    from pql_amd.utils.cfg import load_cfg
    rows = 4 * batch
    cfg = load_cfg(["algo=ddpg_algo", "task.name=AllegroHand", "num_envs=64", f"algo.batch_size={batch}", f"algo.memory_size={rows}",
                    "device=cuda:0", "sim_device=cuda:0", "algo.cri_class=DoubleQBroNet", f"algo.critic_width={width}",
                    f"algo.critic_blocks={blocks}", f"algo.bronet_fused_forward={fused}", f"algo.critic_target_dtype={target_dtype}"])
    agent = AgentDDPG(create_task_env(cfg), cfg)
    dev = agent.device
    memory = ReplayBuffer(rows, (O,), A, device=dev)
    memory.add_to_buffer((torch.randn((rows, O), device=dev), torch.rand((rows, A), device=dev) * 2 - 1, torch.randn((rows, 1), device=dev) * 0.05,
                          torch.randn((rows, O), device=dev), (torch.rand((rows, 1), device=dev) < 0.1).float()))
    return agent, memory


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--launches", type=int, default=100)
    ap.add_argument("--updates", type=int, default=50)
    ap.add_argument("--batch", type=int, default=8192)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_bromlp needs a GPU"
    torch.manual_seed(0)
    dev = torch.device("cuda:0")
    fv = forward_variants(dev, a.batch)
    agents = {(name, fused, dt): make_agent(w, k, fused, a.batch, dt) for name, (w, k) in SHAPES.items()
              for fused, dt in ((False, "float32"), (True, "float32"), (True, "bfloat16"))}
    ftimes, utimes = {k: [] for k in fv}, {k: [] for k in agents}
    for r in range(a.rounds + 1):     # round 0 warms up
        for k, fn in fv.items():
            t = time_launches(fn, a.launches)
            if r:
                ftimes[k].append(t)
        for k, (agent, memory) in agents.items():
            t = time_updates(agent, memory, a.updates)
            if r:
                utimes[k].append(t)
    res = dict(device=torch.cuda.get_device_name(0), torch=torch.__version__, rounds=a.rounds, launches=a.launches, updates=a.updates,
               obs_dim=O, act_dim=A, batch=a.batch, forward=[], update_once=[])
    for (name, what), ts in ftimes.items():
        w, k = SHAPES[name]
        rec = dict(critic_width=w, critic_blocks=k, what=what, us_median=round(statistics.median(ts), 2), us_min=round(min(ts), 2))
        res["forward"].append(rec)
        print(json.dumps(rec), flush=True)
    for (name, fused, dt), ts in utimes.items():
        w, k = SHAPES[name]
        rec = dict(critic_width=w, critic_blocks=k, bronet_fused_forward=fused, critic_target_dtype=dt, us_median=round(statistics.median(ts), 1), us_min=round(min(ts), 1))
        res["update_once"].append(rec)
        print(json.dumps(rec), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
