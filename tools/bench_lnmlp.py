#!/usr/bin/env python3
"""Timing of the one-launch forward of the LayerNorm critic (pql_amd/csrc/fwd_ln.hip) against the per-layer forward, and of a DDPG
update with `algo.critic_fused_forward` on against off, on one MI355X.

ONE call, variants alternating inside every round (deltas between variants come from the same process and the same minutes):

  forward   at (obs 88, act 16), B = 8192, hidden [512, 512, 256] and [128, 128], on the same input and the same arena: the fused
            launch with stash, the fused launch without, and the per-layer forward (15 / 10 launches and a torch.stack); HIP events
            around `--launches` back-to-back forwards, median and min over the rounds.
  update    `AgentDDPG.update_once` at the same sizes with `DoubleQLayerNorm`, key off and key on: host clock around `--updates`
            updates that end in a device synchronise.
  bf16      (`algo.critic_target_dtype=bfloat16`, pql_amd/csrc/fwd_ln_bf16.hip) in the same rounds: the bf16 no-stash forward and the
            pack launch that follows every Polyak step as two more forward columns -- to be read against `fused_no_stash`, the fp32
            forward they replace -- and the update with the key on as a third update column.

    python tools/bench_lnmlp.py --out profiles/lnmlp_bf16_bench.json

`--droq`: the same protocol for the DroQ critic's one-launch dropout forwards (`algo.droq_fused_forward`, pqlk_lnmlp_drop_forward /
_bf16) at hidden [512, 512, 256], p = 0.01: the dropout launches against the per-layer dropout forward and against the plain fused
launches of the same module on the same buffers (`drop=False`), and one `update_net` of algo=droq_algo (20 updates, each with three
dropout forwards) with the key off, on, and on with a bf16 target.

    python tools/bench_lnmlp.py --droq --out profiles/droq_fused_bench.json

`--dx`: the same protocol for the one-launch input gradient of the frozen critic (`algo.critic_fused_dx`, pqlk_lnmlp_dx,
pql_amd/csrc/bwd_ln.hip) at hidden [512, 512, 256] and [1024]: on ONE stash, the per-layer `backward_raw(grads=None, need_dx=True)` with
the torch add, and the copy (plain form, SAC) or the slice and tanh factor over 16 columns (tanh form, DDPG) that `_critic_dx` does
without the key, against the one launch in both forms at 32 and, where it may, 64 rows per block; and one DDPG `update_once` with
`algo.critic_fused_forward=True` and the key off and on.

    python tools/bench_lnmlp.py --dx --out profiles/lnmlp_dx_bench.json

`--bwd`: the same protocol for the one-launch gradient chain of the critic's own update (`algo.critic_fused_backward`,
pqlk_lnmlp_grad_chain, pql_amd/csrc/bwd_ln.hip) at hidden [512, 512, 256], [128, 128] and [1024], B = 8192 and 32768 in the one call:
on ONE arena and stash, the per-layer `backward_raw(grads)` against the chain call with the weight-gradient GEMMs at 32 and, where it
may, 64 rows per block and at the library's choice, and the chain call alone; and one DDPG `update_once` at B = `--batch` with
`algo.critic_fused_forward=True` and the key off and on.

    python tools/bench_lnmlp.py --bwd --out profiles/lnmlp_bwd_bench.json
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

from pql_amd import _lib as L  # noqa: E402

O, A = 88, 16
HIDDEN = {"default": [512, 512, 256], "small": [128, 128]}
DX_HIDDEN = {"default": [512, 512, 256], "wide": [1024]}
BWD_HIDDEN = {"default": [512, 512, 256], "small": [128, 128], "wide": [1024]}


def forward_variants(dev, batch):
    from pql_amd.models.layernorm import DoubleQLayerNorm
    from pql_amd.models.mlp import pad_cols
    out = {}
    for name, hidden in HIDDEN.items():
        per, fus = (DoubleQLayerNorm((O,), A, hidden, fused_forward=f).to(dev) for f in (False, True))
        fus.arena.data.copy_(per.arena.data)
        x = pad_cols(torch.randn((batch, O + A), device=dev), L.ld(O + A))
        out[(name, "fused_stash")] = lambda fus=fus, x=x: fus.forward_raw(x)
        out[(name, "fused_no_stash")] = lambda fus=fus, x=x: fus.forward_raw(x, stash=False)
        out[(name, "per_layer")] = lambda per=per, x=x: per.forward_raw(x)
        b16 = DoubleQLayerNorm((O,), A, hidden, fused_forward=True, target_dtype="bfloat16").to(dev)
        b16.arena.data.copy_(per.arena.data)
        b16.refresh()
        out[(name, "fused_bf16_no_stash")] = lambda b16=b16, x=x: b16.forward_raw(x, stash=False)
        out[(name, "pack_bf16")] = b16.refresh
    return out


def droq_forward_variants(dev, batch, p=0.01):
    from pql_amd.models.droq import DoubleQDropoutLayerNorm
    from pql_amd.models.mlp import pad_cols
    hidden = HIDDEN["default"]
    per, fus, b16 = (DoubleQDropoutLayerNorm((O,), A, hidden, dropout=p, seed=1, **kw).to(dev)
                     for kw in ({}, dict(fused_forward=True), dict(fused_forward=True, target_dtype="bfloat16")))
    fus.arena.data.copy_(per.arena.data)
    b16.arena.data.copy_(per.arena.data)
    b16.refresh()
    x = pad_cols(torch.randn((batch, O + A), device=dev), L.ld(O + A))
    return {"per_layer_drop": lambda: per.forward_raw(x),
            "drop_fused_stash": lambda: fus.forward_raw(x), "plain_fused_stash": lambda: fus.forward_raw(x, drop=False),
            "drop_fused_no_stash": lambda: fus.forward_raw(x, stash=False), "plain_fused_no_stash": lambda: fus.forward_raw(x, drop=False, stash=False),
            "drop_bf16_no_stash": lambda: b16.forward_raw(x, stash=False), "plain_bf16_no_stash": lambda: b16.forward_raw(x, drop=False, stash=False)}


def dx_variants(dev, batch):
    from pql_amd.models.layernorm import DoubleQLayerNorm
    from pql_amd.models.mlp import pad_cols
    out = {}
    for name, hidden in DX_HIDDEN.items():
        q = DoubleQLayerNorm((O,), A, hidden, fused_forward=True).to(dev)
        x = pad_cols(torch.randn((batch, O + A), device=dev), L.ld(O + A))
        dq = torch.zeros((2, batch, 32), device=dev)
        dq[:, :, 0] = torch.randn((2, batch), device=dev)
        a, dx, dz = torch.tanh(torch.randn((batch, L.ld(A)), device=dev)), torch.zeros_like(x), torch.zeros((batch, L.ld(A)), device=dev)
        q.forward_raw(x)   # the one stash every variant reads

        def per_plain(q=q, x=x, dq=dq, dx=dx):
            dx.copy_(q.backward_raw(x, dq, grads=None, need_dx=True))

        def per_tanh(q=q, x=x, dq=dq, a=a, dz=dz):
            g = q.backward_raw(x, dq, grads=None, need_dx=True)
            dz[:, :A] = g[:, O:O + A] * (1.0 - a[:, :A] * a[:, :A])

        out[(name, "per_layer_plain")], out[(name, "per_layer_tanh")] = per_plain, per_tanh
        for r in (1, 2) if max(hidden) <= 512 else (1,):
            out[(name, f"fused_plain_r{r}")] = lambda q=q, dq=dq, dx=dx, r=r: q.fused_dx(dq, dx, r=r)
            out[(name, f"fused_tanh_r{r}")] = lambda q=q, dq=dq, dz=dz, a=a, r=r: q.fused_dx(dq, dz, O, A, a, r=r)
    return out


def dx_main(a, dev):
    fv = dx_variants(dev, a.batch)
    agents = {(name, on): make_agent(hidden, True, a.batch, fused_dx=on) for name, hidden in DX_HIDDEN.items() for on in (False, True)}
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
               obs_dim=O, act_dim=A, batch=a.batch, dx=[], update_once=[])
    for (name, what), ts in ftimes.items():
        res["dx"].append(dict(hidden=DX_HIDDEN[name], what=what, us_median=round(statistics.median(ts), 2), us_min=round(min(ts), 2)))
    for (name, on), ts in utimes.items():
        res["update_once"].append(dict(hidden=DX_HIDDEN[name], critic_fused_forward=True, critic_fused_dx=on,
                                       us_median=round(statistics.median(ts), 1), us_min=round(min(ts), 1)))
    for rec in (*res["dx"], *res["update_once"]):
        print(json.dumps(rec), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


def bwd_variants(dev, batch):
    from pql_amd.models.layernorm import DoubleQLayerNorm
    from pql_amd.models.mlp import pad_cols
    out = {}
    for name, hidden in BWD_HIDDEN.items():
        q = DoubleQLayerNorm((O,), A, hidden, fused_forward=True, fused_backward=True).to(dev)
        x = pad_cols(torch.randn((batch, O + A), device=dev), L.ld(O + A))
        dq = torch.zeros((2, batch, 32), device=dev)
        dq[:, :, 0] = torch.randn((2, batch), device=dev)
        g = torch.zeros(q.total, device=dev)
        q.forward_raw(x)   # the one stash every variant reads

        def run(r, q=q, x=x, dq=dq, g=g):   # r None: the per-layer path of the same module
            q.fused_backward_on, q.grad_r = r is not None, r or 0
            q.backward_raw(x, dq, grads=g)
            q.fused_backward_on = True

        out[(name, batch, "per_layer")] = lambda run=run: run(None)
        for r in (0, 1, 2) if max(hidden) <= 512 else (0, 1):
            out[(name, batch, f"fused_r{r}")] = lambda run=run, r=r: run(r)
            out[(name, batch, f"chain_alone_r{r}")] = lambda q=q, dq=dq, g=g, r=r: q.fused_grad_chain(dq, g, r)
    return out


def bwd_main(a, dev):
    fv = {k: fn for batch in (8192, 32768) for k, fn in bwd_variants(dev, batch).items()}
    agents = {(name, on): make_agent(hidden, True, a.batch, fused_backward=on) for name, hidden in BWD_HIDDEN.items() for on in (False, True)}
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
               obs_dim=O, act_dim=A, backward=[], update_once=[])
    for (name, batch, what), ts in ftimes.items():
        res["backward"].append(dict(hidden=BWD_HIDDEN[name], batch=batch, what=what, us_median=round(statistics.median(ts), 2),
                                    us_min=round(min(ts), 2)))
    for (name, on), ts in utimes.items():
        res["update_once"].append(dict(hidden=BWD_HIDDEN[name], batch=a.batch, critic_fused_forward=True, critic_fused_backward=on,
                                       us_median=round(statistics.median(ts), 1), us_min=round(min(ts), 1)))
    for rec in (*res["backward"], *res["update_once"]):
        print(json.dumps(rec), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


def make_droq_agent(fused, batch, target_dtype):
    from pql_amd.algo.sac import AgentSAC
    from pql_amd.envs.synthetic import create_task_env
    from pql_amd.replay.simple_replay import ReplayBuffer
    from pql_amd.utils.cfg import load_cfg
    rows = 4 * batch
    cfg = load_cfg(["algo=droq_algo", "task.name=AllegroHand", "num_envs=64", f"algo.batch_size={batch}", f"algo.memory_size={rows}",
                    "device=cuda:0", "sim_device=cuda:0", f"algo.hidden_layers={HIDDEN['default']}", "algo.critic_dropout=0.01",
                    f"algo.droq_fused_forward={fused}", f"algo.critic_target_dtype={target_dtype}"])
    agent = AgentSAC(create_task_env(cfg), cfg)
    dev = agent.device
    memory = ReplayBuffer(rows, (O,), A, device=dev)
    memory.add_to_buffer((torch.randn((rows, O), device=dev), torch.rand((rows, A), device=dev) * 2 - 1, torch.randn((rows, 1), device=dev) * 0.05,
                          torch.randn((rows, O), device=dev), (torch.rand((rows, 1), device=dev) < 0.1).float()))
    return agent, memory


def time_update_net(agent, memory):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    agent.update_net(memory)   # (ends in a host read of the loss rings: a device synchronise)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6


def droq_main(a, dev):
    fv = droq_forward_variants(dev, a.batch)
    agents = {(fused, dt): make_droq_agent(fused, a.batch, dt) for fused, dt in ((False, "float32"), (True, "float32"), (True, "bfloat16"))}
    ftimes, utimes = {k: [] for k in fv}, {k: [] for k in agents}
    for r in range(a.rounds + 1):     # round 0 warms up
        for k, fn in fv.items():
            t = time_launches(fn, a.launches)
            if r:
                ftimes[k].append(t)
        for k, (agent, memory) in agents.items():
            t = time_update_net(agent, memory)
            if r:
                utimes[k].append(t)
    med = {k: statistics.median(ts) for k, ts in ftimes.items()}
    res = dict(device=torch.cuda.get_device_name(0), torch=torch.__version__, rounds=a.rounds, launches=a.launches, obs_dim=O, act_dim=A,
               batch=a.batch, hidden=HIDDEN["default"], dropout=0.01, forward=[], update_net=[],
               drop_over_plain={k: round(med[f"drop_{k}"] / med[f"plain_{k}"], 3) for k in ("fused_stash", "fused_no_stash", "bf16_no_stash")},
               per_layer_over_drop={k: round(med["per_layer_drop"] / med[f"drop_{k}"], 2) for k in ("fused_stash", "fused_no_stash", "bf16_no_stash")})
    for what, ts in ftimes.items():
        res["forward"].append(dict(what=what, us_median=round(statistics.median(ts), 2), us_min=round(min(ts), 2)))
    for (fused, dt), ts in utimes.items():
        res["update_net"].append(dict(droq_fused_forward=fused, critic_target_dtype=dt, update_times=int(agents[(fused, dt)][0].cfg.algo.update_times),
                                      us_median=round(statistics.median(ts), 1), us_min=round(min(ts), 1)))
    for rec in (*res["forward"], *res["update_net"], dict(drop_over_plain=res["drop_over_plain"], per_layer_over_drop=res["per_layer_over_drop"])):
        print(json.dumps(rec), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


def time_launches(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / n * 1e3   # us per call


def make_agent(hidden, fused, batch, target_dtype="float32", fused_dx=False, fused_backward=False):
    from pql_amd.algo.ddpg import AgentDDPG
    from pql_amd.envs.synthetic import create_task_env
    from pql_amd.replay.simple_replay import ReplayBuffer
    from pql_amd.utils.cfg import load_cfg
    rows = 4 * batch
    cfg = load_cfg(["algo=ddpg_algo", "task.name=AllegroHand", "num_envs=64", f"algo.batch_size={batch}", f"algo.memory_size={rows}",
                    "device=cuda:0", "sim_device=cuda:0", "algo.cri_class=DoubleQLayerNorm", f"algo.hidden_layers={hidden}",
                    f"algo.critic_fused_forward={fused}", f"algo.critic_target_dtype={target_dtype}", f"algo.critic_fused_dx={fused_dx}",
                    f"algo.critic_fused_backward={fused_backward}"])
    agent = AgentDDPG(create_task_env(cfg), cfg)
    dev = agent.device
    memory = ReplayBuffer(rows, (O,), A, device=dev)
    memory.add_to_buffer((torch.randn((rows, O), device=dev), torch.rand((rows, A), device=dev) * 2 - 1, torch.randn((rows, 1), device=dev) * 0.05,
                          torch.randn((rows, O), device=dev), (torch.rand((rows, 1), device=dev) < 0.1).float()))
    return agent, memory


def time_updates(agent, memory, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        agent.update_once(memory)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--launches", type=int, default=100)
    ap.add_argument("--updates", type=int, default=50)
    ap.add_argument("--batch", type=int, default=8192)
    ap.add_argument("--out", default=None)
    ap.add_argument("--droq", action="store_true", help="the DroQ critic's one-launch dropout forwards (see the module docstring)")
    ap.add_argument("--dx", action="store_true", help="the one-launch input gradient of the frozen critic (see the module docstring)")
    ap.add_argument("--bwd", action="store_true", help="the one-launch gradient chain of the critic's update (see the module docstring)")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_lnmlp needs a GPU"
    torch.manual_seed(0)
    dev = torch.device("cuda:0")
    if a.droq:
        return droq_main(a, dev)
    if a.dx:
        return dx_main(a, dev)
    if a.bwd:
        return bwd_main(a, dev)
    fv = forward_variants(dev, a.batch)
    agents = {(name, fused, dt): make_agent(hidden, fused, a.batch, dt) for name, hidden in HIDDEN.items()
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
        rec = dict(hidden=HIDDEN[name], what=what, us_median=round(statistics.median(ts), 2), us_min=round(min(ts), 2))
        res["forward"].append(rec)
        print(json.dumps(rec), flush=True)
    for (name, fused, dt), ts in utimes.items():
        rec = dict(hidden=HIDDEN[name], critic_fused_forward=fused, critic_target_dtype=dt, us_median=round(statistics.median(ts), 1), us_min=round(min(ts), 1))
        res["update_once"].append(rec)
        print(json.dumps(rec), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
