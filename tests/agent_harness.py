"""What the module and agent tests of a critic class share (tests/test_droq_agents_gpu.py, tests/test_bronet_agents_gpu.py): the
critic's probe input and output gradient, an agent with a ring filled by its warm-up rollout, updates with injected indices and
draws, and the agent's state for bit-for-bit comparisons.  The shapes are arguments; seeds, generator call order, data ranges and
the order of the overrides are fixed here.  Not collected as tests."""
import importlib

import numpy as np
import torch

import detdata as dd
from support import T

AGENTS = {"ddpg_algo": ("pql_amd.algo.ddpg", "AgentDDPG"), "sac_algo": ("pql_amd.algo.sac", "AgentSAC"), "droq_algo": ("pql_amd.algo.sac", "AgentSAC")}


def _x(dev, seed=73, *, O, A, B):
    from pql_amd import _lib as L
    from pql_amd.models.mlp import pad_cols
    x = np.concatenate([dd.uniform((B, O), seed, -2, 2), dd.uniform((B, A), seed + 1, -1, 1)], axis=1)
    return pad_cols(T(x).to(dev), L.ld(O + A))


def _dq(dev, *, B):
    dq = torch.zeros((2, B, 32), device=dev)
    dq[:, :, 0] = T(dd.uniform((2, B), 76, -1, 1)).to(dev)
    return dq


def _agent(algo, *extra, seed=3, shape):
    """Agent and a ring filled by the warm-up rollout, all from `seed`; `shape`: the overrides that stand in front of the devices."""
    from pql_amd.envs.synthetic import create_task_env
    from pql_amd.replay.prioritized_replay import PrioritizedReplayBuffer
    from pql_amd.replay.simple_replay import ReplayBuffer
    from pql_amd.utils.cfg import load_cfg
    from pql_amd.utils.common import preprocess_cfg, set_random_seed
    cfg = load_cfg([f"algo={algo}", *shape, "device=cuda:0", "sim_device=cuda:0", "rl_device=cuda:0", f"seed={seed}", *extra])
    set_random_seed(cfg.seed)
    cfg.algo.v_learner_gpu = cfg.algo.p_learner_gpu = 0
    preprocess_cfg(cfg)
    env = create_task_env(cfg)
    mod, cls = AGENTS[algo]
    agent = getattr(importlib.import_module(mod), cls)(env=env, cfg=cfg)
    agent.reset_agent()
    if cfg.algo.per.enabled:
        memory = PrioritizedReplayBuffer(1024, agent.obs_dim, agent.action_dim, device=agent.device, alpha=float(cfg.algo.per.alpha),
                                         eps=float(cfg.algo.per.eps))
    else:
        memory = ReplayBuffer(1024, agent.obs_dim, agent.action_dim, device=agent.device)
    trajectory, _ = agent.explore_env(env, cfg.algo.warm_up, random=True)
    memory.add_to_buffer(trajectory)
    assert memory.cur_capacity >= 256
    return agent, memory


def _updates(agent, memory, which, *, B, A):
    """update_once with injected indices and draws: update s takes the s-th draws, whoever runs it."""
    sac = type(agent).__name__ == "AgentSAC"
    for s in which:
        g = torch.Generator().manual_seed(1000 + s)
        idx = torch.randint(256, (B,), generator=g)
        d1, d2 = torch.randn((B, A), generator=g), torch.randn((B, A), generator=g)
        if sac:
            agent.update_once(memory, indices=idx, eps_next=d1, eps_cur=d2)
        else:
            agent.update_once(memory, indices=idx, noise=0.2 * d1)
    torch.cuda.synchronize()


def _state(agent):
    torch.cuda.synchronize()
    return {k: v.detach().cpu().clone() for k, v in agent._state_tensors().items()}


def _same(a, b):
    assert set(a) == set(b) and {"critic", "critic_target", "copt.m", "copt.v", "aopt.m", "closs", "aloss", "actor"} <= set(a)
    return all(torch.equal(a[k], b[k]) for k in a)
