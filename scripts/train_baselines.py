#!/usr/bin/env python3
"""Single-process baseline loop -- same shape as the reference's scripts/train_baselines.py:39-72.
Off-policy (DDPG, SAC, CrossQ: `algo=ddpg_algo` / `sac_algo` / `crossq_algo`): warm-up rollout -> replay, then per iteration:
rollout, insert, `agent.update_net(memory)`; `algo.per.enabled=True` makes the replay prioritized (a device sum tree beside the ring).
On-policy (PPO: `algo=ppo_algo`): per iteration rollout, `agent.update_net(trajectory)`.
    python scripts/train_baselines.py algo=ddpg_algo task.name=Toy num_envs=64 algo.batch_size=256 algo.memory_size=100000 max_step=20000
    python scripts/train_baselines.py algo=ppo_algo task.name=Toy num_envs=64 max_step=20000
"""
import os
import sys
import time
from itertools import count

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from pql_amd.algo import alg_name_to_path  # noqa: E402
from pql_amd.envs.synthetic import create_task_env  # noqa: E402
from pql_amd.replay.prioritized_replay import PrioritizedReplayBuffer, per_cfg  # noqa: E402
from pql_amd.replay.simple_replay import ReplayBuffer  # noqa: E402
from pql_amd.utils import checkpoint as CK  # noqa: E402
from pql_amd.utils.cfg import load_cfg  # noqa: E402
from pql_amd.utils.common import capture_keyboard_interrupt, load_class_from_path, preprocess_cfg, set_random_seed  # noqa: E402
from pql_amd.utils.logger import MetricLogger  # noqa: E402


def save_checkpoint(opt, cfg, env, agent, memory, global_steps, next_iter, elapsed):
    """Agent + replay + env + process state at a loop boundary, behind one device synchronisation."""
    import torch
    torch.cuda.synchronize(agent.device)
    state = {"structure": CK.structure(cfg, agent.obs_dim[0], agent.action_dim), "iter_t": int(next_iter), "env": env.state_dict(),
             "agent": agent.training_state(), "memory": memory.training_state(), "elapsed": float(elapsed),
             "process": CK.process_state([agent.device])}
    return CK.save(opt["dir"], global_steps, state, {"ring": memory.rows()} if opt["replay"] else None, keep=opt["keep"])


def load_checkpoint(opt, cfg, env, agent, memory):
    import torch
    ckpt, st = CK.load(opt["resume"])
    has_ring = bool(st["rings"])
    CK.check_structure(st["structure"], CK.structure(cfg, agent.obs_dim[0], agent.action_dim), has_ring)
    env.load_state_dict(st["env"])
    agent.load_training_state(st["agent"], nstep=has_ring)
    if has_ring:
        memory.load_training_state(st["memory"])
        CK.load_ring(ckpt, st, "ring", memory.rows(), verify=opt["verify"])
    torch.cuda.synchronize(agent.device)
    CK.load_process_state(st["process"])   # last: building the agent drew from the generators
    return ckpt, st


def main(cfg, on_finish=None):
    """`on_finish(agent)`: called once the loop has stopped, with the trained agent (tools/learn_pointmass.py evaluates it)."""
    CK.refuse(cfg, int(os.environ.get("WORLD_SIZE", "1")))
    opt = CK.options(cfg)
    set_random_seed(cfg.seed)
    capture_keyboard_interrupt()
    if cfg.device == "cuda":
        cfg.device = cfg.sim_device = cfg.rl_device = "cuda:0"
    cfg.algo.v_learner_gpu = cfg.algo.p_learner_gpu = 0
    preprocess_cfg(cfg)
    env = create_task_env(cfg)
    algo_name = cfg.algo.name if "Agent" in cfg.algo.name else "Agent" + cfg.algo.name
    artifact = cfg.get("artifact")
    if artifact is not None and opt["resume"] is not None:
        print("[train_baselines] warning: resume and artifact are both set; resume wins, artifact is ignored", file=sys.stderr)
        artifact = None
    cfg.artifact = None   # (the agent's base class would read it at construction: here the weights are loaded once the agent is built)
    agent = load_class_from_path(algo_name, alg_name_to_path[algo_name])(env=env, cfg=cfg)
    if artifact is not None:   # local warm start, as the reference does after building the agent (train_baselines.py:33-37)
        from pql_amd.algo.learner import load_artifact
        load_artifact(artifact, actor=agent.actor, critic=agent.critic, obs_rms=getattr(agent, "obs_rms", None))
        if getattr(agent, "critic_target", None) is not None:
            agent.critic_target.arena.data.copy_(agent.critic.arena.data)
    logger = MetricLogger(cfg.logging.get("jsonl") if cfg.get("logging") else None)   # (appends: a resumed run continues the file)
    start, global_steps, start_iter, resumed_from = time.time(), 0, 0, None
    agent.reset_agent()
    is_off_policy = cfg.algo.name != "PPO"
    per = None
    if is_off_policy:
        ring = dict(capacity=int(cfg.algo.memory_size), obs_dim=agent.obs_dim, action_dim=agent.action_dim, device=cfg.device,
                    obs_dtype=agent.replay_obs_dtype)
        per = per_cfg(cfg.algo)   # algo.per.enabled=True: priorities on a device sum tree beside the ring
        memory = ReplayBuffer(**ring) if per is None else PrioritizedReplayBuffer(alpha=float(per.alpha), eps=float(per.eps), **ring)
        saved = None
        if opt["resume"] is not None:
            ckpt, saved = load_checkpoint(opt, cfg, env, agent, memory)
            global_steps, start_iter, start = int(saved["global_steps"]), int(saved["iter_t"]), time.time() - float(saved["elapsed"])
            resumed_from = dict(path=ckpt, global_steps=global_steps, actor_sha=CK.sha(agent.actor.arena.data), critic_sha=CK.sha(agent.critic.arena.data))
        if saved is None or not saved["rings"]:
            if saved is not None:
                print("[train_baselines] resume: the checkpoint holds no replay ring -- repeating the warm-up rollout; from here on this "
                      "run is not bit-exact with the uninterrupted one", file=sys.stderr)
            trajectory, steps = agent.explore_env(env, cfg.algo.warm_up, random=True)
            memory.add_to_buffer(trajectory)
            global_steps += steps
    log_info = {}
    ckpt_dir, ckpt_freq = opt["dir"], opt["freq"]
    for iter_t in count(start_iter):
        trajectory, steps = agent.explore_env(env, cfg.algo.horizon_len, random=False)
        global_steps += steps
        if is_off_policy:
            memory.add_to_buffer(trajectory)
            log_info = agent.update_net(memory)
        else:   # on-policy (PPO): no replay, no warm-up; the update consumes this rollout's trajectory
            log_info = agent.update_net(trajectory)
        if iter_t % cfg.algo.log_freq == 0:
            log_info["global_steps"] = global_steps
            agent.add_info_tracker_log(log_info)   # info_track_keys: the windows' means under the bare key names
            logger.log(log_info, global_steps)
        stop = (cfg.max_step is not None and global_steps > cfg.max_step) or (cfg.max_step is None and time.time() - start > cfg.max_time)
        if ckpt_dir is not None and (stop or (ckpt_freq is not None and (iter_t + 1) % ckpt_freq == 0)):
            save_checkpoint(opt, cfg, env, agent, memory, global_steps, iter_t + 1, time.time() - start)
        if stop:
            break
    if on_finish is not None:
        on_finish(agent)
    result = {**log_info, "global_steps": global_steps, "iters": iter_t + 1}
    if is_off_policy:   # fingerprints of what the run ends with, as scripts/train_pql.py returns them
        import torch
        torch.cuda.synchronize(agent.device)
        result.update(actor_sha=CK.sha(agent.actor.arena.data), critic_sha=CK.sha(agent.critic.arena.data),
                      replay_sha=CK.sha_stream(memory.rows()), resumed_from=resumed_from)
        if per is not None:   # the priorities the run ends with
            result.update(per_sha=CK.sha(memory.leaves), per_pmax=float(memory.pmax))
    return result


if __name__ == "__main__":
    print(main(load_cfg(sys.argv[1:])))
