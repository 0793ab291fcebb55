"""AgentSAC (algo=droq_algo) and AgentDDPG on the DroQ critic with `algo.droq_fused_forward=True`, float32 and bfloat16 targets, small shapes."""
import functools

import pytest
import torch

import agent_harness as ah

pytestmark = pytest.mark.gpu

O, A, B = 8, 2, 96
SHAPE = ["task=pointmass", f"task.obs_dim={O}", f"task.act_dim={A}", "num_envs=16", f"algo.batch_size={B}", "algo.memory_size=1024",
         "algo.hidden_layers=[64,32]", "algo.cri_class=DoubleQDropoutLayerNorm", "algo.critic_dropout=0.1"]
_agent, _updates = functools.partial(ah._agent, shape=SHAPE), functools.partial(ah._updates, B=B, A=A)


@pytest.mark.parametrize("tdt", ["float32", "bfloat16"])
@pytest.mark.parametrize("algo", ["droq_algo", "ddpg_algo"])
def test_update_net_and_resume(algo, tdt, tmp_path):
    extra = ("algo.droq_fused_forward=True", f"algo.critic_target_dtype={tdt}")
    (off, _), (a, memory) = _agent(algo), _agent(algo, *extra)
    assert off.critic.fused is None and a.critic.fused is not None and (a.critic_target.packed is not None) == (tdt == "bfloat16")
    for agent in (off, a):
        for _ in range(2):
            log = agent.update_net(memory)
            assert all(torch.isfinite(torch.tensor(log[k])) for k in ("train/critic_loss", "train/actor_loss"))
    assert (a.critic.drop_calls, a.critic_target.drop_calls) == (off.critic.drop_calls, off.critic_target.drop_calls) != (0, 0)   # as with the key off
    # saved and loaded into a fresh agent from ANOTHER seed: the next update gives the bits of the agent that never stopped
    torch.save(a.training_state(), tmp_path / "state.pt")
    c, _ = _agent(algo, *extra, seed=99)
    c.load_training_state(torch.load(tmp_path / "state.pt", weights_only=False))
    _updates(a, memory, (0,))
    _updates(c, memory, (0,))
    assert ah._same(ah._state(a), ah._state(c)) and all(x.drop_state() == y.drop_state() for x, y in ((a.critic, c.critic), (a.critic_target, c.critic_target)))
