"""AgentDDPG / AgentSAC with `algo.critic_fused_dx`: the actor step's way back through the frozen critic is the one launch of
pql_amd/csrc/bwd_ln.hip.  Toy (8, 2), 64 envs, B = 256, hidden [64, 32], `algo.critic_fused_forward=True`, the switch off and on from
the same seed.  The critic step does not pass through the new launch, so the critic arenas are bit-equal; what the critic hands to the
actor step is held to float64 autograd on the step's own x_pi, the switched-off run's error the bar: e_new <= 4 e_parent."""
import pytest
import torch

import learner_harness as lh
from lnmlp_dx_cases import dx64
from support import dev  # noqa: F401

pytestmark = pytest.mark.gpu

O, A, B = 8, 2, 256


def _step(algo, on, dev):
    """One update_once -> (the critic's arena, max abs error of ws["dz_a"] (DDPG) / ws["dx_pi"] (SAC) against float64)."""
    from pql_amd.envs.synthetic import create_task_env
    from pql_amd.replay.simple_replay import ReplayBuffer
    from pql_amd.utils.cfg import load_cfg
    cfg = load_cfg([f"algo={algo}_algo", "task.name=Toy", "num_envs=64", f"algo.batch_size={B}", "algo.memory_size=400", "device=cuda:0",
                    "sim_device=cuda:0", "algo.cri_class=DoubleQLayerNorm", "algo.hidden_layers=[64,32]", "algo.critic_fused_forward=True",
                    f"algo.critic_fused_dx={on}"])
    if algo == "ddpg":
        from pql_amd.algo.ddpg import AgentDDPG as Agent
    else:
        from pql_amd.algo.sac import AgentSAC as Agent
    torch.manual_seed(5)
    agent = Agent(create_task_env(cfg), cfg)
    assert agent.critic.fused_dx_on == on
    memory = ReplayBuffer(400, (O,), A, device=dev)
    memory.add_to_buffer(tuple(t.to(dev) for t in lh._fill(O, A, 300, 810)))
    g = torch.Generator().manual_seed(100)
    idx = torch.randint(300, (B,), generator=g)
    draws = dict(noise=torch.randn(B, A, generator=g)) if algo == "ddpg" else \
        dict(eps_next=torch.randn(B, A, generator=g), eps_cur=torch.randn(B, A, generator=g))
    agent.update_once(memory, indices=idx, **draws)
    ws = agent._ws
    # through the UPDATED critic, from the d loss / d Q the actor loss left in ws["dy"]
    ref = dx64(agent.critic, ws["x_pi"], ws["dy"], agent.critic.arena.data.double())
    if algo == "sac":
        return agent.critic.arena.data.clone(), float((ws["dx_pi"][:, :O + A].double() - ref).abs().max())
    a = ws["x_pi"][:, O:O + A].double()   # the actor's tanh output
    return agent.critic.arena.data.clone(), float((ws["dz_a"][0, :, :A].double() - ref[:, O:] * (1.0 - a * a)).abs().max())


@pytest.mark.parametrize("algo", ["ddpg", "sac"])
def test_actor_side_gradient(algo, dev):
    (c_new, e_new), (c_old, e_parent) = _step(algo, True, dev), _step(algo, False, dev)
    print(f"{algo}: e_new {e_new:.3e} e_parent {e_parent:.3e} ratio {e_new / e_parent:.2f}")
    assert torch.equal(c_new, c_old)
    assert e_new <= 4.0 * e_parent
