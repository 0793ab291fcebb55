"""AgentDDPG / AgentSAC with `algo.critic_fused_backward` off and on from one seed (Toy (8, 2), 64 envs, B = 256, hidden [64, 32],
`algo.critic_fused_forward=True`): the first critic step's gradient `ws["gc"]` against float64 autograd over every parameter, the
switched-off run's error the bar per parameter group, e_new <= 4 e_parent; three more updates stay finite."""
import pytest
import torch

import learner_harness as lh
from lnmlp_grad_cases import GROUPS, grads64, group_errors
from support import dev  # noqa: F401

pytestmark = pytest.mark.gpu
O, A, B = 8, 2, 256


def _run(algo, on, dev):
    """Four update_once -> (x, dq, arena and ws["gc"] of the first critic step, the critic)."""
    from pql_amd.algo.ddpg import AgentDDPG
    from pql_amd.algo.sac import AgentSAC
    from pql_amd.envs.synthetic import create_task_env
    from pql_amd.replay.simple_replay import ReplayBuffer
    from pql_amd.utils.cfg import load_cfg
    cfg = load_cfg([f"algo={algo}_algo", "task.name=Toy", "num_envs=64", f"algo.batch_size={B}", "algo.memory_size=400", "device=cuda:0",
                    "sim_device=cuda:0", "algo.cri_class=DoubleQLayerNorm", "algo.hidden_layers=[64,32]", "algo.critic_fused_forward=True",
                    f"algo.critic_fused_backward={on}"])
    torch.manual_seed(5)
    agent = (AgentDDPG if algo == "ddpg" else AgentSAC)(create_task_env(cfg), cfg)
    critic, rec = agent.critic, {}
    assert critic.fused_backward_on == on
    inner = critic.backward_raw

    def spy(x, dq, grads=None, need_dx=False):   # the critic step's call is the one with `grads`
        first = grads is not None and not rec
        if first:
            rec.update(x=x.clone(), dq=dq.clone(), arena=critic.arena.data.clone())
        out = inner(x, dq, grads=grads, need_dx=need_dx)
        if first:
            rec["gc"] = grads.clone()
        return out

    critic.backward_raw = spy
    memory = ReplayBuffer(400, (O,), A, device=dev)
    memory.add_to_buffer(tuple(t.to(dev) for t in lh._fill(O, A, 300, 810)))
    g = torch.Generator().manual_seed(100)
    for _ in range(4):
        idx = torch.randint(300, (B,), generator=g)
        draws = dict(noise=torch.randn(B, A, generator=g)) if algo == "ddpg" else \
            dict(eps_next=torch.randn(B, A, generator=g), eps_cur=torch.randn(B, A, generator=g))
        agent.update_once(memory, indices=idx, **draws)
    assert bool(torch.isfinite(critic.arena.data).all()) and bool(torch.isfinite(agent.actor.arena.data).all())
    return rec, critic


@pytest.mark.parametrize("algo", ["ddpg", "sac"])
def test_critic_gradient(algo, dev):
    (new, critic), (old, _) = _run(algo, True, dev), _run(algo, False, dev)
    assert all(torch.equal(new[k], old[k]) for k in ("x", "dq", "arena"))   # one seed: the same critic step goes in
    ref = grads64(critic, old["x"], old["dq"], old["arena"])
    e_new, e_parent = group_errors(critic, new["gc"], ref), group_errors(critic, old["gc"], ref)
    for grp in GROUPS:
        print(f"{algo} {grp}: e_new {e_new[grp]:.3e} e_parent {e_parent[grp]:.3e} ratio {e_new[grp] / e_parent[grp]:.2f}")
        assert e_new[grp] <= 4.0 * e_parent[grp], grp
