"""AgentDDPG / AgentSAC with `algo.bronet_fused_forward=True`: the critic's forwards are the one launch of pql_amd/csrc/fwd_bro.hip, its
backward the untouched `backward_raw` reading the fused stash.  (8, 2), B = 96, critic_width 64, critic_blocks 1.  The gradients of one
`update_once` are held to float64 autograd of the torch twin (tests/bronet_cases.py) on the tensors the step itself left in its
workspace, under the rule of tests/test_bro_fused_kernels_gpu.py: the key-off run's own error is the bar, e_on <= 4 e_off."""
import pytest
import torch
import torch.nn.functional as F

import agent_harness as ah
import bronet_cases as bc
from support import dev  # noqa: F401

pytestmark = pytest.mark.gpu

O, A, B, W, K = 8, 2, 96, 64, 1
KEY = "algo.bronet_fused_forward"
SHAPE = ["task=pointmass", f"task.obs_dim={O}", f"task.act_dim={A}", "num_envs=16", f"algo.batch_size={B}", "algo.memory_size=1024"]


def _agent(algo, fused):
    """Agent and filled ring from one seed: identical parameters with the key off and on."""
    agent, memory = ah._agent(f"{algo}_algo", "algo.cri_class=DoubleQBroNet", f"algo.critic_width={W}", f"algo.critic_blocks={K}",
                              "algo.hidden_layers=[64,32]", f"{KEY}={fused}", shape=SHAPE)
    assert (agent.critic.fused is not None) == fused and (agent.critic_target.fused is not None) == fused
    return agent, memory


def _twin(q, arena):
    """The float64 torch twin holding the parameters of the flat `arena`, laid out like q's."""
    twin = bc.Twin(O + A, W, K).double().to(arena.device)
    twin.load_state_dict({k: v.double() for k, v in q.named_views(arena)})
    return twin


def _q64(twin, x):
    return torch.stack([qn[:, 0] for qn in twin(x)])


def _errors(algo, fused, dev):
    """One update_once -> (agent, max abs error of the critic's parameter gradient, of the gradient the critic hands to the actor step)
    against float64 autograd.  DDPG: the actor's whole parameter gradient; SAC: d loss / d x_pi."""
    agent, memory = _agent(algo, fused)
    before = {k: getattr(agent, k).arena.data.double().clone() for k in ("critic", "critic_target", "actor")}
    alpha = float(agent.log_alpha.exp()) if algo == "sac" else 0.0
    ah._updates(agent, memory, (0,), B=B, A=A)
    ws, algo_cfg = agent._ws, agent.cfg.algo
    x, xn, xpi = (ws[k][:, :O + A].double() for k in ("x_sa", "xn_sa", "x_pi"))
    with torch.no_grad():
        qt = _q64(_twin(agent.critic_target, before["critic_target"]), xn).min(0).values
    if algo == "sac":
        qt = qt - alpha * ws["logp_next"].double()
    y = ws["rew"].double() + (1.0 - ws["done"].double()) * float(algo_cfg.gamma) ** int(algo_cfg.nstep) * qt
    twin = _twin(agent.critic, before["critic"])
    ((_q64(twin, x) - y) ** 2).mean(1).sum().backward()
    want = dict(twin.named_parameters())
    e_critic = max(float((v.double() - want[k].grad).abs().max()) for k, v in agent.critic.named_views(ws["gc"]))
    now = _twin(agent.critic, agent.critic.arena.data)   # the actor side goes through the UPDATED critic: -mean(min Q(s, a))
    if algo == "sac":
        xpi.requires_grad_()
        (-_q64(now, xpi).min(0).values.mean()).backward()
        return agent, e_critic, float((ws["dx_pi"][:, :O + A].double() - xpi.grad).abs().max())
    al, a64 = agent.actor.layout, before["actor"].requires_grad_()
    h = ws["x_obs"][:, :O].double()
    for l in range(al.n_layers):
        h = F.linear(h, al.weight(a64, 0, l), al.bias(a64, 0, l))
        h = F.elu(h) if l < al.n_layers - 1 else torch.tanh(h)
    (-_q64(now, torch.cat((xpi[:, :O], h), 1)).min(0).values.mean()).backward()
    return agent, e_critic, float((ws["ga"].double() - a64.grad).abs().max())


@pytest.mark.parametrize("algo", ["ddpg", "sac"])
def test_gradients_from_the_fused_stash(algo, dev, tmp_path):
    (on, c_on, a_on), (off, c_off, a_off) = _errors(algo, True, dev), _errors(algo, False, dev)
    print(f"{algo}: critic gradient e_on {c_on:.3e} e_off {c_off:.3e} ratio {c_on / c_off:.2f}; "
          f"actor side e_on {a_on:.3e} e_off {a_off:.3e} ratio {a_on / a_off:.2f}")
    assert c_on <= 4.0 * c_off and a_on <= 4.0 * a_off
    assert set(on.critic_target._ws) == {("q", B)} and "stash" in on.critic._ws[B]   # the target forward wrote no stash
    # the key is no part of a checkpoint: a state saved with it on loads with it off
    torch.save(on.training_state(), tmp_path / "state.pt")
    off.load_training_state(torch.load(tmp_path / "state.pt", weights_only=False))
    a, b = on._state_tensors(), off._state_tensors()
    assert set(a) == set(b) and all(torch.equal(a[k], b[k]) for k in a)
