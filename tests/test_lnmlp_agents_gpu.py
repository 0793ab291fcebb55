"""AgentDDPG / AgentSAC with `algo.critic_fused_forward=True`: the critic's forwards are the one launch of pql_amd/csrc/fwd_ln.hip, its
backward the untouched `backward_raw` reading the fused stash.  (8, 2), B = 96, hidden [64, 32].  The gradients of one `update_once`
are held to float64 autograd on the tensors the step itself left in its workspace, under the rule of tests/test_lnmlp_kernels_gpu.py:
the key-off run's own error is the bar, e_new <= 4 e_parent."""
import pytest
import torch
import torch.nn.functional as F

import learner_harness as lh
from support import dev  # noqa: F401

pytestmark = pytest.mark.gpu

O, A, B = 8, 2, 96
KEY = "algo.critic_fused_forward"


def _agent(algo, fused, dev):
    from pql_amd.envs.synthetic import create_task_env
    from pql_amd.replay.simple_replay import ReplayBuffer
    from pql_amd.utils.cfg import load_cfg
    cfg = load_cfg([f"algo={algo}_algo", "task.name=Toy", "num_envs=64", f"algo.batch_size={B}", "algo.memory_size=400", "device=cuda:0",
                    "sim_device=cuda:0", "algo.cri_class=DoubleQLayerNorm", "algo.hidden_layers=[64,32]", f"{KEY}={fused}"])
    if algo == "ddpg":
        from pql_amd.algo.ddpg import AgentDDPG as Agent
    else:
        from pql_amd.algo.sac import AgentSAC as Agent
    torch.manual_seed(5)
    agent = Agent(create_task_env(cfg), cfg)
    assert (agent.critic.fused is not None) == fused and (agent.critic_target.fused is not None) == fused
    memory = ReplayBuffer(400, (O,), A, device=dev)
    memory.add_to_buffer(tuple(t.to(dev) for t in lh._fill(O, A, 300, 810)))
    return agent, memory


def _draws(algo, s):
    g = torch.Generator().manual_seed(100 + s)
    idx = torch.randint(300, (B,), generator=g)
    if algo == "ddpg":
        return dict(indices=idx, noise=torch.randn(B, A, generator=g))
    return dict(indices=idx, eps_next=torch.randn(B, A, generator=g), eps_cur=torch.randn(B, A, generator=g))


def _q64(q, arena, x):
    """min-ready twin Q (2, m) of critic `q` with parameters `arena` (float64, may require grad) on x (m, O + A) in float64."""
    from pql_amd.models.layernorm import LN_EPS
    out, H = [], q.n_layers - 1
    for n in range(2):
        a = x
        for l in range(H):
            z = F.linear(a, q.weight(n, l, arena), q.bias(n, l, arena))
            a = F.elu(F.layer_norm(z, z.shape[1:], q.norm_param(n, l, "gamma", arena), q.norm_param(n, l, "beta", arena), LN_EPS))
        out.append(F.linear(a, q.weight(n, H, arena), q.bias(n, H, arena))[:, 0])
    return torch.stack(out)


def _errors(algo, fused, dev):
    """One update_once -> max abs error of (the critic's parameter gradient, the gradient the critic hands to the actor step) against
    float64 autograd.  DDPG: the actor's whole parameter gradient; SAC: d loss / d x_pi, what the policy head's backward is given."""
    agent, memory = _agent(algo, fused, dev)
    before = {k: getattr(agent, k).arena.data.double().clone() for k in ("critic", "critic_target", "actor")}
    alpha = float(agent.log_alpha.exp()) if algo == "sac" else 0.0
    agent.update_once(memory, **_draws(algo, 0))
    ws, algo_cfg = agent._ws, agent.cfg.algo
    x, xn, xpi = (ws[k][:, :O + A].double() for k in ("x_sa", "xn_sa", "x_pi"))
    # critic: twin MSE against y = r + (1 - d) gamma^n (min Q_t(s', a') - alpha log pi(a'|s'))
    qt = _q64(agent.critic_target, before["critic_target"], xn).min(0).values
    if algo == "sac":
        qt = qt - alpha * ws["logp_next"].double()
    y = ws["rew"].double() + (1.0 - ws["done"].double()) * float(algo_cfg.gamma) ** int(algo_cfg.nstep) * qt
    arena = before["critic"].requires_grad_()
    ((_q64(agent.critic, arena, x) - y) ** 2).mean(1).sum().backward()
    e_critic = float((ws["gc"].double() - arena.grad).abs().max())
    # actor side, through the UPDATED critic: -mean(min Q(s, a))
    now = agent.critic.arena.data.double()
    if algo == "sac":
        xpi.requires_grad_()
        (-_q64(agent.critic, now, xpi).min(0).values.mean()).backward()
        return e_critic, float((ws["dx_pi"][:, :O + A].double() - xpi.grad).abs().max())
    al, a64 = agent.actor.layout, before["actor"].requires_grad_()
    h = ws["x_obs"][:, :O].double()
    for l in range(al.n_layers):
        h = F.linear(h, al.weight(a64, 0, l), al.bias(a64, 0, l))
        h = F.elu(h) if l < al.n_layers - 1 else torch.tanh(h)
    (-_q64(agent.critic, now, torch.cat((xpi[:, :O], h), 1)).min(0).values.mean()).backward()
    return e_critic, float((ws["ga"].double() - a64.grad).abs().max())


@pytest.mark.parametrize("algo", ["ddpg", "sac"])
def test_gradients_from_the_fused_stash(algo, dev):
    (c_new, a_new), (c_old, a_old) = _errors(algo, True, dev), _errors(algo, False, dev)
    print(f"{algo}: critic gradient e_new {c_new:.3e} e_parent {c_old:.3e} ratio {c_new / c_old:.2f}; "
          f"actor side e_new {a_new:.3e} e_parent {a_old:.3e} ratio {a_new / a_old:.2f}")
    assert c_new <= 4.0 * c_old and a_new <= 4.0 * a_old


def test_three_updates_are_reproducible(dev):
    runs = []
    for _ in range(2):
        agent, memory = _agent("ddpg", True, dev)
        for s in range(3):
            agent.update_once(memory, **_draws("ddpg", s))
        runs.append({k: v.clone() for k, v in agent._state_tensors().items()})
    assert set(runs[0]) == set(runs[1]) and all(torch.equal(runs[0][k], runs[1][k]) for k in runs[0])


def test_resume_across_the_switch(dev, tmp_path):
    """A training state saved with the key off loads into an agent with the key on, which goes on from it."""
    from pql_amd.algo.critics import structure_keys
    off, memory = _agent("ddpg", False, dev)
    off.update_once(memory, **_draws("ddpg", 0))
    torch.save(off.training_state(), tmp_path / "state.pt")
    on, _ = _agent("ddpg", True, dev)
    assert structure_keys(on.cfg.algo) == structure_keys(off.cfg.algo)
    on.critic.arena.data.add_(1.0)   # away from the saved state
    on.load_training_state(torch.load(tmp_path / "state.pt", weights_only=False))
    a, b = off._state_tensors(), on._state_tensors()
    assert set(a) == set(b) and all(torch.equal(a[k], b[k]) for k in a)
    for agent in (off, on):
        agent.update_once(memory, **_draws("ddpg", 1))
    torch.testing.assert_close(on.critic.arena.data, off.critic.arena.data, rtol=1e-4, atol=1e-5)
    torch.testing.assert_close(on.actor.arena.data, off.actor.arena.data, rtol=1e-4, atol=1e-5)
