"""`DoubleQDropoutLayerNorm` (pql_amd/models/droq.py) and AgentDDPG / AgentSAC running with it: the module against float64 autograd of
the same net under the model's own masks (tests/droq_cases.py), its ties to `DoubleQLayerNorm`, and the agents' determinism and resume.
Small shapes: obs 11, act 3, hidden [64, 33], batch 37."""
import functools
from copy import deepcopy

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import agent_harness as ah
import detdata as dd
import droq_cases as dc
from agent_harness import _same, _state
from support import T, dev  # noqa: F401

pytestmark = pytest.mark.gpu

O, A, HIDDEN, B = 11, 3, [64, 33], 37
LN, DROQ = "algo.cri_class=DoubleQLayerNorm", "algo.cri_class=DoubleQDropoutLayerNorm"


# =========================================================================== the module
def _critic(dev, p, seed=77):
    from pql_amd.models.droq import DoubleQDropoutLayerNorm
    torch.manual_seed(5)
    q = DoubleQDropoutLayerNorm((O,), A, hidden_layers=HIDDEN, dropout=p, seed=seed).to(dev)
    with torch.no_grad():       # norms away from (1, 0), so that their gradients and both ELU branches are in play
        for n in range(2):
            for l in range(len(HIDDEN)):
                q.norm_param(n, l, "gamma").copy_(T(dd.uniform((HIDDEN[l],), 50 + 2 * n + l, 0.5, 1.5)))
                q.norm_param(n, l, "beta").copy_(T(dd.uniform((HIDDEN[l],), 60 + 2 * n + l, -0.5, 0.5)))
    return q


_x, _dq = functools.partial(ah._x, O=O, A=A, B=B), functools.partial(ah._dq, B=B)


def _float64(q, x, dq, call):
    """Q, dX and the parameter gradients (by state_dict key) of the same net in float64 under the masks of the model's `call`-th
    dropout forward (call None: no dropout)."""
    sd = {k: v.double().cpu().requires_grad_(True) for k, v in q.state_dict().items()}
    xs = x[:, :O + A].double().cpu().requires_grad_(True)
    s = float(dc.scale(q.dropout))
    qs = []
    for n, pre in enumerate(q.key_prefixes):
        h = xs
        for l in range(q.n_layers):
            h = F.linear(h, sd[f"{pre}{3 * l}.weight"], sd[f"{pre}{3 * l}.bias"])
            if l == q.n_layers - 1:
                break
            if call is not None:
                keep = dc.keep_mask(q.seed, q.tag(call, n, l), q.dropout, B, h.shape[1])
                h = h * T(keep.astype(np.float64)) * s
            h = F.elu(F.layer_norm(h, (h.shape[1],), sd[f"{pre}{3 * l + 1}.weight"], sd[f"{pre}{3 * l + 1}.bias"], 1e-5))
        qs.append(h)
    loss = sum((qn[:, 0] * dq[n, :, 0].double().cpu()).sum() for n, qn in enumerate(qs))
    grads = torch.autograd.grad(loss, [xs, *sd.values()])
    return [t.detach().numpy() for t in qs], grads[0].numpy(), {k: g.numpy() for k, g in zip(sd, grads[1:])}


@pytest.mark.parametrize("p", [0.01, 0.5])
def test_module_against_float64_autograd_under_its_own_masks(dev, p):
    """The bars of test_layernorm_critic_known_answer: Q at atol 5e-6, dX and every parameter gradient at rtol 5e-5, atol 1e-5.  The
    second call is compared too: its masks are those of call 1, not of call 0."""
    q, x, dq = _critic(dev, p), _x(dev), _dq(dev)
    for call in (0, 1):
        assert q.drop_calls == call
        out = q.forward_raw(x).clone()
        grads = torch.zeros_like(q.arena.data)
        dx = q.backward_raw(x, dq, grads=grads, need_dx=True).clone()
        qs, dx_ref, g_ref = _float64(q, x, dq, call)
        for n in range(2):
            np.testing.assert_allclose(out[n, :, :1].cpu().numpy(), qs[n], atol=5e-6)
        np.testing.assert_allclose(dx[:, :O + A].cpu().numpy(), dx_ref, rtol=5e-5, atol=1e-5)
        for key, view in q.named_views(grads):
            np.testing.assert_allclose(view.cpu().numpy(), g_ref[key], rtol=5e-5, atol=1e-5, err_msg=key)
        # frozen parameters, the same forward: the same dX bits
        assert torch.equal(q.backward_raw(x, dq, grads=None, need_dx=True), dx)
    assert q.drop_calls == 2


def test_consecutive_calls_and_the_copy_draw_different_masks(dev):
    q, x = _critic(dev, 0.5), _x(dev)
    t = deepcopy(q)
    assert (t.drop_stream, q.drop_stream) == (1, 0) and torch.equal(t.arena.data, q.arena.data)
    first, second = q.forward_raw(x).clone(), q.forward_raw(x).clone()
    assert not torch.equal(first[:, :, 0], second[:, :, 0])                 # call 0 | call 1
    copy_first = t.forward_raw(x).clone()
    assert not torch.equal(copy_first[:, :, 0], first[:, :, 0])             # stream 1 | stream 0, both call 0, the same weights
    t.drop_calls, t.drop_stream = 0, 0
    assert torch.equal(t.forward_raw(x), first)                             # the same (seed, call, stream): the same bits
    assert not torch.equal(first[0, :, 0], first[1, :, 0])
    # the masks are the law's: the first hidden activation is elu(beta) exactly on a row whose units were all dropped -- and in general
    # the kernel's y equals a plain LayerNorm of the dropped z
    q.drop_calls = 0
    q.forward_raw(x)
    from pql_amd import _lib as L
    z = q._ws[B]["z"][(1, 0)][:, :HIDDEN[0]].cpu().numpy()
    u, _ = dc.dropped(z, q.seed, q.tag(0, 1, 0), 0.5)
    zt = torch.zeros((B, L.ld(HIDDEN[0])), device=dev); zt[:, :HIDDEN[0]] = T(u).to(dev)
    y, mean, rstd = torch.zeros_like(zt), torch.zeros(B, device=dev), torch.zeros(B, device=dev)
    L.check(L.lib.pqlk_ln_elu_forward(L.ptr(zt), zt.stride(0), B, HIDDEN[0], L.ptr(q.norm_param(1, 0, "gamma")), L.ptr(q.norm_param(1, 0, "beta")),
                                      1e-5, L.ptr(y), L.ptr(mean), L.ptr(rstd), L.stream(dev)))
    assert torch.equal(y[:, :HIDDEN[0]], q._ws[B]["y"][(1, 0)][:, :HIDDEN[0]])


def test_drop_false_is_the_layernorm_critic_bit_for_bit(dev):
    from pql_amd.models.layernorm import DoubleQLayerNorm
    q, x, dq = _critic(dev, 0.5), _x(dev), _dq(dev)
    ln = DoubleQLayerNorm((O,), A, hidden_layers=HIDDEN).to(dev)
    ln.load_state_dict(q.state_dict())
    want = ln.forward_raw(x)
    g_ln = torch.zeros_like(ln.arena.data)
    dx_ln = ln.backward_raw(x, dq, grads=g_ln, need_dx=True)
    q.forward_raw(x)                                    # a dropout forward first: its stash must not leak into what follows
    got = q.forward_raw(x, drop=False)
    g = torch.zeros_like(q.arena.data)
    dx = q.backward_raw(x, dq, grads=g, need_dx=True)
    assert torch.equal(got, want) and torch.equal(dx, dx_ln) and torch.equal(g, g_ln) and q.drop_calls == 1
    s, a = x[:, :O], x[:, O:O + A]
    q1, q2 = q.get_q1_q2(s, a)                          # the reference surface: no dropout, the counter stands still
    assert torch.equal(q1, want[0, :, :1]) and torch.equal(q2, want[1, :, :1]) and q.drop_calls == 1
    assert torch.equal(q.get_q_min(s, a), torch.min(q1, q2)) and torch.equal(q.get_q1(s, a), q1)
    # p = 0 with dropout on: the same bits through the dropout entries
    q0 = _critic(dev, 0.0)
    q0.load_state_dict(q.state_dict())
    assert torch.equal(q0.forward_raw(x), want) and q0.drop_calls == 1
    g0 = torch.zeros_like(q0.arena.data)
    assert torch.equal(q0.backward_raw(x, dq, grads=g0, need_dx=True), dx_ln) and torch.equal(g0, g_ln)


# =========================================================================== the agents
SHAPE = ["task=pointmass", f"task.obs_dim={O}", f"task.act_dim={A}", "num_envs=16", f"algo.batch_size={B}", "algo.memory_size=1024",
         f"algo.hidden_layers=[{HIDDEN[0]},{HIDDEN[1]}]"]


_agent, _updates = functools.partial(ah._agent, shape=SHAPE), functools.partial(ah._updates, B=B, A=A)


@pytest.mark.parametrize("algo", ["ddpg_algo", "sac_algo"])
def test_agents_tie_to_the_layernorm_critic_and_are_reproducible(algo):
    """Three updates.  critic_dropout = 0: the bits of the same agent on DoubleQLayerNorm (arenas, optimiser state, loss rings).
    0.01: other bits, and the same bits from the same seed twice."""
    ends = {}
    for name, extra in (("ln", (LN,)), ("p0", (DROQ, "algo.critic_dropout=0")), ("p1", (DROQ,)), ("p1_again", (DROQ,))):
        agent, memory = _agent(algo, *extra)
        assert type(agent.critic).__name__ == type(agent.critic_target).__name__ == ("DoubleQLayerNorm" if name == "ln" else "DoubleQDropoutLayerNorm")
        if name != "ln":
            assert (agent.critic.dropout, agent.critic.seed) == (0.0 if name == "p0" else 0.01, 3)
            assert (agent.critic.drop_stream, agent.critic_target.drop_stream) == (0, 1)
        _updates(agent, memory, range(3))
        ends[name] = _state(agent)
        if name != "ln":     # dropout is on in the target forward, the critic-loss forward and the actor-loss forward
            assert (agent.critic.drop_calls, agent.critic_target.drop_calls) == (6, 3)
        assert bool(torch.isfinite(ends[name]["closs"]).all()) and bool(torch.isfinite(ends[name]["critic"]).all())
    assert _same(ends["ln"], ends["p0"])
    assert not torch.equal(ends["ln"]["critic"], ends["p1"]["critic"]) and not torch.equal(ends["ln"]["actor"], ends["p1"]["actor"])
    assert _same(ends["p1"], ends["p1_again"])


def test_droq_algo_with_prioritized_replay_is_reproducible():
    ends = []
    for _ in range(2):
        agent, memory = _agent("droq_algo", "algo.per.enabled=True")
        assert agent.per is not None and agent.cfg.algo.update_times == 20 and agent.critic.dropout == 0.01
        _updates(agent, memory, range(3))
        ends.append((_state(agent), memory.tree.cpu().clone()))
    assert _same(ends[0][0], ends[1][0]) and torch.equal(ends[0][1].view(torch.int32), ends[1][1].view(torch.int32))


@pytest.mark.parametrize("algo", ["ddpg_algo", "droq_algo"])
def test_save_and_resume_continues_bit_for_bit(algo, tmp_path):
    """Training state saved after two updates and loaded into a fresh agent -- built from ANOTHER seed, so the mask seed, the call
    counters and the stream ids must come from the state: two more updates equal four uninterrupted ones bitwise."""
    extra = (DROQ, "algo.critic_dropout=0.1")
    a, memory = _agent(algo, *extra)
    _updates(a, memory, range(4))
    b, _ = _agent(algo, *extra)
    _updates(b, memory, range(2))
    st = b.training_state()
    assert st["drop"] == {"critic": {"seed": 3, "drop_calls": 4, "drop_stream": 0}, "critic_target": {"seed": 3, "drop_calls": 2, "drop_stream": 1}}
    torch.save(st, tmp_path / "state.pt")
    c, _ = _agent(algo, *extra, seed=99)
    assert c.critic.seed == 99 and c.critic.drop_calls == 0
    c.load_training_state(torch.load(tmp_path / "state.pt", weights_only=False))
    assert c.critic.drop_state() == st["drop"]["critic"] and c.critic_target.drop_state() == st["drop"]["critic_target"]
    _updates(c, memory, (2, 3))
    assert _same(_state(a), _state(c))
    assert c.critic.drop_state() == a.critic.drop_state() == {"seed": 3, "drop_calls": 8, "drop_stream": 0}
    assert c.critic_target.drop_state() == a.critic_target.drop_state() == {"seed": 3, "drop_calls": 4, "drop_stream": 1}
