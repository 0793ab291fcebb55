"""`DoubleQBroNet` (pql_amd/models/bronet.py) and AgentDDPG / AgentSAC running with it: the module against float64 autograd of the
torch twin (tests/bronet_cases.py), the K = 0 tie to `DoubleQLayerNorm`, the target's own workspace, and the agents' ties,
determinism and resume.  Small shapes: obs 8, act 2, batch 37, widths 64 (16-byte rows) and 130 (ragged), K = 2."""
import functools
from copy import deepcopy

import numpy as np
import pytest
import torch

import agent_harness as ah
import bronet_cases as bc
import detdata as dd
import task_cases as tc
from agent_harness import _same, _state
from support import T, dev  # noqa: F401

pytestmark = pytest.mark.gpu

O, A, B, K = 8, 2, 37, 2
WIDTHS = [64, 130]
LN, BRO = "algo.cri_class=DoubleQLayerNorm", "algo.cri_class=DoubleQBroNet"


# =========================================================================== the module
def _critic(dev, W, blocks=K, seed=43):
    from pql_amd.models.bronet import DoubleQBroNet
    q = DoubleQBroNet((O,), A, width=W, blocks=blocks).to(dev)
    q.load_state_dict(bc.twin_state(O + A, W, blocks, seed))     # norms away from (1, 0): their gradients and both ELU branches in play
    return q


_x, _dq = functools.partial(ah._x, O=O, A=A, B=B), functools.partial(ah._dq, B=B)


def _float64(q, x, dq):
    """Q, dX and the parameter gradients (by state_dict key) of the torch twin holding q's parameters, in float64."""
    twin = bc.Twin(O + A, q.width, q.blocks).double()
    twin.load_state_dict({k: v.double().cpu() for k, v in q.state_dict().items()}, strict=True)
    xs = x[:, :O + A].double().cpu().requires_grad_(True)
    qs = twin(xs)
    loss = sum((qn[:, 0] * dq[n, :, 0].double().cpu()).sum() for n, qn in enumerate(qs))
    names, params = zip(*twin.named_parameters())
    grads = torch.autograd.grad(loss, [xs, *params])
    return [t.detach().numpy() for t in qs], grads[0].numpy(), {k: g.numpy() for k, g in zip(names, grads[1:])}


@pytest.mark.parametrize("W", WIDTHS)
def test_module_against_the_float64_twin(dev, W):
    """The bars of test_layernorm_critic_known_answer: Q at atol 5e-6, dX and every parameter gradient at rtol 5e-5, atol 1e-5 -- here
    element by element, and on the fingerprint [sum, l2, probes] of detdata.summarize as there.  As there, the plain sum of a pre-norm
    Linear's gradient has an allowance: LayerNorm's backward gives sum_j dz_rj = 0 in every row, so the sum over ALL entries of dW
    (= sum_r sum_j dz_rj x_ri) and of db of every Linear in front of a norm (all but `out`) is zero in exact arithmetic, the
    reference's own value is rounding noise, and it is held to the absolute bar plus 2e-6 of the tensor's l2 norm."""
    q, x, dq = _critic(dev, W), _x(dev), _dq(dev)
    out = q.forward_raw(x)
    assert out.shape == (2, B, 32)
    qs, dx_ref, g_ref = _float64(q, x, dq)
    for n in range(2):
        np.testing.assert_allclose(out[n, :, :1].cpu().numpy(), qs[n], atol=5e-6)
    q1, q2 = q.get_q1_q2(x[:, :O], x[:, O:O + A])
    assert torch.equal(q1, out[0, :, :1]) and torch.equal(q2, out[1, :, :1]) and not torch.equal(q1, q2)
    assert torch.equal(q.get_q_min(x[:, :O], x[:, O:O + A]), torch.min(q1, q2)) and torch.equal(q.get_q1(x[:, :O], x[:, O:O + A]), q1)
    q.eval()                                                                    # no train / eval difference
    assert torch.equal(q.get_q1(x[:, :O], x[:, O:O + A]), q1)
    q.forward_raw(x)
    grads = torch.zeros_like(q.arena.data)
    dx = q.backward_raw(x, dq, grads=grads, need_dx=True).clone()
    np.testing.assert_allclose(dx[:, :O + A].cpu().numpy(), dx_ref, rtol=5e-5, atol=1e-5)
    assert set(k for k, _ in q.named_views()) == set(g_ref)
    for key, view in q.named_views(grads):
        got = view.cpu().numpy()
        np.testing.assert_allclose(got, g_ref[key], rtol=5e-5, atol=1e-5, err_msg=key)
        s_got, s_want = dd.summarize(got), dd.summarize(g_ref[key])
        np.testing.assert_allclose(s_got[1:], s_want[1:], rtol=5e-5, atol=1e-5, err_msg=key)
        cancels = ".out." not in key and re_is_linear(key)
        np.testing.assert_allclose(s_got[0], s_want[0], rtol=5e-5, atol=1e-5 + (2e-6 * float(s_want[1]) if cancels else 0.0), err_msg=key + " (sum)")
    # pad entries of the gradient and of the arena are zero: whatever is not a view of a parameter
    mask = torch.ones_like(grads, dtype=torch.bool)
    idx = torch.arange(grads.numel(), device=dev)
    for _, view in q.named_views(idx.to(torch.float32)):
        mask[view.reshape(-1).long()] = False
    assert int(mask.sum()) > 0 and bool((grads[mask] == 0).all()) and bool((q.arena.data[mask] == 0).all())
    # frozen parameters: the same dX bits, nothing else needed
    q.forward_raw(x)
    assert torch.equal(q.backward_raw(x, dq, grads=None, need_dx=True), dx)
    # and the backward can be repeated on the same forward: the running skip gradient starts afresh
    again = torch.zeros_like(grads)
    assert torch.equal(q.backward_raw(x, dq, grads=again, need_dx=True), dx) and torch.equal(again, grads)


def re_is_linear(key):
    """Whether a twin key names a Linear (stem.0, blocks.k.0, blocks.k.3, out), not a LayerNorm (stem.1, blocks.k.1, blocks.k.4)."""
    return key.split(".")[-2] in ("0", "3", "out")


@pytest.mark.parametrize("W", WIDTHS)
def test_zero_blocks_is_the_layernorm_critic_bit_for_bit(dev, W):
    from pql_amd.models.layernorm import DoubleQLayerNorm
    q, x, dq = _critic(dev, W, blocks=0), _x(dev), _dq(dev)
    ln = DoubleQLayerNorm((O,), A, hidden_layers=[W]).to(dev)
    assert ln.arena.numel() == q.arena.numel() and ln.off == q.off
    ln.arena.data.copy_(q.arena.data)                   # the same parameters (the keys differ, the layout does not)
    for (ka, va), (kb, vb) in zip(q.named_views(), ln.named_views()):
        assert torch.equal(va, vb), (ka, kb)
    want = ln.forward_raw(x)
    g_ln = torch.zeros_like(ln.arena.data)
    dx_ln = ln.backward_raw(x, dq, grads=g_ln, need_dx=True)
    got = q.forward_raw(x)
    g = torch.zeros_like(q.arena.data)
    dx = q.backward_raw(x, dq, grads=g, need_dx=True)
    assert torch.equal(got, want) and torch.equal(dx, dx_ln) and torch.equal(g, g_ln)
    assert "skip" not in q._ws[B]                       # nothing of the residual path exists
    for (ka, va), (kb, vb) in zip(q.named_views(g), ln.named_views(g_ln)):
        assert torch.equal(va, vb), (ka, kb)


def test_target_forward_does_not_disturb_the_stash(dev):
    """deepcopy gives the target its own workspace: a target forward between the online forward and its backward leaves the gradient's
    bits alone."""
    q = _critic(dev, 130)
    tgt = deepcopy(q)
    x, x2 = _x(dev), _x(dev).flip(0).contiguous()
    dq = _dq(dev)
    outs = []
    for between in (False, True):
        mine = q.forward_raw(x).clone()
        if between:
            assert not torch.equal(tgt.forward_raw(x2), mine)
        grads = torch.zeros_like(q.arena.data)
        dx = q.backward_raw(x, dq, grads=grads, need_dx=True)
        outs.append((grads, dx.clone()))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    assert set(tgt._ws) == {B} and tgt._ws[B] is not q._ws[B] and tgt._ws[B]["skip"] is not q._ws[B]["skip"]


# =========================================================================== the agents
SHAPE = ["task=pointmass", f"task.obs_dim={O}", f"task.act_dim={A}", "num_envs=16", f"algo.batch_size={B}", "algo.memory_size=1024"]


_agent, _updates = functools.partial(ah._agent, shape=SHAPE), functools.partial(ah._updates, B=B, A=A)


@pytest.mark.parametrize("W", WIDTHS)
@pytest.mark.parametrize("algo", ["ddpg_algo", "sac_algo"])
def test_agents_tie_to_the_layernorm_critic_and_are_reproducible(algo, W):
    """Three updates.  critic_blocks = 0: the bits of the same agent on DoubleQLayerNorm with hidden_layers [W] (arenas, optimiser
    state, loss rings; the actor has hidden_layers [W] in both).  K = 2: other bits, and the same bits from the same seed twice."""
    hidden, width = f"algo.hidden_layers=[{W}]", f"algo.critic_width={W}"
    ends = {}
    for name, extra in (("ln", (LN,)), ("k0", (BRO, width, "algo.critic_blocks=0")), ("k2", (BRO, width, f"algo.critic_blocks={K}")),
                        ("k2_again", (BRO, width, f"algo.critic_blocks={K}"))):
        agent, memory = _agent(algo, hidden, *extra)
        assert type(agent.critic).__name__ == type(agent.critic_target).__name__ == ("DoubleQLayerNorm" if name == "ln" else "DoubleQBroNet")
        if name != "ln":
            assert (agent.critic.width, agent.critic.blocks) == (W, 0 if name == "k0" else K)
            assert agent.critic_target._ws is not agent.critic._ws
        _updates(agent, memory, range(3))
        ends[name] = _state(agent)
        assert bool(torch.isfinite(ends[name]["closs"]).all()) and bool(torch.isfinite(ends[name]["critic"]).all())
    assert _same(ends["ln"], ends["k0"])
    assert ends["k2"]["critic"].numel() > ends["ln"]["critic"].numel() and not torch.equal(ends["ln"]["actor"], ends["k2"]["actor"])
    assert _same(ends["k2"], ends["k2_again"])


@pytest.mark.parametrize("algo", ["ddpg_algo", "sac_algo"])
def test_prioritized_replay_is_reproducible(algo):
    ends = []
    for _ in range(2):
        agent, memory = _agent(algo, BRO, "algo.critic_width=130", f"algo.critic_blocks={K}", "algo.hidden_layers=[64]", "algo.per.enabled=True")
        assert agent.per is not None and type(agent.critic).__name__ == "DoubleQBroNet"
        _updates(agent, memory, range(3))
        ends.append((_state(agent), memory.tree.cpu().clone()))
    assert _same(ends[0][0], ends[1][0]) and torch.equal(ends[0][1].view(torch.int32), ends[1][1].view(torch.int32))


@pytest.mark.parametrize("algo", ["ddpg_algo", "sac_algo"])
def test_save_and_resume_continues_bit_for_bit(algo, tmp_path):
    """Training state saved after one update and loaded into an agent built from ANOTHER seed: two more updates equal three
    uninterrupted ones bitwise (arenas of actor, critic and targets, optimiser moments, loss rings)."""
    extra = (BRO, "algo.critic_width=64", f"algo.critic_blocks={K}", "algo.hidden_layers=[64]")
    a, memory = _agent(algo, *extra)
    _updates(a, memory, range(3))
    b, _ = _agent(algo, *extra)
    _updates(b, memory, range(1))
    torch.save(b.training_state(), tmp_path / "state.pt")
    c, _ = _agent(algo, *extra, seed=99)
    assert not torch.equal(c.critic.arena.data, b.critic.arena.data)
    c.load_training_state(torch.load(tmp_path / "state.pt", weights_only=False))
    _updates(c, memory, (1, 2))
    assert _same(_state(a), _state(c))


# --------------------------------------------------------------------------- it learns
# profiles/pointmass_learning_bro.json (tools/learn_pointmass.py --algos ddpg --shapes small --iters 500 --curve 63,125,250 --override
# algo.cri_class=DoubleQBroNet on an MI355X), DDPG at the small shape with the residual critic at its defaults (width 512, 2 blocks), f
# of seeds 0..4 by iteration count:
#    63: 0.9027 0.9752 0.9236 0.8894 0.9910    125: 0.8965 0.9801 0.9275 0.9433 0.9900    250: 0.9329 0.9627 0.9299 0.9732 0.9896
# 63 is the smallest count of the recorded curve at which the lowest of the five (seed 3: 0.8894) is >= 0.2.  The bar is half of the
# lowest of the five values at that count, the rule of f7-f9 / f13: the yardsticks (zero action, PD controller) depend on no learner
# kernel, and the half covers seed-to-seed and box-to-box spread.
LEARN_ITERS = 63        # rollout iterations (8 critic + 8 actor updates each); about 0.8 s on an MI355X
F_MIN = 0.5 * 0.8894


def test_ddpg_learns_pointmass_with_the_bronet_critic():
    """DDPG with `algo.cri_class=DoubleQBroNet` at (8, 2), 64 envs, batch 256, actor hidden [128, 128], episode_length 64, seed 0, 63
    iterations: the trained deterministic policy closes at least F_MIN = 0.5 x 0.8894 of the gap between the zero action and the PD
    controller.  Recorded f at 63 iterations, seeds 0-4: 0.9027, 0.9752, 0.9236, 0.8894, 0.9910."""
    lp = tc.load_script("tools/learn_pointmass.py", "learn_pointmass")
    r = lp.run("ddpg", "small", 0, LEARN_ITERS, (BRO,))
    print(f"pointmass ddpg + BroNet critic seed 0, {LEARN_ITERS} iterations: R={r['R']:.3f} R_zero={r['R_zero']:.3f} "
          f"R_pd={r['R_pd']:.3f} f={r['f']:.4f} wall={r['wall_s']}s")
    assert r["R_pd"] > r["R_zero"]
    assert r["f"] >= F_MIN, r
