"""`DoubleQLayerNorm` (pql_amd/models/layernorm.py) and AgentDDPG / AgentSAC running with it, against tests/golden/layernorm.npz: the
torch twin (`nn.Sequential` with `nn.LayerNorm`) plugged into the reference's own AgentDDPG / AgentSAC by tools/gen_golden.py."""
import functools

import numpy as np
import pytest
import torch

import detdata as dd
import learner_harness as lh
import task_cases as tc
from learner_harness import _sd
from support import T, dev  # noqa: F401

pytestmark = pytest.mark.gpu

O, A, B = 8, 2, 64
LN = "algo.cri_class=DoubleQLayerNorm"
_fill = functools.partial(lh._fill, O, A)


def _check_views(views, g, prefix, rtol=5e-5, atol=5e-7):
    """The bars of the DDPG / SAC golden traces (tests/test_learners_gpu.py `_check_module`): fingerprint [sum, l2, probes...]; probes
    and l2 at rtol / atol, the cancelling plain sum at atol + 2e-6 l2."""
    for key, view in views:
        got, want = dd.summarize(view.cpu().numpy()), g[f"{prefix}{key}"]
        np.testing.assert_allclose(got[1:], want[1:], rtol=rtol, atol=atol, err_msg=prefix + key)
        np.testing.assert_allclose(got[0], want[0], rtol=rtol, atol=atol + 2e-6 * float(want[1]), err_msg=prefix + key + " (sum)")


def _cfg(algo, *extra):
    from pql_amd.utils.cfg import load_cfg
    return load_cfg([f"algo={algo}", "task.name=Toy", "num_envs=64", f"algo.batch_size={B}", "algo.memory_size=400", "device=cuda:0",
                     "sim_device=cuda:0", LN, *extra])


def _memory(dev):
    from pql_amd.replay.simple_replay import ReplayBuffer
    memory = ReplayBuffer(400, (O,), A, device=dev)
    memory.add_to_buffer(tuple(t.to(dev) for t in _fill(300, 810)))
    return memory


def _ddpg(golden, dev):
    from pql_amd.algo.ddpg import AgentDDPG
    from pql_amd.envs.synthetic import create_task_env
    from pql_amd.models.layernorm import DoubleQLayerNorm
    g = golden("layernorm")
    cfg = _cfg("ddpg_algo", "algo.no_tgt_actor=False")
    agent = AgentDDPG(create_task_env(cfg), cfg)
    # (the plugin table loads the class from its file: compare by name, not identity)
    assert type(agent.critic).__name__ == type(agent.critic_target).__name__ == DoubleQLayerNorm.__name__
    assert agent.critic_target._ws is not agent.critic._ws
    agent.actor.load_state_dict(_sd(dd.mlp_state(O, A, 11)))
    agent.actor_target.load_state_dict(_sd(dd.mlp_state(O, A, 13)))
    agent.critic.load_state_dict(_sd(dd.bn_critic_state(O, A, 43))); agent.critic_target.arena.data.copy_(agent.critic.arena.data)
    agent.obs_rms.mean, agent.obs_rms.var = T(g["ln_norm_mean"]).to(dev), T(g["ln_norm_var"]).to(dev)
    return agent, g


def _kat_inputs(dev):
    from pql_amd import _lib as L
    from pql_amd.models.mlp import pad_cols
    x = np.concatenate([dd.uniform((B, O), 73, -2, 2), dd.uniform((B, A), 74, -1, 1)], axis=1)
    return pad_cols(T(x).to(dev), L.ld(O + A))


def _critic(dev):
    from pql_amd.models.layernorm import DoubleQLayerNorm
    q = DoubleQLayerNorm((O,), A).to(dev)
    q.load_state_dict(_sd(dd.bn_critic_state(O, A, 43)))
    return q


def test_layernorm_critic_known_answer(golden, dev):
    """Forward (Q at atol 5e-6) and backward (dX and every parameter gradient's fingerprint, at the bars of test_crossq_golden_trace:
    rtol 5e-5, atol 1e-5) of one (2, B, 1) dq against the torch twin's autograd."""
    g = golden("layernorm")
    q = _critic(dev)
    x = _kat_inputs(dev)
    out = q.forward_raw(x)
    assert out.shape == (2, B, 32)
    np.testing.assert_allclose(out[0, :, :1].cpu().numpy(), g["ln_kat_q1"], atol=5e-6)
    np.testing.assert_allclose(out[1, :, :1].cpu().numpy(), g["ln_kat_q2"], atol=5e-6)
    q1, q2 = q.get_q1_q2(x[:, :O], x[:, O:O + A])
    assert torch.equal(q1, out[0, :, :1]) and torch.equal(q2, out[1, :, :1])
    assert torch.equal(q.get_q_min(x[:, :O], x[:, O:O + A]), torch.min(q1, q2)) and torch.equal(q.get_q1(x[:, :O], x[:, O:O + A]), q1)
    q.eval()                                                                    # no train / eval difference
    assert torch.equal(q.get_q1(x[:, :O], x[:, O:O + A]), q1)
    q.forward_raw(x)
    dq = torch.zeros((2, B, 32), device=dev); dq[:, :, :1] = T(g["ln_kat_dq"]).to(dev)
    grads = torch.zeros_like(q.arena.data)
    dx = q.backward_raw(x, dq, grads=grads, need_dx=True)
    np.testing.assert_allclose(dx[:, :O + A].cpu().numpy(), g["ln_kat_dx"], rtol=5e-5, atol=1e-5)
    for key, view in q.named_views(grads):
        got, want = dd.summarize(view.cpu().numpy()), g[f"ln_kat_g_{key}"]
        np.testing.assert_allclose(got[1:], want[1:], rtol=5e-5, atol=1e-5, err_msg=key)
        # The plain sum, summary entry 0.  LayerNorm's backward gives sum_j dz_rj = 0 in every row, so the sum over ALL entries of a
        # pre-norm Linear's dW (= sum_r sum_j dz_rj x_ri) and of its db is zero in exact arithmetic: the twin's own value there is the
        # rounding noise of its summation order (-6.4e-5 at an l2 of 75 for net_q1.net.3.weight), as BatchNorm's pre-norm bias gradient
        # is in test_crossq_golden_trace, which skips it.  Here it is not skipped but held, like every cancelling sum of the DDPG / SAC
        # traces (`_check_module`), to the absolute bar scaled by the tensor's l2 norm.
        layer = int(key.split(".")[2])
        cancels = layer % 3 == 0 and layer < 9
        np.testing.assert_allclose(got[0], want[0], rtol=5e-5, atol=1e-5 + (2e-6 * float(want[1]) if cancels else 0.0), err_msg=key + " (sum)")
    np.testing.assert_allclose(q.norm_param(0, 0, "gamma", grads).cpu().numpy(), g["ln_kat_g_q1_ln0_gamma"], rtol=5e-5, atol=1e-5)
    np.testing.assert_allclose(q.norm_param(0, 0, "beta", grads).cpu().numpy(), g["ln_kat_g_q1_ln0_beta"], rtol=5e-5, atol=1e-5)
    # pad entries of the gradient are zero: whatever is not a view of a parameter
    mask = torch.ones_like(grads, dtype=torch.bool)
    idx = torch.arange(grads.numel(), device=dev)
    for _, view in q.named_views(idx.to(torch.float32)):
        mask[view.reshape(-1).long()] = False
    assert bool((grads[mask] == 0).all()) and bool((q.arena.data[mask] == 0).all())
    # frozen parameters: the same dX bits, nothing else needed
    q.forward_raw(x)
    assert torch.equal(q.backward_raw(x, dq, grads=None, need_dx=True), dx)


def test_target_forward_does_not_disturb_the_stash(dev):
    """deepcopy gives the target its own workspace: a target forward between the online forward and its backward leaves the gradient's
    bits alone."""
    from copy import deepcopy
    q = _critic(dev)
    tgt = deepcopy(q)
    x, x2 = _kat_inputs(dev), _kat_inputs(dev).flip(0).contiguous()
    dq = torch.zeros((2, B, 32), device=dev); dq[:, :, 0] = T(dd.uniform((2, B), 76, -1, 1)).to(dev)
    outs = []
    for between in (False, True):
        mine = q.forward_raw(x).clone()
        if between:
            assert not torch.equal(tgt.forward_raw(x2), mine)
        grads = torch.zeros_like(q.arena.data)
        dx = q.backward_raw(x, dq, grads=grads, need_dx=True)
        outs.append((grads, dx.clone()))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    assert set(tgt._ws) == {B} and tgt._ws[B] is not q._ws[B]


def test_ddpg_layernorm_golden_trace(golden, dev):
    """AgentDDPG.update_once with DoubleQLayerNorm vs three iterations of the reference's AgentDDPG on the torch twin, identical samples
    and target-policy noise, no_tgt_actor=False: losses, every parameter tensor of actor, critic and both targets."""
    agent, g = _ddpg(golden, dev)
    memory = _memory(dev)
    for s in range(3):
        agent.update_once(memory, indices=T(g["ln_ddpg_idx"][s]), noise=T(g["ln_ddpg_noise"][s]))
        np.testing.assert_allclose(agent.closs[s % 5].item(), g["ln_ddpg_closs"][s], rtol=2e-5)
        np.testing.assert_allclose(agent.aloss[s % 5].item(), g["ln_ddpg_aloss"][s], rtol=2e-5, atol=1e-7)
        _check_views(agent.actor.named_views(), g, f"ln_ddpg_s{s}_a_")
        _check_views(agent.critic.named_views(), g, f"ln_ddpg_s{s}_c_")
        _check_views(agent.critic_target.named_views(), g, f"ln_ddpg_s{s}_t_")
        _check_views(agent.actor_target.named_views(), g, f"ln_ddpg_s{s}_at_")
    np.testing.assert_allclose(agent.actor.layout.weight(agent.actor.arena.data, 0, 3).cpu().numpy(), g["ln_ddpg_final_actor_last_w"],
                               rtol=5e-5, atol=5e-7)
    np.testing.assert_allclose(agent.critic.weight(0, 3).cpu().numpy(), g["ln_ddpg_final_q1_last_w"], rtol=5e-5, atol=5e-7)
    np.testing.assert_allclose(agent.critic_target.norm_param(0, 0, "gamma").cpu().numpy(), g["ln_ddpg_final_tq1_ln0_gamma"], rtol=5e-5, atol=5e-7)


def test_sac_layernorm_golden_trace(golden, dev):
    """AgentSAC.update_once with DoubleQLayerNorm vs the reference's AgentSAC on the torch twin: losses, log_alpha, every parameter."""
    from pql_amd.algo.sac import AgentSAC
    from pql_amd.envs.synthetic import create_task_env
    g = golden("layernorm")
    cfg = _cfg("sac_algo")
    agent = AgentSAC(create_task_env(cfg), cfg)
    agent.actor.load_state_dict(_sd(dd.mlp_state(O, 2 * A, 11)))
    agent.critic.load_state_dict(_sd(dd.bn_critic_state(O, A, 43))); agent.critic_target.arena.data.copy_(agent.critic.arena.data)
    agent.obs_rms.mean, agent.obs_rms.var = T(g["ln_norm_mean"]).to(dev), T(g["ln_norm_var"]).to(dev)
    memory = _memory(dev)
    for s in range(3):
        agent.update_once(memory, indices=T(g["ln_sac_idx"][s]), eps_next=T(g["ln_sac_eps"][2 * s]), eps_cur=T(g["ln_sac_eps"][2 * s + 1]))
        np.testing.assert_allclose(agent.closs[s % 5].item(), g["ln_sac_closs"][s], rtol=2e-5)
        np.testing.assert_allclose(agent.aloss[s % 5].item(), g["ln_sac_aloss"][s], rtol=2e-5, atol=1e-7)
        np.testing.assert_allclose(agent.log_alpha.item(), g["ln_sac_log_alpha"][s], rtol=1e-5)
        _check_views(agent.actor.named_views(), g, f"ln_sac_s{s}_a_")
        _check_views(agent.critic.named_views(), g, f"ln_sac_s{s}_c_")
        _check_views(agent.critic_target.named_views(), g, f"ln_sac_s{s}_t_")
    np.testing.assert_allclose(agent.actor.layout.weight(agent.actor.arena.data, 0, 3).cpu().numpy(), g["ln_sac_final_actor_last_w"],
                               rtol=5e-5, atol=5e-7)
    np.testing.assert_allclose(agent.critic.weight(0, 3).cpu().numpy(), g["ln_sac_final_q1_last_w"], rtol=5e-5, atol=5e-7)


def test_ddpg_layernorm_save_and_resume(golden, dev, tmp_path):
    """Training state saved after step 1 and loaded into a fresh agent: steps 2-3 are bit-equal to the uninterrupted run (arenas of
    actor, critic and both targets, optimiser moments, loss rings)."""
    memory = _memory(dev)

    def steps(agent, g, which):
        for s in which:
            agent.update_once(memory, indices=T(g["ln_ddpg_idx"][s]), noise=T(g["ln_ddpg_noise"][s]))
        torch.cuda.synchronize()

    a, g = _ddpg(golden, dev)
    steps(a, g, (0, 1, 2))
    b, _ = _ddpg(golden, dev)
    steps(b, g, (0,))
    torch.save(b.training_state(), tmp_path / "state.pt")
    c, _ = _ddpg(golden, dev)
    c.critic.arena.data.add_(1.0)                      # away from the saved state
    c.load_training_state(torch.load(tmp_path / "state.pt", weights_only=False))
    steps(c, g, (1, 2))
    ta, tc_ = a._state_tensors(), c._state_tensors()
    assert set(ta) == set(tc_) and {"critic", "critic_target", "actor_target", "copt.m", "aopt.v", "closs"} <= set(ta)
    for k in ta:
        assert torch.equal(ta[k], tc_[k]), k


# --------------------------------------------------------------------------- it learns
# profiles/pointmass_learning_ln.json (tools/learn_pointmass.py --override algo.cri_class=DoubleQLayerNorm on an MI355X), DDPG at the
# small shape with the LayerNorm critic, f of seeds 0..4 by iteration count:
#   125: 0.8752 0.8900 0.9250 0.8710 0.8767     250: 0.9244 0.9340 0.9304 0.8827 0.9356     500: 0.9538 0.9342 0.9562 0.9564 0.9537
# 125 is the smallest count at which the record's f (seed 0: 0.875; the lowest of the five: 0.871) is >= 0.2.  The bar is half of the
# lowest of the five values at that count, the rule of f7-f9: the yardsticks (zero action, PD controller) depend on no learner kernel,
# and the half covers seed-to-seed and box-to-box spread.
LEARN_ITERS = 125       # rollout iterations (8 critic + 8 actor updates each); about 0.8 s on an MI355X
F_MIN = 0.5 * 0.8710


def test_ddpg_learns_pointmass_with_layernorm_critic():
    """DDPG with `algo.cri_class=DoubleQLayerNorm` at (8, 2), 64 envs, batch 256, hidden [128, 128], episode_length 64, seed 0, 125
    iterations: the trained deterministic policy closes at least F_MIN = 0.5 x 0.8710 of the gap between the zero action and the PD
    controller.  Recorded f at 125 iterations, seeds 0-4: 0.8752, 0.8900, 0.9250, 0.8710, 0.8767."""
    lp = tc.load_script("tools/learn_pointmass.py", "learn_pointmass")
    r = lp.run("ddpg", "small", 0, LEARN_ITERS, (LN,))
    print(f"pointmass ddpg + LayerNorm critic seed 0, {LEARN_ITERS} iterations: R={r['R']:.3f} R_zero={r['R_zero']:.3f} "
          f"R_pd={r['R_pd']:.3f} f={r['f']:.4f} wall={r['wall_s']}s")
    assert r["R_pd"] > r["R_zero"]
    assert r["f"] >= F_MIN, r
