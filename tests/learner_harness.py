"""What the learner tests of every critic class share: configurations, deterministic weights and replay rows, a V-learner with a
policy, statistics and rows in its ring, its state for bit-for-bit comparisons, and the comparison against an autograd learner's
nets.  The shapes are arguments; the seeds, the generator call order and the data ranges are fixed here, and inputs to golden and
bit-for-bit comparisons come out of these functions.  Not collected as tests."""
import numpy as np
import torch

import detdata as dd
from support import T

PER = ("algo.per.enabled=True", "algo.per.refresh=run", "algo.per.alpha=0.5", "algo.per.eps=1.0e-3")


def make_cfg(distl=False, B=64, memory=400, hidden=None, graph=False, nstep=3, streams=False, task=None):
    """streams=False: learner work on the caller's stream (results readable right after the call); streams=True: the
    learners' own HIP streams with event-fenced hand-offs -- read results after `learner.synchronize()`."""
    from pql_amd.utils.cfg import load_cfg
    ov = [f"algo.batch_size={B}", f"algo.memory_size={memory}", f"algo.distl={distl}", "algo.v_learner_gpu=0",
          "algo.p_learner_gpu=0", "algo.num_gpus=1", f"algo.graph={graph}", f"algo.nstep={nstep}", f"algo.streams={streams}"]
    if task:
        ov.append(f"task={task}")
    cfg = load_cfg(ov)
    cfg.algo.hidden_layers = hidden
    return cfg


def _sd(state):
    return {k: T(v) for k, v in state.items()}


def _fill(O, A, rows, seed, rew=0.05):
    return (T(dd.uniform((rows, O), seed, -3, 3)), T(dd.uniform((rows, A), seed + 1)), T(dd.uniform((rows, 1), seed + 2, -rew, rew)),
            T(dd.uniform((rows, O), seed + 3, -3, 3)), T(dd.bernoulli((rows, 1), seed + 4, 0.1)))


def _compare_nets(module, nets, what=None, rtol=1e-5, atol=1e-5):
    lay, pre = module.layout, "" if what is None else f"{what} "
    for n, net in enumerate(nets):
        for l in range(lay.n_layers):
            np.testing.assert_allclose(lay.weight(module.arena.data, n, l).cpu().numpy(), net[2 * l].detach().numpy(), rtol=rtol, atol=atol,
                                       err_msg=f"{pre}net {n} layer {l} weight")
            np.testing.assert_allclose(lay.bias(module.arena.data, n, l).cpu().numpy(), net[2 * l + 1].detach().numpy(), rtol=rtol, atol=atol,
                                       err_msg=f"{pre}net {n} layer {l} bias")


def _rows(O, A, n, seed, device):
    g = torch.Generator().manual_seed(seed)
    u = lambda shape, lo, hi: (torch.rand(shape, generator=g) * (hi - lo) + lo).to(device)  # noqa: E731
    return (u((n, O), -3, 3), u((n, A), -1, 1), u((n, 1), -0.5, 0.5), u((n, O), -3, 3), (torch.rand((n, 1), generator=g) < 0.1).float().to(device))


def _learner(cfg_of, O, A, rows, seed=11):
    """A V-learner on the configuration `cfg_of()` (made after the seeding), a policy, statistics and `rows` rows in the ring."""
    from pql_amd.algo.learner import make_actor
    from pql_amd.algo.pql_v_learner import PQLVLearner
    torch.manual_seed(seed)
    cfg = cfg_of()
    v = PQLVLearner((O,), A, cfg)
    actor = make_actor(cfg, (O,), A, v.device)
    g = torch.Generator().manual_seed(seed + 1)
    norm = ((torch.rand(O, generator=g) - 0.5).to(v.device), (torch.rand(O, generator=g) * 1.5 + 0.5).to(v.device), 1e-4)
    v.update(actor, _rows(O, A, rows, seed + 2, v.device), norm, 0)
    return v, actor, norm


def _state(v):
    v.flush_priorities()
    torch.cuda.synchronize()
    out = dict(critic=v.critic.arena.data, target=v.critic_target.arena.data, adam_m=v.opt.m, adam_v=v.opt.v, adam_step=v.opt.step,
               loss_ring=v.loss_ring)
    if getattr(v.memory, "prioritized", False):
        out.update(tree=v.memory.tree, pmax=v.memory.pmax)
    return {k: t.detach().cpu().clone() for k, t in out.items()}


def _same_state(a, b):
    assert set(a) == set(b)
    for k in a:
        assert torch.equal(a[k], b[k]) and a[k].dtype == b[k].dtype, k


def _run(v, mode, n):
    if mode == "run":
        v.learn_many(n)
    else:
        for _ in range(n):
            v.learn()
