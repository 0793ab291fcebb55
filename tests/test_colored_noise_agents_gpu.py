"""The coloured exploration noise in the rollout and in training runs, on PointMass at (8, 2), 64 envs, hidden [32, 32], batch 64: white
is the code path it was (with the key, and with a config that lacks the keys), ar1 at rho = 0 is white's bits env feedback included,
the reset flags follow the raw done, seeded runs repeat, a slice of the global env axis has the global run's rows, and a run that is
stopped and resumed ends with the uninterrupted run's bits."""
import numpy as np
import pytest
import torch

import colored_noise_model as M
import detdata as dd
from resume_cases import BASELINE_KEYS, BASELINES, PQL, PQL_KEYS, child, same
from support import T, bits, dev  # noqa: F401
from task_cases import RecordingEnv

pytestmark = pytest.mark.gpu
N, O, A, HIDDEN = 64, 8, 2, (32, 32)
SHAPE = ["task=pointmass", f"task.obs_dim={O}", f"task.act_dim={A}", "algo.hidden_layers=[32, 32]", "algo.batch_size=64"]
NOISE_KEYS = ("color", "corr_min", "corr_max", "corr_groups", "octaves")
ITERS = 6


def _actor(dev, *extra, n=N, env_offset=0, total_envs=None, strip=False, prepare=None):
    """A rollout actor on a recording PointMass env with a fixed policy, everything from fixed seeds; strip: the config loses the
    colour keys after it is composed (a config written before they existed)."""
    from pql_amd.algo.pql_actor import PQLActor
    from pql_amd.envs.synthetic import create_task_env
    from pql_amd.models.mlp import TanhMLPPolicy
    from pql_amd.utils.cfg import load_cfg
    from pql_amd.utils.common import set_random_seed
    cfg = load_cfg([*SHAPE, f"num_envs={n}", "algo.v_learner_gpu=0", "algo.p_learner_gpu=0", "algo.num_gpus=1", "sim_device=cuda:0",
                    "device=cuda:0", "seed=3", *extra])
    if strip:
        for k in NOISE_KEYS:
            del cfg.algo.noise[k]
    set_random_seed(cfg.seed)
    inner = create_task_env(cfg, env_offset=env_offset)
    env = RecordingEnv(inner)
    actor = PQLActor(env, cfg, env_offset=env_offset, total_envs=total_envs)
    pol = TanhMLPPolicy((O,), A, hidden_layers=list(HIDDEN)).to(dev)
    pol.load_state_dict({k: T(v) for k, v in dd.mlp_state(O, A, 17, hidden=HIDDEN).items()})
    actor.set_actor(pol)
    actor.gen.manual_seed(4242)
    actor.reset_agent()
    if prepare is not None:
        prepare(inner)
        actor.obs = inner._observe()
    return actor, env


def _rollout(dev, *extra, iters=ITERS, **kw):
    """The training loops' order: a random warm-up that fills the n-step window (3 env steps), then `iters` rollout iterations of
    one env step -> (every emitted block, the recorded transitions, the last obs, the generator's state, the actor)."""
    actor, env = _actor(dev, *extra, **kw)
    actor.explore_env(env, 3, random=True)
    del env.log[:]
    blocks = []
    for _ in range(iters):
        _, v_data, steps = actor.explore_env(env, 1, random=False)
        assert steps == N
        torch.cuda.synchronize()
        blocks.append([t.detach().cpu().clone() for t in v_data])
    return blocks, env.log, actor.obs.cpu().clone(), actor.gen.get_state().clone(), actor


def _same_rollout(a, b):
    assert len(a[0]) == len(b[0]) and len(a[1]) == len(b[1]) == ITERS
    for x, y in zip(a[0], b[0]):
        assert len(x) == len(y) == 5 and all(torch.equal(p, q) for p, q in zip(x, y))
    for x, y in zip(a[1], b[1]):                       # action, next_obs, reward, done, truncated of every env step
        assert all(torch.equal(p, q) for p, q in zip(x, y))
    assert torch.equal(a[2], b[2]) and torch.equal(a[3], b[3])


def test_white_is_the_path_it_was_with_and_without_the_keys(dev):
    """color=white and a config that lacks the keys: no noise state, nothing new in the training state, and equal trajectories, obs
    and generator state after 6 rollout iterations."""
    with_key = _rollout(dev, "algo.noise.color=white")
    without = _rollout(dev, strip=True)
    _same_rollout(with_key, without)
    for run in (with_key, without):
        actor = run[4]
        assert actor._colored is None and not {"noise_state", "noise_fresh"} & set(actor._state_tensors())
    assert "color" not in without[4].cfg.algo.noise


def test_ar1_at_rho_zero_is_white_bit_for_bit(dev):
    """corr_min = corr_max = 0: the same draws from the generator (R = 1), the same actions, so the same env feedback."""
    white = _rollout(dev, "algo.noise.color=white")
    ar1 = _rollout(dev, "algo.noise.color=ar1", "algo.noise.corr_min=0.0", "algo.noise.corr_max=0.0")
    _same_rollout(white, ar1)
    assert {"noise_state", "noise_fresh"} <= set(ar1[4]._state_tensors())
    moved = _rollout(dev, "algo.noise.color=ar1")       # ... and the default correlation does move the actions
    assert not torch.equal(moved[1][-1][0], white[1][-1][0]) and torch.equal(moved[3], white[3])


@pytest.mark.parametrize("color, R", [("ar1", 1), ("pink", 6)])
def test_fresh_follows_the_raw_done_and_resets_the_state(dev, color, R):
    """episode_length 3, and some envs pushed out of the box so that episodes also end on their own: after every env step noise_fresh
    is that step's raw done (time limits included); the rows that were fresh going into a step leave it with state == the step's
    draw, the others with something else."""
    def leave_the_box(inner):
        inner.x[::4, 0], inner.v[::4, 0] = 1.4, 0.9

    actor, env = _actor(dev, f"algo.noise.color={color}", "task.episode_length=3", "algo.nstep=1", prepare=leave_the_box)
    g = torch.Generator().manual_seed(9)
    fresh_in = np.ones(N, dtype=bool)
    kinds = set()
    for step in range(8):
        d = torch.randn((N, R * A), generator=g)
        actor.explore_env(env, 1, random=False, draws=[d.to(dev)])
        torch.cuda.synchronize()
        st = actor._state_tensors()
        state, fresh = st["noise_state"].cpu().numpy(), st["noise_fresh"].cpu().numpy()
        done, trunc = env.log[-1][3].numpy().astype(bool), env.log[-1][4].numpy().astype(bool)
        assert fresh.dtype == np.uint8 and np.array_equal(fresh, done.astype(np.uint8)), step
        want = d.numpy().reshape(N, R, A)
        assert np.array_equal(bits(state[fresh_in]), bits(want[fresh_in])), step
        if (~fresh_in).any():
            carried = state[~fresh_in][:, -1]           # (pink's octave 0 has rho = 0: the slowest octave tells)
            assert not np.array_equal(carried, want[~fresh_in][:, -1]), step
        kinds |= {("limit" if t else "terminal") for dn, t in zip(done, trunc) if dn}
        if 0 < done.sum() < N:
            kinds.add("some")
        fresh_in = done
    assert kinds == {"limit", "terminal", "some"}, kinds


@pytest.mark.parametrize("extra", [("algo.noise.color=ar1",), ("algo.noise.color=pink",), ("algo.noise.color=pink", "algo.noise.type=fixed")],
                         ids=["ar1", "pink", "pink_fixed"])
def test_two_seeded_runs_give_the_same_bits(dev, extra):
    a, b = _rollout(dev, *extra), _rollout(dev, *extra)
    _same_rollout(a, b)
    sa, sb = a[4]._state_tensors(), b[4]._state_tensors()
    assert torch.equal(sa["noise_state"], sb["noise_state"]) and torch.equal(sa["noise_fresh"], sb["noise_fresh"])
    assert bool(sa["noise_state"].abs().sum() > 0)


@pytest.mark.parametrize("color, R", [("ar1", 1), ("pink", 6)])
def test_a_slice_of_the_global_env_axis_has_the_global_runs_rows(dev, color, R):
    """Envs [16, 48) as a rank with env_offset 16 of 64 against the 64-env run, injected draws, a policy whose action is 0 for every
    row (zero weights), so the action is the clamped noise: correlation groups and mixed sigma are taken at the GLOBAL env index."""
    lo, hi = 16, 48
    full, _ = _actor(dev, f"algo.noise.color={color}")
    part, _ = _actor(dev, f"algo.noise.color={color}", n=hi - lo, env_offset=lo, total_envs=N)
    for a in (full, part):
        a.actor.arena.data.zero_()
        a.set_actor(a.actor)
    g = torch.Generator().manual_seed(21)
    obs = torch.randn((N, O), generator=g).to(dev)
    rho, coef, w = M.tables(color, groups=8, octaves=R)
    sigma = torch.linspace(0.05, 0.8, N).numpy()
    state = np.zeros((N, R, A), dtype=np.float32)
    for step in range(4):
        d = torch.randn((N, R * A), generator=g)
        done = torch.rand(N, generator=g) < (2.0 if step == 0 else 0.3)
        if step > 0:
            full._colored.mark(done.to(dev))
            part._colored.mark(done[lo:hi].to(dev))
        out_full = full.get_actions(obs, sample=True, draw=d.to(dev)).cpu()
        out_part = part.get_actions(obs[lo:hi].contiguous(), sample=True, draw=d[lo:hi].contiguous().to(dev)).cpu()
        assert torch.equal(out_part, out_full[lo:hi]), step
        assert torch.equal(part._colored.state.cpu(), full._colored.state.cpu()[lo:hi]), step
        want, state = M.step(np.zeros((N, A), dtype=np.float32), d.numpy(), sigma, rho, coef, w, 0, done.numpy(), state)
        assert np.array_equal(bits(out_full.numpy()), bits(want)), step       # ... and both are the law's bits
    assert len({float(x) for x in full._colored.rho.cpu().reshape(-1)}) == (8 if color == "ar1" else R)


# --------------------------------------------------------------------------- resume
def _upto(iters):
    return f"max_step={(32 + iters) * N - 1}"          # the warm-up's 32 env steps, then one per iteration


RUNS = {"ddpg": (BASELINES, ["algo=ddpg_algo"], BASELINE_KEYS, "iters"), "pql": (PQL, ["algo.num_gpus=1"], PQL_KEYS, "rollout_iterations")}


@pytest.mark.parametrize("color", ["ar1", "pink"])
@pytest.mark.parametrize("run", sorted(RUNS))
def test_resume_is_bit_exact(tmp_path, run, color):
    """8 iterations uninterrupted == 4 iterations, checkpoint, a fresh process, to 8: the processes' state and reset flags travel."""
    script, algo, keys, count = RUNS[run]
    base = [*algo, *SHAPE, f"num_envs={N}", "algo.memory_size=4000", "task.episode_length=5", f"algo.noise.color={color}"]
    a = child(script, base + [_upto(8)], tmp_path)
    ck = tmp_path / "ck"
    b1 = child(script, base + [_upto(4), f"checkpoint.dir={ck}"], tmp_path)
    assert (a[count], b1[count]) == (8, 4) and b1["actor_sha"] != a["actor_sha"]
    b2 = child(script, base + [_upto(8), f"resume={ck}"], tmp_path)
    assert b2["resumed_from"]["global_steps"] == b1["global_steps"]
    same(b2["resumed_from"], b1, ("actor_sha", "critic_sha"))
    same(a, b2, keys)


def test_a_white_checkpoint_is_refused_under_a_colour(tmp_path):
    base = ["algo=ddpg_algo", *SHAPE, f"num_envs={N}", "algo.memory_size=4000"]
    ck = tmp_path / "ck"
    child(BASELINES, base + [_upto(2), f"checkpoint.dir={ck}"], tmp_path)
    r = child(BASELINES, base + [_upto(4), f"resume={ck}", "algo.noise.color=ar1"], tmp_path, check=False)
    assert r.returncode != 0 and "ValueError" in r.stderr and "noise_state" in r.stderr and "one side only" in r.stderr, r.stderr[-2000:]
