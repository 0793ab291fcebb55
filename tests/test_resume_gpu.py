"""Save / resume of the full training state (pql_amd/utils/checkpoint.py), on the GPU.

The yardstick is the uninterrupted run of the same code on the same device: a run that is stopped at iteration k and resumed in
a NEW process must end with the same bits as a run that was never stopped.  Every run here is a child process with its own
timeout (Toy shape: obs 8, act 2, 64 envs, batch 256, ring 20 000 -- a few seconds each), one after the other; a failing child
ends the test.
"""
import importlib.util
import math
import os

import pytest
import torch

from resume_cases import BASELINE_KEYS, BASELINES, PQL, PQL_KEYS, PQL_TOY, TOY, child, same

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_RUNS = {}
A_CFG = ("algo.distl=False", "algo.graph=True", "algo.memory_size=20000")


def uninterrupted(tmp, *extra):
    """Run A: max_step=6000, no checkpoint keys.  Cached per configuration: several tests compare against the same one."""
    key = tuple(extra)
    if key not in _RUNS:
        _RUNS[key] = child(PQL, PQL_TOY + ["max_step=6000", *extra], tmp)
    return _RUNS[key]


def test_entry_point_is_deterministic(tmp_path):
    """Control: train_pql.main twice in fresh processes -> every fingerprint, counter and loss is equal."""
    a = uninterrupted(tmp_path, *A_CFG)
    b = child(PQL, PQL_TOY + ["max_step=6000", "algo.graph=True"], tmp_path)
    same(a, b, PQL_KEYS)
    assert a["resumed_from"] is None and a["rollout_iterations"] == 62 and a["critic_updates"] == 8 * 62


@pytest.mark.parametrize("distl,graph,memory", [(False, True, 20000), (True, True, 20000), (True, False, 20000), (False, False, 2500)])
def test_resume_is_bit_exact(tmp_path, distl, graph, memory):
    """A: 6000 steps.  B1: 3000 steps, checkpoint at stop.  B2 (new process): resume, to 6000.  B2 == A.  With a ring of 2500 rows
    (1920 after the warm-up) the ring wraps around iteration 10, B1 stops at 15: a wrapped ring, next_p and if_full are saved."""
    cfgs = [f"algo.distl={distl}", f"algo.graph={graph}", f"algo.memory_size={memory}"]
    a = uninterrupted(tmp_path, *cfgs)
    ck = tmp_path / "ck"
    b1 = child(PQL, PQL_TOY + ["max_step=3000", f"checkpoint.dir={ck}", *cfgs], tmp_path)
    assert b1["rollout_iterations"] == 15 and b1["critic_sha"] != a["critic_sha"]
    b2 = child(PQL, PQL_TOY + ["max_step=6000", f"resume={ck}", *cfgs], tmp_path)
    rf = b2["resumed_from"]
    assert rf["global_steps"] == b1["global_steps"] and os.path.basename(rf["path"]) == f"step-{b1['global_steps']}"
    same(rf, b1, ("critic_sha", "critic_target_sha", "actor_sha"))
    same(a, b2, PQL_KEYS)


def test_saving_has_no_side_effects_and_older_checkpoint_resumes(tmp_path):
    """C = A + periodic checkpoints: same result; `keep` checkpoints stay and `latest` names the newest; the OLDER one resumes to A."""
    a = uninterrupted(tmp_path, *A_CFG)
    ck = tmp_path / "ck2"
    c = child(PQL, PQL_TOY + ["max_step=6000", "algo.graph=True", f"checkpoint.dir={ck}", "checkpoint.freq=5"], tmp_path)
    same(a, c, PQL_KEYS)
    steps = sorted(int(n[len("step-"):]) for n in os.listdir(ck) if n.startswith("step-"))
    assert len(steps) == 2 and not [n for n in os.listdir(ck) if n.startswith(".tmp-")], os.listdir(ck)
    assert (ck / "latest").read_text().strip() == f"step-{steps[-1]}" and steps[-1] == a["global_steps"]
    d = child(PQL, PQL_TOY + ["max_step=6000", "algo.graph=True", f"resume={ck / ('step-%d' % steps[0])}"], tmp_path)
    assert d["resumed_from"]["global_steps"] == steps[0] < a["global_steps"]
    same(a, d, PQL_KEYS)


def test_two_stage_resume(tmp_path):
    """2000 -> resume -> 4000 -> resume -> 6000 equals A: state survives being loaded and saved again."""
    a = uninterrupted(tmp_path, *A_CFG)
    ck = tmp_path / "ck3"
    base = PQL_TOY + ["algo.graph=True", f"checkpoint.dir={ck}"]
    child(PQL, base + ["max_step=2000"], tmp_path)
    mid = child(PQL, base + ["max_step=4000", f"resume={ck}"], tmp_path)
    assert mid["resumed_from"]["global_steps"] < mid["global_steps"] < a["global_steps"]
    end = child(PQL, base + ["max_step=6000", f"resume={ck}"], tmp_path)
    assert end["resumed_from"]["global_steps"] == mid["global_steps"]
    same(a, end, PQL_KEYS)


@pytest.mark.parametrize("algo", ["ddpg_algo", "sac_algo", "crossq_algo"])
def test_baselines_resume_is_bit_exact(tmp_path, algo):
    base = TOY + [f"algo={algo}"]
    a = child(BASELINES, base + ["max_step=6000"], tmp_path)
    ck = tmp_path / "ck"
    b1 = child(BASELINES, base + ["max_step=3000", f"checkpoint.dir={ck}"], tmp_path)
    assert b1["actor_sha"] != a["actor_sha"] and sorted(os.listdir(ck / f"step-{b1['global_steps']}")) == ["ring.bin", "state.pt"]
    b2 = child(BASELINES, base + ["max_step=6000", f"resume={ck}"], tmp_path)
    assert b2["resumed_from"]["global_steps"] == b1["global_steps"]
    same(b2["resumed_from"], b1, ("actor_sha", "critic_sha"))
    same(a, b2, BASELINE_KEYS)


def test_resume_without_rings_repeats_the_warm_up(tmp_path):
    ck, ck_b2 = tmp_path / "ck", tmp_path / "ck_b2"
    b1 = child(PQL, PQL_TOY + ["max_step=3000", f"checkpoint.dir={ck}", "checkpoint.replay=False"], tmp_path)
    assert sorted(os.listdir(ck / f"step-{b1['global_steps']}")) == ["state.pt"]
    b2 = child(PQL, PQL_TOY + ["max_step=6000", f"resume={ck}", f"checkpoint.dir={ck_b2}"], tmp_path)
    assert "not bit-exact" in b2["_stderr"]
    rf = b2["resumed_from"]
    assert rf["global_steps"] == b1["global_steps"]
    same(rf, b1, ("critic_sha", "critic_target_sha", "actor_sha"))   # taken right after loading
    iters = b2["rollout_iterations"] - b1["rollout_iterations"]
    assert iters > 0
    assert b2["global_steps"] == b1["global_steps"] + 64 * 32 + 64 * iters > 6000       # the warm-up rollout ran again
    assert b2["critic_updates"] == b1["critic_updates"] + 8 * iters and b2["actor_updates"] == b1["actor_updates"] + 4 * iters
    assert math.isfinite(b2["critic_loss"]) and math.isfinite(b2["actor_loss"])
    # the rings started empty and the n-step windows with them: the warm-up left (32 - nstep + 1) * 64 = 1920 rows (>= batch_size
    # before the first learner step), every iteration 64 more
    st = torch.load(ck_b2 / f"step-{b2['global_steps']}" / "state.pt", map_location="cpu", weights_only=True)
    rows = 1920 + 64 * iters
    assert 1920 >= 256 and st["v_learner"]["memory"]["cur_capacity"] == rows and st["p_learner"]["memory"]["cur_capacity"] == rows
    assert st["rings"]["ring_v"]["bytes"] == rows * st["v_learner"]["memory"]["ring"]["rec_ld"] * 4


def test_free_running_resume(tmp_path):
    """algo.async_learners=True: the learner threads are parked at their locks during the save; counters continue; no equality of bits."""
    ck = tmp_path / "ck"
    base = PQL_TOY + ["algo.async_learners=True", "algo.eval_freq=100000", "algo.log_freq=100000", f"checkpoint.dir={ck}"]
    b1 = child(PQL, base + ["max_time=4"], tmp_path)
    b2 = child(PQL, base + ["max_time=8", f"resume={ck}"], tmp_path)   # max_time is a budget over the whole run
    print("free-running", {k: (b1[k], b2[k]) for k in ("global_steps", "critic_updates", "actor_updates", "rollout_iterations", "waits")})
    assert b2["resumed_from"]["global_steps"] == b1["global_steps"]
    st = torch.load(os.path.join(b2["resumed_from"]["path"], "state.pt"), map_location="cpu", weights_only=True)
    # the second session starts at the SAVED counters (the first session's threads took a few more steps between its save and
    # their stop, which nothing recorded) and grows from there
    v0, p0 = st["v_learner"]["update_count"], st["p_learner"]["update_count"]
    assert 0 <= b1["critic_updates"] - v0 <= 64 and 0 <= b1["actor_updates"] - p0 <= 64 and st["ratio"] is not None
    assert st["iter_t"] == b1["rollout_iterations"] and st["ratio"]["sim_count"] == b1["rollout_iterations"]
    iters = b2["rollout_iterations"] - b1["rollout_iterations"]
    dv, dp = b2["critic_updates"] - v0, b2["actor_updates"] - p0
    assert iters > 0 and dv > 0 and dp > 0 and b2["global_steps"] == b1["global_steps"] + 64 * iters
    # the design ratios, with the bounds of test_train_pql_free_running_with_ratio_controller
    assert 4.0 < dv / iters < 12.0, (dv, dp, iters)
    assert 1.5 < dv / dp < 2.7, (dv, dp, iters)
    assert dp / iters > 1.5, (dv, dp, iters)


def _load(path):
    spec = importlib.util.spec_from_file_location(os.path.basename(path)[:-3], path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_artifact_is_a_local_warm_start(tmp_path):
    from pql_amd.algo.pql_actor import PQLActor
    from pql_amd.algo.pql_p_learner import PQLPLearner
    from pql_amd.algo.pql_v_learner import PQLVLearner, make_actor, make_critic
    from pql_amd.envs.synthetic import create_task_env
    from pql_amd.utils import checkpoint as CK
    from pql_amd.utils.cfg import load_cfg
    from pql_amd.utils.model_util import load_model
    child(PQL, PQL_TOY + ["max_step=3000", f"+logging.dir={tmp_path}"], tmp_path)   # the evaluator writes <dir>/model.pth
    path = str(tmp_path / "model.pth")
    file = torch.load(path, map_location="cpu", weights_only=True)
    assert file["obs_rms"] is not None and file["actor"] and file["critic"]
    toy = PQL_TOY + ["device=cuda:0", "algo.v_learner_gpu=0", "algo.p_learner_gpu=0"]
    cfg = load_cfg(toy + [f"artifact={path}"])
    v, p = PQLVLearner((8,), 2, cfg), PQLPLearner((8,), 2, cfg)
    actor = PQLActor(create_task_env(cfg), cfg)
    for module, want in ((v.critic, file["critic"]), (v.critic_target, file["critic"]), (p.actor, file["actor"])):
        got = module.state_dict()
        assert sorted(got) == sorted(want)
        for k in want:
            assert torch.equal(got[k].cpu(), want[k]), k
    assert torch.equal(v.critic.arena.data, v.critic_target.arena.data)
    assert torch.equal(actor.obs_rms.mean.cpu(), file["obs_rms"][0]) and torch.equal(actor.obs_rms.var.cpu(), file["obs_rms"][1])
    # anything that is not an existing file is a W&B artifact name: still refused, in all three components
    wandb = load_cfg(toy + ["artifact=someone/project/model:v3"])
    for build in (lambda: PQLVLearner((8,), 2, wandb), lambda: PQLPLearner((8,), 2, wandb), lambda: PQLActor(create_task_env(wandb), wandb)):
        with pytest.raises(NotImplementedError, match="artifact"):
            build()
    # scripts/train_baselines.py, DDPG: actor + critic + obs_rms after the agent is built.  update_times=0: no gradient step, so the
    # run ends with the weights it was started from.
    plain = load_cfg(TOY + ["device=cuda:0"])
    plain.algo.v_learner_gpu = plain.algo.p_learner_gpu = 0
    ref_a, ref_c = make_actor(plain, (8,), 2, torch.device("cuda:0")), make_critic(plain, (8,), 2, torch.device("cuda:0"))
    load_model(ref_a, "actor", path)
    load_model(ref_c, "critic", path)
    mod = _load(BASELINES)
    with pytest.warns(RuntimeWarning):   # (the mean of zero losses)
        out = mod.main(load_cfg(TOY + ["algo=ddpg_algo", "algo.update_times=0", "max_step=2200", f"artifact={path}"]))
    assert out["actor_sha"] == CK.sha(ref_a.arena.data) and out["critic_sha"] == CK.sha(ref_c.arena.data)
    cold = mod.main(load_cfg(TOY + ["algo=ddpg_algo", "algo.update_times=0", "max_step=2200"]))
    assert cold["actor_sha"] != out["actor_sha"]
    with pytest.raises(NotImplementedError, match="artifact"):
        mod.main(load_cfg(TOY + ["algo=ddpg_algo", "max_step=2200", "artifact=someone/project/model:v3"]))


def test_refusals(tmp_path):
    ppo = ["task=Toy", "num_envs=64", "algo=ppo_algo", "max_step=3000"]
    r = child(BASELINES, ppo + [f"checkpoint.dir={tmp_path / 'ck'}"], tmp_path, check=False)
    assert r.returncode != 0 and "ValueError" in r.stderr and "ppo_algo" in r.stderr, r.stderr[-2000:]
    r = child(BASELINES, ppo + [f"resume={tmp_path / 'ck'}"], tmp_path, check=False)
    assert r.returncode != 0 and "ValueError" in r.stderr and "ppo_algo" in r.stderr, r.stderr[-2000:]
    # data parallel: the check sits in front of init_data_parallel, so this child needs no peer and cannot wait for one
    r = child(PQL, PQL_TOY + ["max_step=3000", f"checkpoint.dir={tmp_path / 'ck'}"], tmp_path, extra_env={"WORLD_SIZE": "2", "RANK": "0"},
              check=False, timeout=120)
    assert r.returncode != 0 and "ValueError" in r.stderr and "WORLD_SIZE=2" in r.stderr, r.stderr[-2000:]
    assert not os.path.exists(tmp_path / "ck")
