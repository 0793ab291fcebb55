"""PPO baseline, CPU side: config composition and presets, the C ABI's declarations and argument errors, the class registry,
the reference's state_dict keys and checkpoint format.  No kernel is launched here."""
import ctypes as C
import os

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PPO_SYMBOLS = ("pqlk_gae", "pqlk_ppo_gauss_head", "pqlk_ppo_gather_parts", "pqlk_ppo_gather", "pqlk_ppo_scratch_floats",
               "pqlk_ppo_policy_loss", "pqlk_ppo_value_loss")


def _cfg(*ov):
    from pql_amd.utils.cfg import load_cfg
    return load_cfg(["algo=ppo_algo", *ov])


def test_ppo_algo_composes_to_the_reference_values():
    c = _cfg()
    a = c.algo
    assert a.name == "PPO" and a.batch_size == 32768   # _self_ overrides actor_critic.yaml's 8192
    assert (a.horizon_len, a.update_times, a.gamma, a.eval_freq) == (16, 4, 0.99, 20)
    assert (a.use_gae, a.value_clip, a.lambda_gae_adv, a.lambda_entropy, a.ratio_clip) == (True, True, 0.95, 0.0, 0.2)
    assert (a.act_class, a.cri_class, a.no_tgt_actor) == ("DiagGaussianMLPPolicy", "MLPCritic", True)
    assert (a.actor_lr, a.critic_lr, a.max_grad_norm, a.obs_norm, a.value_norm, a.handle_timeout) == (5e-4, 5e-4, 0.5, True, False, True)
    assert _cfg("algo.batch_size=512").algo.batch_size == 512


@pytest.mark.parametrize("task,want", [
    ("Ant", (4096, 32768, 16, 4, False)),
    ("Humanoid", (4096, 32768, 32, 5, True)),
    ("Anymal", (4096, 32768, 16, 5, False)),
    ("AllegroHand", (16384, 32768, 8, 5, True)),
    ("FrankaCubeStack", (8192, 16384, 32, 5, False)),
    ("ShadowHand", (4096, 32768, 16, 4, False)),   # the reference compares cfg.task (not .name) with 'ShadowHand': never matches
    ("Toy", (4096, 32768, 16, 4, False)),
])
def test_isaac_param_presets(task, want):
    from pql_amd.utils.common import preprocess_cfg
    c = _cfg("isaac_param=True", f"task.name={task}")
    preprocess_cfg(c)
    assert (c.num_envs, c.algo.batch_size, c.algo.horizon_len, c.algo.update_times, c.algo.value_norm) == want
    d = _cfg(f"task.name={task}")   # isaac_param=False: untouched
    preprocess_cfg(d)
    assert (d.num_envs, d.algo.batch_size, d.algo.horizon_len, d.algo.update_times, d.algo.value_norm) == (4096, 32768, 16, 4, False)


def test_ppo_symbols_are_declared_and_exported():
    from pql_amd import _lib as L
    text = open(os.path.join(ROOT, "include", "pqlk.h")).read()
    raw = C.CDLL(os.fspath(L.LIB_FILE))
    for s in PPO_SYMBOLS:
        assert f"{s}(" in text and s in L.PROTOTYPES and hasattr(raw, s), s
    assert L.lib.pqlk_ppo_gather_parts(32768) == 512 and L.lib.pqlk_ppo_gather_parts(24) == 1 and L.lib.pqlk_ppo_gather_parts(0) == 0
    assert L.lib.pqlk_ppo_scratch_floats(32768, 16) == 256 * 17
    assert L.lib.pqlk_ppo_scratch_floats(16, 2) == 1 * 3
    assert L.lib.pqlk_ppo_scratch_floats(100, 65) == 0


def test_ppo_c_abi_reports_argument_errors_as_codes():
    from pql_amd import _lib as L
    E_NULL, E_SHAPE, E_RANGE, E_WORKSPACE = 1, 2, 3, 6
    P = C.c_void_p(0x1000)
    lib = L.lib
    assert lib.pqlk_gae(None, P, P, P, P, None, 4, 8, 0.99, 0.95, 1, P, P, None) == E_NULL
    assert lib.pqlk_gae(P, P, P, P, P, None, 0, 8, 0.99, 0.95, 1, P, P, None) == E_SHAPE
    assert lib.pqlk_gae(P, P, P, P, P, None, 4, 0, 0.99, 0.95, 1, P, P, None) == E_SHAPE
    assert lib.pqlk_ppo_gauss_head(P, 32, None, P, 4, 2, P, 2, P, None, None) == E_NULL
    assert lib.pqlk_ppo_gauss_head(P, 32, P, P, 4, 65, P, 65, P, None, None) == E_SHAPE
    assert lib.pqlk_ppo_gauss_head(P, 1, P, P, 4, 2, P, 2, P, None, None) == E_SHAPE
    g = lambda **k: lib.pqlk_ppo_gather(*[k.get(n, d) for n, d in (  # noqa: E731
        ("idx", P), ("mb", 4), ("rows", 8), ("obs", P), ("O", 8), ("mean", P), ("var", P), ("eps", 1e-4), ("x", P), ("ldx", 32),
        ("act", P), ("A", 2), ("act_out", P), ("logp", P), ("adv", P), ("ret", P), ("val", P), ("lo", P), ("ao", P), ("ro", P),
        ("vo", P), ("part", P), ("st", None))])
    assert g(idx=None) == E_NULL and g(part=None) == E_NULL
    assert g(mean=None) == E_NULL                     # mean and var come together
    assert g(mb=0) == E_SHAPE and g(ldx=4) == E_SHAPE
    pl = lambda **k: lib.pqlk_ppo_policy_loss(*[k.get(n, d) for n, d in (  # noqa: E731
        ("y", P), ("ld", 32), ("ls", P), ("act", P), ("old", P), ("adv", P), ("part", P), ("np", 1), ("b", 64), ("A", 2), ("clip", 0.2),
        ("lam", 0.0), ("dy", P), ("dls", P), ("lp", None), ("sc", P), ("scn", 4096), ("ring", P), ("slot", P), ("rl", 4), ("st", None))])
    assert pl(dy=None) == E_NULL and pl(sc=None) == E_NULL
    assert pl(b=0) == E_SHAPE and pl(A=0) == E_SHAPE and pl(A=65) == E_SHAPE and pl(np=0) == E_SHAPE and pl(rl=0) == E_SHAPE
    assert pl(clip=-0.1) == E_RANGE
    assert pl(scn=2) == E_WORKSPACE
    vl = lambda **k: lib.pqlk_ppo_value_loss(*[k.get(n, d) for n, d in (  # noqa: E731
        ("v", P), ("ld", 32), ("ret", P), ("old", P), ("b", 64), ("clip_on", 1), ("clip", 0.2), ("dy", P), ("lddy", 32), ("sc", P),
        ("scn", 256), ("ring", P), ("slot", P), ("rl", 4), ("st", None))])
    assert vl(old=None) == E_NULL and vl(ret=None) == E_NULL
    assert vl(b=0) == E_SHAPE and vl(clip=-1.0) == E_RANGE and vl(scn=0) == E_WORKSPACE


def test_registry_resolves_the_ppo_classes():
    from pql_amd.algo import alg_name_to_path
    from pql_amd.models import model_name_to_path
    assert alg_name_to_path["AgentPPO"].name == "ppo.py"
    for name in ("DiagGaussianMLPPolicy", "MLPCritic"):
        assert model_name_to_path.resolve(name).__name__ == name
    import pql.algo.ppo
    import pql.models.mlp
    import pql_amd.algo.ppo
    import pql_amd.models.mlp
    assert pql.algo.ppo.AgentPPO is pql_amd.algo.ppo.AgentPPO
    assert pql.models.mlp.DiagGaussianMLPPolicy is pql_amd.models.mlp.DiagGaussianMLPPolicy
    assert pql.models.mlp.MLPCritic is pql_amd.models.mlp.MLPCritic


def test_state_dict_keys_and_flat_buffer():
    from pql_amd import _lib as L
    from pql_amd.models.mlp import DiagGaussianMLPPolicy, MLPCritic
    pol = DiagGaussianMLPPolicy((88,), 16, init_log_std=-0.5)
    keys = list(pol.state_dict())
    assert keys == [f"net.{i}.{k}" for i in (0, 2, 4, 6) for k in ("weight", "bias")] + ["logstd"]
    assert pol.arena.numel() == pol.layout.total + L.ld(16)
    assert torch.all(pol.logstd == -0.5) and torch.count_nonzero(pol.logstd_block(pol.arena.data)[16:]) == 0
    assert pol.num_params() == sum(v.numel() for v in pol.state_dict().values())
    cri = MLPCritic((88,), 16)
    assert list(cri.state_dict()) == [f"critic.net.{i}.{k}" for i in (0, 2, 4, 6) for k in ("weight", "bias")]
    assert cri.layout.dims == [88, 512, 256, 128, 1]
    with pytest.raises(RuntimeError):
        pol.load_state_dict({k: v for k, v in pol.state_dict().items() if k != "logstd"})


def test_reference_checkpoint_round_trip(golden, tmp_path):
    """The reference's own PPO checkpoint (weights held in tests/golden/ckpt.npz) loads into the new classes and saves back in the
    same format and key set."""
    from pql_amd.models.mlp import DiagGaussianMLPPolicy, MLPCritic
    from pql_amd.utils.model_util import load_model, save_model
    g = golden("ckpt")
    actor_sd = {k[len("actor_w_"):]: torch.from_numpy(v) for k, v in g.items() if k.startswith("actor_w_")}
    actor_sd["logstd"] = torch.from_numpy(g["actor_logstd"])
    critic_sd = {"critic." + k[len("critic_w_"):]: torch.from_numpy(v) for k, v in g.items() if k.startswith("critic_w_")}
    O, A = actor_sd["net.0.weight"].shape[1], actor_sd["net.6.weight"].shape[0]
    path = tmp_path / "model.pth"
    torch.save({"obs_rms": None, "actor": actor_sd, "critic": critic_sd}, path)
    pol, cri = DiagGaussianMLPPolicy((O,), A), MLPCritic((O,), A)
    assert load_model(pol, "actor", path) and load_model(cri, "critic", path)
    for k, v in actor_sd.items():
        assert torch.equal(pol.state_dict()[k], v), k
    for k, v in critic_sd.items():
        assert torch.equal(cri.state_dict()[k], v), k
    out = tmp_path / "again.pth"
    save_model(out, pol, cri, None)
    back = torch.load(out, weights_only=True)
    assert set(back["actor"]) == set(actor_sd) and set(back["critic"]) == set(critic_sd)
    assert torch.equal(back["actor"]["logstd"], actor_sd["logstd"])


def test_train_baselines_has_the_on_policy_branch():
    src = open(os.path.join(ROOT, "scripts", "train_baselines.py")).read()
    assert 'is_off_policy = cfg.algo.name != "PPO"' in src
    assert "agent.update_net(trajectory)" in src


def test_minibatch_plan_keeps_the_short_last_minibatch():
    from pql_amd.algo.ppo import AgentPPO
    a = AgentPPO.__new__(AgentPPO)
    a.cfg = _cfg("algo.batch_size=24")
    assert a.minibatch_plan(64) == [(0, 24), (24, 48), (48, 64)]
    assert a.minibatch_plan(16) == [(0, 16)]
    a.cfg = _cfg()
    assert len(a.minibatch_plan(16384 * 8)) == 4
