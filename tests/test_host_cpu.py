"""CPU-side checks: the C-ABI library loads and exports every symbol include/pqlk.h declares, the
host-side integer logic (ring pointer law, arena layout) matches the oracle / reference fixtures, and
the product refuses to run without a GPU (no fallback).  No kernel is launched here."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import detdata as dd
from task_cases import load_script

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared_symbols():
    text = open(os.path.join(ROOT, "include", "pqlk.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(pqlk_[a-z0-9_]+)\s*\(", text)))


def test_library_exports_every_declared_symbol():
    from pql_amd import _lib as L
    names = _declared_symbols()
    assert len(names) >= 20
    raw = C.CDLL(os.fspath(L.LIB_FILE))
    for n in names:
        assert hasattr(raw, n), f"libpqlk.so does not export {n}"
    assert set(names) == set(L.PROTOTYPES), "ctypes prototypes out of sync with include/pqlk.h"
    assert L.lib.pqlk_version() == 100
    assert b"NULL" in L.lib.pqlk_strerror(1) and L.lib.pqlk_strerror(0) == b"ok"


def test_host_side_argument_errors_without_gpu():
    """Argument validation happens before any launch, so it is checkable on CPU."""
    from pql_amd import _lib as L
    assert L.lib.pqlk_replay_insert(None, 0, 0, None, 0, None, 0, None, 0, None, 0, None, 0, None) == 1
    d = L.mlp_desc([104, 512, 256, 128, 1], 3)
    assert L.lib.pqlk_mlp_param_floats(C.byref(d)) == 0          # n_nets = 3 unsupported
    with pytest.raises(L.PqlkError):
        L.mlp_desc([4], 1)


def test_ld_and_record_layout():
    from pql_amd import _lib as L
    assert [L.ld(c) for c in (1, 32, 33, 104, 231)] == [32, 32, 64, 128, 256]
    rec = L.lib.pqlk_replay_rec_ld
    assert rec(88, 16) == 224 and rec(211, 20) == 448 and rec(108, 21) == 256 and rec(8, 2) == 32
    assert rec(88, -1) == 96 and rec(211, -1) == 224


@pytest.mark.parametrize("name", ["wrap4", "exact", "ragged"])
def test_ring_plan_matches_reference_trace(golden, name):
    from oracle import pql_ref_cpu as ref
    from pql_amd.replay.simple_replay import ring_plan
    g = golden("replay")
    cap = int(g[f"ring_{name}_meta"][0])
    p, full = 0, False
    for step, m in enumerate(int(v) for v in g[f"ring_{name}_inserts"]):
        expect = ref.ring_plan(p, full, cap, m)
        segs, p, full, cur = ring_plan(p, full, cap, m)
        assert (segs, p, full, cur) == expect
        assert [p, cur, int(full)] == g[f"ring_{name}_trace"][step].tolist()
    with pytest.raises(RuntimeError):
        ring_plan(3, False, 10, 25)


def test_arena_layout_and_state_dict_roundtrip():
    from pql_amd.models.mlp import DoubleQ, TanhMLPPolicy, DistributionalDoubleQ
    q = DoubleQ((88,), 16)
    assert q.num_params() == 436226 and q.layout.total % 32 == 0
    assert TanhMLPPolicy((88,), 16).num_params() == 211856
    assert DistributionalDoubleQ((211,), 20, device="cpu").num_params() == 579174
    st = {k: torch.from_numpy(v) for k, v in dd.doubleq_state(88, 16, 1, 21).items()}
    q.load_state_dict(st)
    back = q.state_dict()
    assert list(back) == list(st)
    for k in st:
        assert torch.equal(back[k], st[k]), k
    # pads stay zero: arena mass equals the mass of the logical views
    views = sum(v.abs().sum().item() for _, v in q.named_views())
    np.testing.assert_allclose(q.arena.data.abs().sum().item(), views, rtol=1e-6)
    with pytest.raises(RuntimeError):
        q.load_state_dict({"net_q1.net.0.weight": torch.zeros(3, 3)})


def test_reference_checkpoint_key_format_loads():
    """Rank-1 'next' item of SURVEY 8f: the on-disk dict format {'obs_rms','actor','critic'} with the
    reference key names.  (The reference's own pql/model.pth is a PPO checkpoint with a different head
    and is not read here; the key format is what matters.)"""
    from pql_amd.models.mlp import TanhMLPPolicy
    a = TanhMLPPolicy((8,), 2)
    sd = {k: torch.from_numpy(v) for k, v in dd.mlp_state(8, 2, 11).items()}
    assert sorted(sd) == sorted(["net.0.weight", "net.0.bias", "net.2.weight", "net.2.bias", "net.4.weight",
                                 "net.4.bias", "net.6.weight", "net.6.bias"])
    a.load_state_dict(sd)
    assert torch.equal(a.state_dict()["net.6.bias"], sd["net.6.bias"])


def test_model_registry_resolves_by_class_name():
    from pql_amd.models import model_name_to_path
    from pql_amd.utils.common import load_class_from_path
    for name in ("TanhMLPPolicy", "DoubleQ", "DistributionalDoubleQ", "MLPNet"):
        cls = load_class_from_path(name, model_name_to_path[name])
        assert cls.__name__ == name


def test_product_refuses_cpu_tensors():
    from pql_amd._lib import PqlkError
    from pql_amd.models.mlp import TanhMLPPolicy
    from pql_amd.replay.nstep_replay import NStepReplay
    from pql_amd.replay.simple_replay import ReplayBuffer
    with pytest.raises(PqlkError):
        ReplayBuffer(10, (3,), 2, device="cpu")
    with pytest.raises(PqlkError):
        NStepReplay((3,), 2, 4, 3, device="cpu")
    with pytest.raises(PqlkError):
        TanhMLPPolicy((3,), 2)(torch.zeros(5, 3))      # CPU arena -> loud failure, never an eager fallback


def test_checkpoint_roundtrip_in_reference_format(tmp_path):
    """{'obs_rms','actor','critic'} with the reference's state_dict keys, loadable with
    weights_only=True (nothing is unpickled)."""
    from pql_amd.models.mlp import DoubleQ, TanhMLPPolicy
    from pql_amd.utils.model_util import load_model, save_model
    a, q = TanhMLPPolicy((8,), 2), DoubleQ((8,), 2)
    rms = (torch.arange(8.0), torch.ones(8) * 2, 1e-4)
    path = tmp_path / "model.pth"
    save_model(path, a, q, rms)
    raw = torch.load(path, weights_only=True)
    assert sorted(raw) == ["actor", "critic", "obs_rms"] and "net_q2.net.6.bias" in raw["critic"] and "net.0.weight" in raw["actor"]
    a2, q2 = TanhMLPPolicy((8,), 2), DoubleQ((8,), 2)
    assert load_model(a2, "actor", path) and load_model(q2, "critic", path)
    assert torch.equal(a2.arena.data, a.arena.data) and torch.equal(q2.arena.data, q.arena.data)
    holder = type("R", (), {"mean": torch.zeros(8), "var": torch.ones(8), "epsilon": 0.0})()
    assert load_model(holder, "obs_rms", path) and torch.equal(holder.mean, rms[0]) and holder.epsilon == 1e-4
    with pytest.raises(KeyError):
        load_model(a2, "policy", path)


def test_noise_schedules_match_reference_semantics():
    from pql_amd.utils.schedule_util import ExponentialSchedule, LinearSchedule
    lin = LinearSchedule(0.8, 0.05, 4)
    assert [round(lin.step(), 4) for _ in range(7)] == [0.8, 0.6125, 0.425, 0.2375, 0.05, 0.05, 0.05]
    ex = ExponentialSchedule(0.8, 0.5, 0.05)
    assert ex.total_iters == 4 and [round(ex.step(), 4) for _ in range(6)] == [0.4, 0.2, 0.1, 0.05, 0.025, 0.025]


def test_config_composition_and_overrides():
    from pql_amd.utils.cfg import load_cfg
    c = load_cfg([])
    assert (c.algo.name, c.algo.nstep, c.algo.critic_sample_ratio, c.algo.critic_actor_ratio) == ("PQL", 3, 8, 2)
    assert int(c.algo.memory_size) == 5_000_000 and c.algo.noise.tgt_pol_noise_bound == 0.2 and c.sim_device == "cuda"
    assert (c.algo.v_learner_gpu, c.algo.p_learner_gpu, c.algo.num_gpus, c.algo.distl, c.algo.num_atoms) == (1, 1, 2, False, 51)
    d = load_cfg(["algo=ddpg_algo", "algo.batch_size=256", "num_envs=64", "task.name=Toy", "algo.noise.std_max=0.5"])
    assert (d.algo.name, d.algo.update_times, d.algo.batch_size, d.num_envs, d.algo.noise.std_max) == ("DDPG", 8, 256, 64, 0.5)
    assert d.algo.max_grad_norm == 0.5 and d.algo.tau == 0.05   # inherited through off_policy.yaml <- actor_critic.yaml


# --------------------------------------------------------------------------- evaluator
def _reference_style_eval(cfg, policy, states):
    """pql/utils/evaluator.py:41-121 restated with the host-side Tracker (the form the reference runs)."""
    from pql_amd.envs.synthetic import create_task_env
    from pql_amd.utils.common import Tracker
    n = int(cfg.eval_num_envs)
    env = create_task_env(cfg, num_envs=n)
    ret_t, len_t = Tracker(n), Tracker(n)
    cur_r, cur_l = torch.zeros(n), torch.zeros(n)
    obs = env.reset()
    for _ in range(env.max_episode_length):
        x = (obs - states[0]) / torch.sqrt(states[1] + states[2]) if cfg.algo.obs_norm else obs
        obs, reward, done, _ = env.step(policy(x))
        cur_r += reward; cur_l += 1
        idx = torch.where(done)[0]
        ret_t.update(cur_r[idx]); len_t.update(cur_l[idx])
        cur_r[idx] = 0; cur_l[idx] = 0
    return {"eval/return": ret_t.mean(), "eval/episode_length": len_t.mean()}


def test_override_of_a_missing_key_fails_like_hydra_struct_mode():
    """A typo in an override must not train a default silently (the reference composes with Hydra, whose struct mode refuses
    `key=value` for a key the composed config lacks): `key=` overrides, `+key=` adds, `++key=` does either."""
    from pql_amd.utils.cfg import load_cfg
    with pytest.raises(KeyError, match="Could not override 'algo.critic.hidden_layers'"):
        load_cfg(["algo.critic.hidden_layers=[512,512,256]"])
    with pytest.raises(KeyError, match="Could not override 'algo.update_times'"):   # a DDPG/SAC key, absent from the PQL group
        load_cfg(["algo.update_times=4"])
    assert load_cfg(["algo=ddpg_algo", "algo.update_times=4"]).algo.update_times == 4
    with pytest.raises(KeyError, match="Could not append 'algo.batch_size'"):
        load_cfg(["+algo.batch_size=64"])
    cfg = load_cfg(["+algo.my_note=7", "++algo.batch_size=64", "++algo.other.note=x", "algo.hidden_layers=[512,512,256]"])
    assert (cfg.algo.my_note, cfg.algo.batch_size, cfg.algo.other.note, list(cfg.algo.hidden_layers)) == (7, 64, "x", [512, 512, 256])


def test_evaluator_in_process_engine(tmp_path):
    """Cooperative evaluator: same numbers as the reference's rollout loop, results appear after enough polls, the best
    model is kept, and the stop criterion follows evaluator.py:34-38."""
    from types import SimpleNamespace
    from pql_amd.utils.cfg import load_cfg
    from pql_amd.utils.evaluator import Evaluator
    cfg = load_cfg(["task.name=Toy", "task.episode_length=20", "eval_num_envs=7", "device=cpu", "eval_steps_per_poll=6", "max_step=1000"])
    A = 2
    policy = lambda x: torch.tanh(x[:, :A] * 0.5)   # noqa: E731
    mean, var = torch.linspace(-1, 1, 8), torch.linspace(0.5, 2, 8)
    norm = SimpleNamespace(get_states=lambda device=None: (mean, var, 1e-4))
    ev = Evaluator(cfg, wandb_run=SimpleNamespace(dir=str(tmp_path)))
    assert not ev.parent.poll()
    ev.eval_policy(policy, None, step=5, normalizer=norm)
    polls = 0
    while not ev.parent.poll():
        polls += 1
        assert polls < 10
    assert polls == 3            # 20 steps at 6 per poll: the 4th poll enqueues the last 2 and finds the result
    got = ev.parent.recv()
    want = _reference_style_eval(cfg, policy, (mean, var, 1e-4))
    assert got.keys() == want.keys()
    for k in want:
        assert abs(got[k] - want[k]) <= 1e-9 * max(1.0, abs(want[k])), (k, got[k], want[k])
    ckpt = torch.load(tmp_path / "model.pth", weights_only=True)
    assert torch.equal(ckpt["obs_rms"][0], mean) and ckpt["actor"] == {} and ckpt["critic"] == {}
    # a worse policy later does not overwrite the best checkpoint; recv() on an unfinished job drives it to the end
    (tmp_path / "model.pth").unlink()
    ev.eval_policy(lambda x: torch.full((x.shape[0], A), 1.0), None, step=6, normalizer=norm)   # action penalty -> lower return
    worse = ev.parent.recv()
    assert worse["eval/return"] < got["eval/return"] and not (tmp_path / "model.pth").exists()
    assert ev.parent.pending() == 0
    assert not ev.check_if_should_stop(1000) and ev.check_if_should_stop(1001)
    cfg2 = load_cfg(["device=cpu", "max_time=0", "task.name=Toy", "eval_num_envs=2"])
    ev2 = Evaluator(cfg2, enabled=False)
    assert ev2.check_if_should_stop(0) and not ev2.parent.poll()


def test_evaluator_module_spec_round_trip_is_plain_data():
    """Subprocess mode ships (class name, kwargs, CPU state_dict); the spec must survive pickle and name every argument the
    constructor needs."""
    import inspect, pickle
    import pql_amd.models.mlp as M
    from pql_amd.utils.evaluator import module_to_spec
    for mod in (M.TanhMLPPolicy((8,), 2, hidden_layers=[64, 32]), M.DoubleQ((8,), 2, hidden_layers=[64, 32]),
                M.DistributionalDoubleQ((8,), 2, num_atoms=11, device="cpu", hidden_layers=[32, 32])):
        spec = pickle.loads(pickle.dumps(module_to_spec(mod)))
        assert spec["cls"] == type(mod).__name__
        params = inspect.signature(type(mod).__init__).parameters
        assert set(spec["kwargs"]) <= set(params)
        clone = type(mod)(**spec["kwargs"])
        clone.load_state_dict(spec["state"])
        assert torch.equal(clone.arena.data, mod.arena.data)


def test_c_abi_reports_argument_errors_as_codes():
    """Error behaviour of the boundary (include/pqlk.h): bad arguments come back as positive PQLK_E_* codes before anything
    is launched -- no exception across the ABI, no abort, no launch (so this runs without a GPU).  0x1000 stands in for a
    device pointer: argument validation never dereferences it."""
    import ctypes as C
    from pql_amd import _lib as L
    E_NULL, E_SHAPE, E_ALIGN, E_UNSUPPORTED = 1, 2, 4, 5
    P = C.c_void_p(0x1000)
    d = L.mlp_desc([8, 64, 1], 2)
    lib = L.lib
    # MLP forward / backward
    assert lib.pqlk_mlp_forward(None, P, None, 1, P, 32, 4, L.ACT_NONE, None, 0.0, 0.0, P, None, 0, None) == E_NULL
    assert lib.pqlk_mlp_forward(C.byref(d), None, None, 1, P, 32, 4, L.ACT_NONE, None, 0.0, 0.0, P, None, 0, None) == E_NULL
    assert lib.pqlk_mlp_forward(C.byref(d), P, None, 1, P, 32, 0, L.ACT_NONE, None, 0.0, 0.0, P, None, 0, None) == E_SHAPE
    assert lib.pqlk_mlp_forward(C.byref(d), P, None, 1, P, 20, 4, L.ACT_NONE, None, 0.0, 0.0, P, None, 0, None) == E_ALIGN      # ldx % 32
    assert lib.pqlk_mlp_forward(C.byref(d), C.c_void_p(0x1004), None, 1, P, 32, 4, L.ACT_NONE, None, 0.0, 0.0, P, None, 0, None) == E_ALIGN
    assert lib.pqlk_mlp_forward(C.byref(d), P, None, 1, P, 32, 4, 99, None, 0.0, 0.0, P, None, 0, None) == E_UNSUPPORTED        # activation id
    assert lib.pqlk_mlp_forward(C.byref(d), P, None, 1, P, 32, 4, L.ACT_TANH_NOISE, None, 0.5, 0.2, P, None, 0, None) == E_NULL  # noise needs a draw
    d3 = L.mlp_desc([8, 64, 1], 3)
    assert lib.pqlk_mlp_forward(C.byref(d3), P, None, 1, P, 32, 4, L.ACT_NONE, None, 0.0, 0.0, P, None, 0, None) == E_UNSUPPORTED  # n_nets > 2
    assert lib.pqlk_mlp_backward(C.byref(d), P, P, 32, 4, P, None, P, 1, None, 0, 0, 0, None, 0, P, 1 << 20, None) == E_NULL      # dy
    # replay / n-step
    ring = L.PqlReplayDesc(0x1000, 100, 8, 2, int(lib.pqlk_replay_rec_ld(8, 2)), 0)
    assert lib.pqlk_replay_gather(C.byref(ring), None, 4, P, P, P, P, P, None) == E_NULL
    assert lib.pqlk_replay_gather(None, P, 4, P, P, P, P, P, None) == E_NULL
    assert lib.pqlk_replay_insert(C.byref(ring), 98, 4, P, 8, P, 2, P, 1, P, 8, P, 1, None) != 0      # rows 98..101 of a 100-row ring
    # losses / optimiser
    assert lib.pqlk_td_mse_loss(P, P, 32, P, P, 0.97, 0, P, P, None, 1, P, None) == E_SHAPE
    assert lib.pqlk_clip_adamw_polyak(P, P, P, P, None, 0, 1.0, 0.5, 5e-4, 0.9, 0.999, 1e-8, 1e-2, 0.05, P, None, P, None) == E_SHAPE
    assert lib.pqlk_clip_adamw_polyak(P, None, P, P, None, 64, 1.0, 0.5, 5e-4, 0.9, 0.999, 1e-8, 1e-2, 0.05, P, None, P, None) == E_NULL
    # SAC head, BatchNorm block, synthetic env
    assert lib.pqlk_sg_head_forward(P, 32, P, 4, 65, P, 65, P, None) == E_SHAPE          # more than 64 actions
    assert lib.pqlk_sg_head_forward(P, 8, P, 4, 8, P, 8, P, None) == E_SHAPE             # ld_y < 2 A
    assert lib.pqlk_sg_head_backward(P, 32, None, P, 8, P, 8, None, 1.0, 4, 8, P, None) == E_NULL
    assert lib.pqlk_bn_elu_forward(P, 64, 1, 64, P, P, P, P, 1e-5, 1, 0.1, P, P, P, None) == E_SHAPE   # one row has no variance
    assert lib.pqlk_bn_elu_forward(P, 64, 8, 64, None, None, P, P, 1e-5, 1, 0.1, P, P, P, None) == E_NULL
    assert lib.pqlk_bn_elu_backward(P, P, P, 32, 8, 64, P, P, P, 1e-5, P, None, None, P, None) == E_SHAPE  # ld < cols
    assert lib.pqlk_synth_env_step(0, 8, 2, 1, 0, 1, 0.01, P, P, P, P, None) == E_SHAPE
    # round-2 entry points: rollout bookkeeping, fused learner tail, min-net DPG backward
    roll = lambda n, t, obs: lib.pqlk_rollout_step(n, 8, 2, 4, t, obs, P, P, P, P, None, P, P, P, P, P, P, P, P, P, P, P, 100, None)  # noqa: E731
    assert roll(16, 0, None) == E_NULL
    assert roll(0, 0, P) == E_SHAPE
    assert roll(16, 4, P) == E_SHAPE                                                      # t must be < horizon
    assert roll(16, 0, C.c_void_p(0x1004)) == E_ALIGN                                     # obs_dim % 4 == 0: 16-B rows
    WS = 6                                                                                # PQLK_E_WORKSPACE
    assert lib.pqlk_mlp_backward_norm(C.byref(d), P, P, 32, 4, P, P, None, 1, None, 0, 0, 0, None, 0, P, 1 << 20, P, P, None) == E_NULL  # grads
    assert lib.pqlk_mlp_backward_norm(C.byref(d), P, P, 32, 4, P, P, P, 1, None, 0, 0, 0, None, 0, P, 1 << 20, None, P, None) == E_NULL  # sumsq_part
    assert lib.pqlk_dpg_critic_backward(C.byref(d), P, P, 32, 4, P, P, P, 32, 6, 2, P, 32, P, P, 8, None) == WS     # workspace too small
    assert lib.pqlk_dpg_backward_ws_floats(C.byref(d), 0) == 0
    assert lib.pqlk_dpg_loss_owner(None, 32, 1, None, 4, P, P, None, 1, P, P, None) == E_NULL
    assert lib.pqlk_dpg_loss_owner(P, 20, 1, None, 4, P, P, None, 1, P, P, None) == E_ALIGN                        # ld % 32
    assert lib.pqlk_adamw_polyak_fused(None, P, P, P, P, P, None, None, 1.0, 0.5, 5e-4, 0.9, 0.999, 1e-8, 1e-2, 0.05, P, None, P, 8,
                                       None, 0, 1.0, None, 0, None) == E_NULL
    assert lib.pqlk_loss_parts(8192, 1) > 0 and lib.pqlk_mlp_norm_parts(C.byref(d)) > 0
    # round-3 entry points: TD-fused critic backward, Philox draws
    E_RANGE = 3
    assert lib.pqlk_mlp_backward_td(C.byref(d), P, P, 32, 4, P, None, P, P, 0.97, P, P, 1, P, 1 << 20, None, None, None) == E_NULL   # target stash
    assert lib.pqlk_mlp_backward_td(C.byref(d), P, P, 32, 4, P, P, P, P, 0.97, P, P, 1, P, 1 << 20, P, None, None) == E_NULL        # sumsq without step
    d1 = L.mlp_desc([8, 64, 1], 1)
    assert lib.pqlk_mlp_backward_td(C.byref(d1), P, P, 32, 4, P, P, P, P, 0.97, P, P, 1, P, 1 << 20, None, None, None) == E_UNSUPPORTED  # one net
    assert lib.pqlk_td_head_loss_parts(C.byref(d), 8192) == 512 and lib.pqlk_td_head_loss_parts(C.byref(d1), 8192) == 0
    assert lib.pqlk_td_head_loss_parts(C.byref(L.mlp_desc([8, 64, 51], 2)), 8192) == 0                                    # C51 heads: own loss kernel
    # the head's backward inside the critic's forward launch: which layouts take it (no GPU call: eligibility + argument checks)
    parts = lambda dims, b, nets=2: lib.pqlk_td_forward_loss_parts(C.byref(L.mlp_desc(dims, nets)), b)   # noqa: E731
    assert parts([104, 512, 512, 256, 1], 8192) == 256        # cfg #2: 128 tiles of 64 rows x 2 nets
    assert parts([104, 512, 256, 128, 1], 1000) == 64         # reference default widths, ragged batch: 32 tiles of 32 rows x 2
    assert parts([129, 1024, 512, 1], 300) == 20              # 1024-wide layer: 32-row tiles
    assert parts([104, 512, 512, 512, 1], 8192) == 0          # no 256 free LDS columns beside the last hidden layer
    assert parts([104, 256, 256, 1], 96) == 0 and parts([104, 512, 256, 1], 512, nets=1) == 0 and parts([229, 512, 256, 51], 512) == 0
    assert parts([48, 100, 36, 1], 64) == 0                   # widths not multiples of 32: no fused stack
    dq = L.mlp_desc([104, 512, 512, 256, 1], 2)
    ft, tail = lib.pqlk_mlp_forward_td, lib.pqlk_mlp_backward_td_tail
    assert ft(C.byref(dq), P, None, P, 128, 64, P, P, P, P, 0.97, P, P, 1 << 40, 16, None) == E_NULL       # needs the packed copy
    assert ft(C.byref(dq), P, P, P, 100, 64, P, P, P, P, 0.97, P, P, 1 << 40, 16, None) == E_ALIGN         # ldx % 32
    assert ft(C.byref(dq), P, P, P, 128, 64, P, P, P, P, 0.97, P, P, 1024, 16, None) == WS                 # backward workspace too small
    assert ft(C.byref(d1), P, P, P, 32, 64, P, P, P, P, 0.97, P, P, 1 << 40, 16, None) == E_UNSUPPORTED    # one net
    assert tail(C.byref(dq), P, P, 128, 64, P, None, 16, P, 1 << 40, None, None, None) == E_NULL           # no gradient arena
    assert tail(C.byref(dq), P, P, 128, 64, P, P, 16, P, 1 << 40, P, None, None) == E_NULL                 # sumsq without step
    assert tail(C.byref(d1), P, P, 32, 64, P, P, 16, P, 1 << 40, None, None, None) == E_UNSUPPORTED
    # data-parallel buckets: layer ranges are checked before anything is launched
    bl = lib.pqlk_mlp_backward_layers
    assert bl(C.byref(d), P, P, 32, 4, P, P, None, None, None, 0.97, None, P, 1, P, 1 << 20, 2, 0, None) == E_RANGE      # 2 layers: 0..1
    assert bl(C.byref(d), P, P, 32, 4, P, P, None, None, None, 0.97, None, P, 1, P, 1 << 20, 0, 1, None) == E_RANGE      # hi < lo
    assert bl(C.byref(d), P, P, 32, 4, P, P, None, None, None, 0.97, None, None, 1, P, 1 << 20, 1, 0, None) == E_NULL    # no gradient arena
    assert bl(C.byref(d), P, P, 32, 4, P, P, P, None, None, 0.97, None, P, 1, P, 1 << 20, 1, 0, None) == E_NULL          # TD inputs: all four or none
    assert bl(C.byref(d), P, P, 32, 4, P, None, None, None, None, 0.97, None, P, 1, P, 1 << 20, 1, 1, None) == E_NULL    # the head's call needs dy
    assert lib.pqlk_philox_draws(1, 0, 0, None, 100, None, 8, None, 0, 1, 1, None) == E_NULL
    assert lib.pqlk_philox_draws(1, 0, 0, None, 1 << 28, P, 8, None, 0, 1, 1, None) == E_RANGE       # torch draws 64-bit values from 2^28 on
    assert lib.pqlk_philox_draws(1, 2, 0, None, 100, P, 8, None, 0, 1, 1, None) == E_ALIGN          # offsets advance in whole Philox blocks
    assert lib.pqlk_philox_draws(1, 0, 0, None, 100, P, 0, None, 0, 1, 1, None) == E_SHAPE
    # torch's calc_execution_policy on a 256-CU device: 256 * min(2048, ceil(n / 256)) threads, 4 values per thread and round
    for n, inc in ((1, 4), (8192, 4), (8192 * 16, 4), (2048 * 256, 4), (2048 * 256 * 4, 4), (2048 * 256 * 4 + 1, 8), (32768 * 21, 4)):
        assert lib.pqlk_philox_increment(n) == inc, n
    assert lib.pqlk_philox_increment(0) == 0
    # round-4 entry points: the P-learner's fused backward (eligibility + argument checks: nothing is launched), the output-only
    # forward, the critic forward with a compact Q copy and a second input source
    crit, act = L.mlp_desc([104, 512, 512, 256, 1], 2), L.mlp_desc([88, 512, 512, 256, 16], 1)
    ok = lambda c, a, b=8192: lib.pqlk_dpg_fused_ok(C.byref(c), C.byref(a), b)   # noqa: E731
    assert ok(crit, act) == 1 and ok(crit, act, 256) == 1
    assert ok(L.mlp_desc([28, 512, 256, 128, 1], 2), L.mlp_desc([8, 512, 256, 128, 2], 1), 64) == 1       # the toy / golden-trace shapes
    assert ok(crit, L.mlp_desc([108, 512, 512, 256, 21], 1)) == 0      # Humanoid: 21 actions > 16 -> the separate launches
    assert ok(L.mlp_desc([104, 512, 512, 256, 51], 2), act) == 0       # C51 heads: the minimum is over expectations
    assert ok(L.mlp_desc([104, 512, 320, 256, 1], 2), act) == 0        # 320: no whole 128-column tiles in the compact dX chain
    assert ok(crit, L.mlp_desc([88, 512, 512, 96, 16], 1)) == 0        # actor head over 96 inputs: neither 128 nor 256
    assert ok(crit, act, 200000) == 0 and ok(crit, act, 0) == 0 and ok(crit, crit) == 0
    assert lib.pqlk_dpg_fused_loss_parts() == 32 and lib.pqlk_dpg_fused_head_parts(8192) == 512 and lib.pqlk_dpg_fused_head_parts(1000) == 64
    assert lib.pqlk_dpg_fused_mn_offset(C.byref(crit), 8192) == 2 * 16384 * 512 + 16384 and lib.pqlk_dpg_fused_mn_offset(None, 8192) == -1
    assert lib.pqlk_dpg_backward_ws_floats(C.byref(crit), 8192) >= lib.pqlk_dpg_fused_mn_offset(C.byref(crit), 8192) + 64 + 16384   # mn + tie0 fit
    fq = lib.pqlk_mlp_forward_qc
    assert fq(C.byref(crit), P, None, 1, P, 128, None, 0, 0, 64, P, P, None) == E_NULL                     # needs the packed copy
    assert fq(C.byref(crit), P, P, 1, P, 128, None, 0, 0, 64, P, None, None) == E_NULL                     # ... and somewhere to put qc
    assert fq(C.byref(crit), P, P, 1, P, 100, None, 0, 0, 64, P, P, None) == E_ALIGN                       # one source: ldx % 32
    assert fq(C.byref(crit), P, P, 1, P, 96, P, 32, 90, 64, P, P, None) == E_RANGE                         # split off a 16-byte boundary
    assert fq(C.byref(crit), P, P, 1, P, 96, P, 8, 88, 64, P, P, None) == E_ALIGN                          # second source narrower than the action
    assert fq(C.byref(L.mlp_desc([104, 512, 512, 256, 51], 2)), P, P, 1, P, 128, None, 0, 0, 64, P, P, None) == E_UNSUPPORTED
    bf = lambda c, a, wsf=1 << 40, awsf=1 << 40, qc=P: lib.pqlk_dpg_backward_fused(   # noqa: E731
        C.byref(c), P, None, 0, 8192, P, qc, P, 32, 88, P, 32, P, P, wsf, C.byref(a), P, P, P, awsf, 16, None)
    assert bf(crit, act, qc=None) == E_NULL
    assert bf(crit, L.mlp_desc([108, 512, 512, 256, 21], 1)) == E_UNSUPPORTED
    assert bf(crit, act, wsf=1024) == WS and bf(crit, act, awsf=1024) == WS
    bt = lib.pqlk_mlp_backward_tail
    assert bt(C.byref(act), P, P, 96, 8192, P, None, 16, P, 1 << 40, None, None, 512, None, None) == E_NULL            # no gradient arena
    assert bt(C.byref(act), P, P, 96, 8192, P, P, 16, P, 1 << 40, P, None, 512, None, None) == E_NULL                  # sumsq without step
    assert bt(C.byref(act), P, P, 96, 8192, P, P, 16, P, 1 << 40, None, None, 0, None, None) == E_UNSUPPORTED           # no head partials
    assert bt(C.byref(act), P, P, 96, 8192, P, P, 16, P, 1 << 40, None, None, 1 << 20, None, None) == WS                # more partials than the workspace holds
    assert lib.pqlk_mlp_forward(C.byref(d), P, None, 3, P, 32, 4, L.ACT_NONE, None, 0.0, 0.0, P, None, 0, None) == E_RANGE         # stash_all in {0, 1, 2}
    assert lib.pqlk_mlp_forward(C.byref(d), P, None, 2, P, 32, 4, L.ACT_NONE, None, 0.0, 0.0, P, None, 0, None) == E_UNSUPPORTED   # output-only: fused path only
    for code in (E_NULL, E_SHAPE, 3, E_ALIGN, E_UNSUPPORTED, 6):
        assert len(lib.pqlk_strerror(code)) > 2


# --------------------------------------------------------------------------- the `pql` name
def test_pql_alias_package_resolves_to_the_same_modules():
    """north_star: "keeps the pql.algo / scripts/train_pql.py entry points".  Every name SURVEY 8(b) lists must import
    from `pql.*` and be the SAME object as under `pql_amd.*` (one class, two names)."""
    import importlib
    import pql
    import pql_amd
    assert pql.LIB_PATH == pql_amd.LIB_PATH and (pql.LIB_PATH / "cfg" / "default.yaml").exists()
    wanted = {
        "pql.algo.pql_actor": ["PQLActor"],
        "pql.algo.pql_v_learner": ["PQLVLearner", "asyn_v_learner"],
        "pql.algo.pql_p_learner": ["PQLPLearner", "asyn_p_learner"],
        "pql.algo.ddpg": ["AgentDDPG"], "pql.algo.sac": ["AgentSAC"], "pql.algo.crossQ": ["AgentCrossQ"],
        "pql.replay.simple_replay": ["ReplayBuffer", "create_buffer"],
        "pql.replay.nstep_replay": ["NStepReplay"],
        "pql.models.mlp": ["MLPNet", "TanhMLPPolicy", "DoubleQ", "DistributionalDoubleQ", "TanhDiagGaussianMLPPolicy"],
        "pql.utils.common": ["Tracker", "normalize", "load_class_from_path", "set_random_seed", "preprocess_cfg",
                             "capture_keyboard_interrupt", "handle_timeout"],
        "pql.utils.torch_util": ["RunningMeanStd", "soft_update"],
        "pql.utils.noise": ["add_normal_noise", "add_mixed_normal_noise"],
        "pql.utils.distl_util": ["projection"],
        "pql.utils.schedule_util": ["LinearSchedule", "ExponentialSchedule"],
        "pql.utils.evaluator": ["Evaluator"],
        "pql.utils.model_util": ["save_model", "load_model"],
        "pql.utils.isaacgym_util": ["create_task_env"],
    }
    for mod_name, names in wanted.items():
        mod = importlib.import_module(mod_name)
        real = importlib.import_module(mod.__name__)
        assert mod is real and mod.__name__.startswith("pql_amd."), mod_name
        for n in names:
            assert hasattr(mod, n), f"{mod_name}.{n}"
    from pql.models import model_name_to_path
    from pql.algo import alg_name_to_path
    assert {"DoubleQ", "DistributionalDoubleQ", "TanhMLPPolicy"} <= set(model_name_to_path)
    assert "AgentDDPG" in alg_name_to_path
    with pytest.raises(ModuleNotFoundError):
        importlib.import_module("pql.no_such_module")


def test_reference_cli_task_names_compose():
    """`task=<IsaacGymEnvs name>` (pql/cfg/default.yaml:7-9) composes onto the synthetic env with that task's shapes;
    the fast path (graph + own streams) is the default."""
    from pql_amd.envs.synthetic import create_task_env
    from pql_amd.utils.cfg import load_cfg
    for name, shape in (("AllegroHand", (88, 16)), ("ShadowHand", (211, 20)), ("Humanoid", (108, 21)), ("Ant", (60, 8))):
        cfg = load_cfg([f"task={name}", "device=cpu", "num_envs=4"])
        assert cfg.task.name == name and cfg.algo.graph is True and cfg.algo.streams is True
        env = create_task_env(cfg)
        assert (env.observation_space.shape[0], env.action_space.shape[0]) == shape
    assert load_cfg([]).algo.async_learners is False
    with pytest.raises(ValueError, match="AlegroHand"):   # a typo fails at config load (Hydra: missing config), not later
        load_cfg(["task=AlegroHand", "device=cpu"])


# --------------------------------------------------------------------------- a25 ratio controller
def test_ratio_controller_matches_the_reference_law():
    from oracle.pql_ref_cpu import ratio_control_ref
    from pql_amd.utils.ratio_control import RatioController
    rng = np.random.default_rng(0)
    for trial in range(4):
        n = 400
        dt = rng.uniform(0.5e-3, 3e-3, n)
        t = np.cumsum(dt)
        cri = np.cumsum(rng.integers(0 if trial == 3 else 1, 14, n))      # trial 3: windows where a counter stalls
        act = np.cumsum(rng.integers(0 if trial == 3 else 1, 7, n))
        if trial == 3:
            cri[:15] = 0; act[:15] = 0
        obs = [(float(a), int(b), int(c)) for a, b, c in zip(t, cri, act)]
        want = ratio_control_ref(obs, 8, 2)
        now = [0.0]
        ctl = RatioController(8, 2, clock=lambda: now[0])
        got = []
        for (t_i, c, a) in obs:
            now[0] = t_i
            got.append(ctl.observe(c, a))
        np.testing.assert_allclose(np.array(got, dtype=np.float64), np.array(want, dtype=np.float64), rtol=0, atol=0)


def test_ratio_controller_closed_loop_reaches_design_ratios():
    """Closed loop in virtual time: three components with fixed unit costs, learners sleeping what they are told.  The law is
    an integrating controller over a 100-iteration window, so it needs a few thousand iterations (as in the reference)."""
    from pql_amd.utils.ratio_control import RatioController
    for ts, tv, tp in ((1e-3, 0.15e-3, 0.15e-3), (0.5e-3, 0.7e-3, 0.6e-3), (4e-3, 0.1e-3, 0.1e-3)):
        now = [0.0]
        ctl = RatioController(8, 2, clock=lambda: now[0])
        v_t = p_t = 0.0
        v_n = p_n = 0
        cw = aw = 0.0
        hist = []
        for it in range(3000):
            end = now[0] + ts
            while v_t + tv + cw <= end:
                v_t += tv + cw; v_n += 1
            while p_t + tp + aw <= end:
                p_t += tp + aw; p_n += 1
            now[0] = end
            sw, cw, aw = ctl.observe(v_n, p_n)
            now[0] += sw
            hist.append((it + 1, v_n, p_n))
        a, b = hist[len(hist) // 2], hist[-1]
        assert abs((b[1] - a[1]) / (b[0] - a[0]) - 8) < 0.8, (ts, tv, tp)
        assert abs((b[1] - a[1]) / (b[2] - a[2]) - 2) < 0.1, (ts, tv, tp)


# --------------------------------------------------------------------------- trackers
def test_device_tracker_keeps_the_last_max_len_values_like_the_reference_deque():
    """More finished episodes in one step than the window holds (tracker_len 100 vs 4096 envs): deque.extend keeps the
    LAST max_len values; the scatter form must keep exactly those (and be deterministic)."""
    import torch
    from pql_amd.algo.pql_actor import DeviceTracker
    from pql_amd.utils.common import Tracker
    rng = np.random.default_rng(3)
    dt, ref = DeviceTracker(10, "cpu"), Tracker(10)
    for step in range(12):
        n = 64
        vals = torch.from_numpy(rng.normal(size=n).astype(np.float32))
        p = (0.02, 0.5, 0.9, 0.0)[step % 4]
        mask = torch.from_numpy(rng.random(n) < p)
        dt.update(vals, mask)
        ref.update(vals[mask])
        assert sorted(dt.ring[:10].tolist()) == pytest.approx(sorted(float(x) for x in ref.moving_average))
        assert dt.mean() == pytest.approx(float(ref.mean()), rel=1e-6, abs=1e-7)


def test_bench_refuses_more_gpus_than_visible():
    """`python bench.py --gpus N` from a bare shell starts N ranks itself -- and fails loudly, before any GPU call, when the
    box has fewer devices (it used to benchmark one GPU and print n_gpus: 1)."""
    import subprocess, sys, os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    import torch
    n = torch.cuda.device_count() + 2
    for extra in ([], ["--layout", "split2"] if n == 2 else []):
        r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", str(n), *extra], env=env,
                           capture_output=True, text=True, timeout=300)
        assert r.returncode != 0 and "GPU(s) visible" in (r.stderr + r.stdout)


def test_no_kernel_of_the_library_goes_through_scratch():
    """Every kernel's own metadata (tools/kernel_resources.py): no spilled VGPR, no private segment.  A spilling kernel stays
    correct and green everywhere else; round 3's k_mlp_fwd_fused<1,4> (hidden widths > 512) carried 59 spilled registers."""
    kr = load_script("tools/kernel_resources.py", "kernel_resources")
    if not os.path.exists(f"{kr.LLVM}/llvm-readelf"):
        pytest.skip("no llvm-readelf")
    res = kr.resources()
    assert len(res) >= 60
    for want in ("k_mlp_fwd_fused<1, 2, false>", "k_mlp_fwd_fused<2, 2, false>", "k_mlp_fwd_fused<1, 4, false>", "k_mlp_fwd_fused<2, 2, true>",
                 "k_replay_gather_fast<true, 2>", "k_replay_gather_obs<true, 4>", "k_dpg_minnet_head", "k_dx_slice<16, 16>", "k_adamw"):
        assert any(want in k for k in res), want
    bad = kr.spilling(res)
    assert not bad, {k: (v.get("vgpr_spill_count"), v.get("private_segment_fixed_size")) for k, v in bad.items()}
    for k, v in res.items():   # the register file is 512 per SIMD lane: nothing may ask for more than 256 + 256
        assert v.get("vgpr_count", 0) <= 512 and v.get("max_flat_workgroup_size", 0) <= 1024, k


def test_c51_kernels_with_one_atom_per_lane_hold_no_lds_image():
    """The C51 kernels are one template over NJ = atoms per lane.  NJ = 1 (K <= 64) projects with cross-lane shuffles and must not
    allocate the LDS image of the NJ > 1 instances, which would cost the shipped 51-atom path its occupancy: static LDS is
    block_sum_256's four floats, or nothing.  NJ > 1: sizeof(C51Image) * 4 waves (+ those four floats)."""
    kr = load_script("tools/kernel_resources.py", "kernel_resources")
    if not os.path.exists(f"{kr.LLVM}/llvm-readelf"):
        pytest.skip("no llvm-readelf")
    res = kr.resources()
    lds = lambda name: res[f"void {name}"]["group_segment_fixed_size"]  # noqa: E731
    assert lds("k_c51_project<1>") == 0
    assert lds("k_c51_bce<1>") == 16 and lds("k_dpg_dist<1>") == 16
    for nj in (2, 3, 4):
        assert lds(f"k_c51_bce<{nj}>") == 4096 * 4 + 16
        assert lds(f"k_c51_project<{nj}>") == 4096 * 4
        assert lds(f"k_dpg_dist<{nj}>") == 16


def test_gather_kernels_keep_their_counted_waits():
    """The gather kernels are chains of loads and stores on gfx9's one in-order vector-memory counter; what they cost hangs on the
    compiler waiting with COUNTED `s_waitcnt vmcnt(n)`.  Round 4 twice produced a kernel with the same bits and 14 full drains
    (`vmcnt(0)`) instead of 2 -- 23 -> 28-30 us -- by adding a wave-uniform branch, then a template flag and selects, to the
    per-record loop; no parity test can see that.  This counts the drains in the built library (tools/kernel_resources.py)."""
    kr = load_script("tools/kernel_resources.py", "kernel_resources")
    if not os.path.exists(f"{kr.LLVM}/llvm-objdump"):
        pytest.skip("no llvm-objdump")
    drains = kr.full_drains(want=("k_replay_gather_fast<true", "k_replay_gather_obs<true"))
    assert len(drains) == 7, sorted(drains)
    for name, n in drains.items():
        limit = 3 if "gather_fast" in name else 5
        assert n <= limit, f"{name}: {n} full drains of the vector-memory queue (was 2 / 3-5): look at the loop's waits before shipping this"
