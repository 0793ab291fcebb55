"""The critic diagnostics (algo.diag.enabled=True) in the PQL V-learner and in DDPG on the GPU.

Yardsticks: the same learner / agent from the same seed with the key off (the probe must not move a bit of what training writes);
the two entries called by hand on an independent forward of the handed-out weights (bitwise); a float64 torch recomputation from the
state_dict within a forward bound derived below; spies on `L.lib.pqlk_critic_stats` / `pqlk_unit_stats` for when the probe runs; the
training scripts' JSONL logs; the uninterrupted run for a resumed one.  Shapes: O = 8, A = 2, hidden [64, 64], B = 256, 64 envs.
"""
import functools
import json

import numpy as np
import pytest
import torch

import agent_harness as ah
import diag_cases as dc
import learner_harness as lh
import task_cases as tc
from learner_harness import PER, _same_state, _state
from resume_cases import PQL, PQL_KEYS, PQL_TOY, child, same
from support import dev  # noqa: F401

pytestmark = pytest.mark.gpu

O, A, B, K, HID = 8, 2, 256, 4, (64, 64)
ON = "algo.diag.enabled=True"
ENTRIES = ("pqlk_critic_stats", "pqlk_unit_stats")
MODES = {"eager": ("algo.graph=False",), "slot": ("algo.graph=True", "algo.run_graph=False"), "run": ("algo.graph=True",)}
_rows = functools.partial(lh._rows, O, A)


def _cfg(*extra):
    from pql_amd.utils.cfg import load_cfg
    cfg = load_cfg(["algo=pql_algo", "task.name=Toy", f"algo.batch_size={B}", "algo.memory_size=4096", "algo.v_learner_gpu=0",
                    "algo.p_learner_gpu=0", "algo.num_gpus=1", f"algo.prefetch_steps={K}", *extra])
    cfg.algo.hidden_layers = list(HID)
    return cfg


def _learner(*extra, seed=11):
    return lh._learner(lambda: _cfg(*extra), O, A, 600, seed)


def _handoffs(v, actor, norm, n, mode="run", steps=K, keep=None):
    """n times: `steps` gradient steps (`learn_many`: one run graph, per-slot graphs or eager launches, as the mode has it), then a
    hand-off with 64 new rows (what 64 envs deliver).  The learner's construction (learner_harness._learner) was hand-off 1."""
    for h in range(n):
        if steps:
            v.learn_many(steps)
        out = v.update(actor, _rows(64, 100 + h, v.device), norm, 0)
        if keep is not None:
            keep.append(out)


@pytest.fixture
def spies(monkeypatch):
    """Call counters in front of the real entries."""
    from pql_amd import _lib as L
    seen = {n: 0 for n in ENTRIES}
    for name in ENTRIES:
        real = getattr(L.lib, name)

        def spy(*a, _n=name, _real=real):
            seen[_n] += 1
            return _real(*a)
        monkeypatch.setattr(L.lib, name, spy)
    return seen


# =========================================================================== the probe moves no bit of the training state
@pytest.mark.parametrize("mode", list(MODES))
def test_pql_training_state_is_bit_equal_with_diagnostics_on(dev, spies, mode):
    ends = {}
    for name, extra in (("off", ()), ("on", (ON, "algo.diag.every=1"))):
        v, actor, norm = _learner(*MODES[mode], *extra)
        _handoffs(v, actor, norm, 6, mode)
        ends[name] = _state(v)
        if name == "off":
            assert spies == {"pqlk_critic_stats": 0, "pqlk_unit_stats": 0} and v.diagnostics() == {}
    assert spies == {"pqlk_critic_stats": 6, "pqlk_unit_stats": 6 * 2 * len(HID)}
    _same_state(ends["off"], ends["on"])
    assert int(ends["on"]["adam_step"]) == 6 * K and bool(torch.isfinite(ends["on"]["loss_ring"]).all())
    d = v.diagnostics()
    assert d["diag/nonfinite"] == 0 and d["diag/q_min"] <= d["diag/q1_mean"] <= d["diag/q_max"]


@pytest.mark.parametrize("extra", [PER, ("algo.target_dtype=bfloat16",)], ids=["per", "bf16"])
def test_pql_bit_equal_with_prioritized_replay_and_bf16_targets(dev, spies, extra):
    ends = {}
    for name, on in (("off", ()), ("on", (ON, "algo.diag.every=2"))):
        v, actor, norm = _learner(*MODES["run"], *extra, *on)
        _handoffs(v, actor, norm, 6)
        ends[name] = _state(v)
    assert spies["pqlk_critic_stats"] == 3      # the probe did run: hand-offs 2, 4, 6 of 7 (the first built the learner)
    _same_state(ends["off"], ends["on"])


def test_every_counts_handoffs_and_an_idle_handoff_probes_nothing(dev, spies):
    v, actor, norm = _learner(*MODES["run"], ON, "algo.diag.every=3")
    at = []
    for handoff in range(2, 8):      # (hand-off 1 filled the ring when the learner was built: no step before it, no probe)
        before = spies["pqlk_critic_stats"]
        _handoffs(v, actor, norm, 1)
        if spies["pqlk_critic_stats"] != before:
            at.append(handoff)
    assert at == [3, 6] and spies == {"pqlk_critic_stats": 2, "pqlk_unit_stats": 2 * 2 * len(HID)}
    # no step between two hand-offs: hand-off 9 is due, and nothing runs
    _handoffs(v, actor, norm, 1)              # 8
    _handoffs(v, actor, norm, 1, steps=0)     # 9
    assert spies["pqlk_critic_stats"] == 2
    _handoffs(v, actor, norm, 3)              # 10, 11, 12
    assert spies["pqlk_critic_stats"] == 3


# =========================================================================== the values
def _by_hand(v, critic, slot):
    """The two entries on an independent full-stash forward of `critic` (the handed-out snapshot) and of the target on the remembered
    tiles -> the log dict, decoded by the probe's own table."""
    from pql_amd import _lib as L
    from pql_amd.models.mlp import mlp_forward_raw, output_view
    cl, tiles, dv = v.critic.layout, v._ws["slots"][slot], v.device
    acts_c = mlp_forward_raw(cl, critic.arena.data.clone(), tiles["x_sa"].clone(), L.ACT_NONE)
    acts_t = mlp_forward_raw(cl, v.critic_target.arena.data.clone(), tiles["xn_sa"].clone(), L.ACT_NONE)
    out = torch.zeros(10 + 6 * len(HID), device=dv)
    scr = torch.zeros(int(max(L.lib.pqlk_critic_stats_scratch_floats(B, 1), L.lib.pqlk_unit_stats_scratch_floats(max(HID)))), device=dv)
    gamma_n = float(v.cfg.algo.gamma) ** int(v.cfg.algo.nstep)
    L.check(L.lib.pqlk_critic_stats(L.ptr(output_view(cl, acts_c, B)), L.ptr(output_view(cl, acts_t, B)), cl.ld_out, L.HEAD_SCALAR, 1, None, 0.0, 0.0,
                                    L.ptr(tiles["rew"]), L.ptr(tiles["done"]), gamma_n, B, L.ptr(out), L.ptr(scr), L.stream(dv)))
    for net in range(2):
        for layer in range(len(HID)):
            off, ld = cl.act_offset(B, net, layer)
            o = 10 + 3 * (net * len(HID) + layer)
            L.check(L.lib.pqlk_unit_stats(L.ptr(acts_c[off:]), ld, B, HID[layer], float(v.cfg.algo.diag.tau), L.ptr(out[o: o + 3]), L.ptr(scr),
                                          L.stream(dv)))
    torch.cuda.synchronize()
    return v._diag.decode(out.tolist())


def _float64(v, critic, slot):
    """(values, bounds) of the summed statistics from the state_dict in float64, with a running forward bound of the fp32 MLP:
    e_0 = 0 (the tiles are fp32 values); a Linear of n inputs, whatever its summation order: e_z = |W| e_x + (n + 2) U (|W| |x| + |b|);
    ELU is 1-Lipschitz and its expm1 good to a few ulp: e_h = e_z + 4 U |h|.  y = fl(r + fl(c min Q')): c max_i e_Q'_i + 3 U |y| (+ |r|
    rounding inside the 3 U |y| + U |r|).  A mean of B terms adds (log2-deep tree or chain) at most 40 U times the mean magnitude."""
    U = dc.U
    tiles = v._ws["slots"][slot]

    def forward(sd, x):
        x = x[:, : O + A].double().cpu()
        qs, es, hs, ehs = [], [], [], []
        for pre in ("net_q1.net.", "net_q2.net."):
            h, e, n_lin = x, torch.zeros_like(x), len(HID) + 1
            hid, ehid = [], []
            for l in range(n_lin):
                W, b = sd[f"{pre}{2 * l}.weight"].double().cpu(), sd[f"{pre}{2 * l}.bias"].double().cpu()
                z = h @ W.T + b
                e = e @ W.abs().T + (W.shape[1] + 2) * U * (h.abs() @ W.abs().T + b.abs())
                if l < n_lin - 1:
                    h = torch.where(z > 0, z, torch.expm1(z))
                    e = e + 4 * U * h.abs()
                    hid.append(h); ehid.append(e)
                else:
                    h = z
            qs.append(h[:, 0]); es.append(e[:, 0]); hs.append(hid); ehs.append(ehid)
        return qs, es, hs, ehs

    q, eq, hs, ehs = forward(critic.state_dict(), tiles["x_sa"])
    qt, eqt, _, _ = forward(v.critic_target.state_dict(), tiles["xn_sa"])
    r, d = tiles["rew"].double().cpu(), tiles["done"].double().cpu()
    c = (1.0 - d) * dc.f32(float(v.cfg.algo.gamma) ** int(v.cfg.algo.nstep))
    y = r + c * torch.minimum(qt[0], qt[1])
    ey = c * torch.maximum(eqt[0], eqt[1]) + 3 * U * y.abs() + U * r.abs()
    td = torch.maximum((q[0] - y).abs(), (q[1] - y).abs())
    etd = torch.maximum(eq[0], eq[1]) + ey + U * td
    vals, bounds = {}, {}

    def put(key, t, e):
        vals[key] = float(t.mean())
        bounds[key] = dc.SLOP * (float(e.mean()) + 40 * U * float(t.abs().mean()))

    put("diag/q1_mean", q[0], eq[0]); put("diag/q2_mean", q[1], eq[1]); put("diag/target_mean", y, ey)
    put("diag/td_bias", (q[0] + q[1]) / 2 - y, (eq[0] + eq[1]) / 2 + ey + U * ((q[0] + q[1]).abs() / 2 + ((q[0] + q[1]) / 2 - y).abs()))
    put("diag/td_abs_mean", td, etd)
    put("diag/twin_gap", (q[0] - q[1]).abs(), eq[0] + eq[1] + U * (q[0] - q[1]).abs())
    for key, t, e in (("diag/q_min", torch.minimum(q[0], q[1]).min(), torch.maximum(eq[0], eq[1]).max()),
                      ("diag/q_max", torch.maximum(q[0], q[1]).max(), torch.maximum(eq[0], eq[1]).max()), ("diag/td_abs_max", td.max(), etd.max())):
        vals[key], bounds[key] = float(t), dc.SLOP * float(e)
    for l in range(len(HID)):
        # the two nets' means averaged; |h| and the slope (h > 0 ? 1 : h + 1, continuous at 0) are 1-Lipschitz in h
        ab = [h[l].abs().mean(dim=0).mean() for h in hs]
        sl = [torch.where(h[l] > 0, torch.ones_like(h[l]), h[l] + 1).mean() for h in hs]
        eh = sum(float(e[l].mean()) for e in ehs) / 2
        vals[f"diag/act_abs_l{l + 1}"], bounds[f"diag/act_abs_l{l + 1}"] = float(sum(ab)) / 2, dc.SLOP * (eh + 80 * U * float(sum(ab)) / 2)
        vals[f"diag/elu_slope_l{l + 1}"], bounds[f"diag/elu_slope_l{l + 1}"] = float(sum(sl)) / 2, dc.SLOP * (eh + 80 * U * float(sum(sl)) / 2)
    return vals, bounds


@pytest.mark.parametrize("mode", ["eager", "run"])
def test_values_are_the_entries_on_the_handed_out_weights(dev, mode):
    from pql_amd.algo.diag import log_keys
    v, actor, norm = _learner(*MODES[mode], ON, "algo.diag.every=1")
    assert v.diagnostics() == {}
    keep = []
    _handoffs(v, actor, norm, 3, mode, keep=keep)
    v.synchronize()
    torch.cuda.synchronize()
    got = v.diagnostics()
    assert list(got) == log_keys(len(HID))
    critic = keep[-1][0]                                   # the snapshot the last hand-off published
    assert torch.equal(critic.arena.data, v.critic.arena.data)
    slot = K - 1 if v._ahead is not None else 0            # the tiles of the last step before that hand-off
    want = _by_hand(v, critic, slot)
    assert {k: np.float32(x).tobytes() for k, x in got.items()} == {k: np.float32(x).tobytes() for k, x in want.items()}, (got, want)
    vals, bounds = _float64(v, v.critic, slot)
    for key in vals:
        print(f"{key}: {got[key]:.9g} vs float64 {vals[key]:.9g}  |err| {abs(got[key] - vals[key]):.2e}  bound {bounds[key]:.2e}")
        assert abs(got[key] - vals[key]) <= bounds[key], key
    assert got["diag/nonfinite"] == 0 and 0 <= got["diag/dormant_l1"] <= 1 and 0 < got["diag/elu_slope_l2"] <= 1


# =========================================================================== DDPG, every critic class it accepts
DDPG_SHAPE = ["task=pointmass", f"task.obs_dim={O}", f"task.act_dim={A}", "num_envs=64", f"algo.batch_size={B}", "algo.memory_size=1024",
              f"algo.hidden_layers=[{HID[0]},{HID[1]}]", "algo.update_times=2"]
CRITICS = {"DoubleQ": ((), 2), "DoubleQLayerNorm": (("algo.cri_class=DoubleQLayerNorm",), 2),
           "DoubleQDropoutLayerNorm": (("algo.cri_class=DoubleQDropoutLayerNorm",), 2),
           "DoubleQBroNet": (("algo.cri_class=DoubleQBroNet", "algo.critic_width=64", "algo.critic_blocks=1"), 2),
           "QuantileDoubleQ": (("algo.cri_class=QuantileDoubleQ",), 2), "hl_gauss": (("algo.distl=True", "algo.distl_loss=hl_gauss"), 2)}


@pytest.mark.parametrize("name", list(CRITICS))
def test_ddpg_training_state_is_bit_equal_and_logs_the_values(dev, spies, name):
    from pql_amd.algo.diag import log_keys
    extra, layers = CRITICS[name]
    ends, logs = {}, {}
    for which, on in (("off", ()), ("on", (ON, "algo.diag.every=2"))):
        agent, memory = ah._agent("ddpg_algo", *extra, *on, shape=DDPG_SHAPE)
        for _ in range(4):
            logs[which] = agent.update_net(memory)
        ends[which] = ah._state(agent)
        if hasattr(agent.critic, "drop_calls"):
            ends[which]["drop_calls"] = torch.tensor([agent.critic.drop_calls, agent.critic_target.drop_calls])
        if which == "off":
            assert spies["pqlk_critic_stats"] == 0 and not any(k.startswith("diag/") for k in logs["off"])
    assert spies == {"pqlk_critic_stats": 2, "pqlk_unit_stats": 2 * 2 * layers}      # update_net calls 2 and 4
    assert set(ends["off"]) == set(ends["on"])
    for k in ends["off"]:
        assert torch.equal(ends["off"][k], ends["on"][k]), k
    d = {k: x for k, x in logs["on"].items() if k.startswith("diag/")}
    assert list(d) == log_keys(layers)
    assert all(np.isfinite(x) for x in d.values()) and d["diag/nonfinite"] == 0 and d["diag/q_min"] <= d["diag/q1_mean"] <= d["diag/q_max"]
    rest = {k: x for k, x in logs["on"].items() if k not in d}
    assert list(rest) == list(logs["off"]) and all(np.array_equal(rest[k], logs["off"][k], equal_nan=True) for k in rest)


# =========================================================================== the training scripts
SMALL = ["num_envs=64", f"algo.batch_size={B}", "algo.hidden_layers=[64, 64]", "algo.memory_size=20000", "task.episode_length=16"]


def _jsonl(path):
    return [json.loads(line) for line in open(path)]


def _check_rows(rows, layers, first_event):
    from pql_amd.algo.diag import log_keys
    with_diag = [r for r in rows if any(k.startswith("diag/") for k in r)]
    assert with_diag and with_diag == rows[len(rows) - len(with_diag):]       # once they appear they are in every later row
    assert len(rows) - len(with_diag) <= first_event
    for r in with_diag:
        assert set(log_keys(layers)) <= set(r)
        assert all(np.isfinite(r[k]) for k in log_keys(layers)) and r["diag/nonfinite"] == 0
        assert r["diag/q_min"] <= r["diag/q1_mean"] <= r["diag/q_max"]


def test_train_pql_logs_the_diag_columns(tmp_path):
    """scripts/train_pql.py on SwingUp for 48 iterations, a probe every 4th hand-off: every logged row after the first probe has
    landed carries all diag/* keys; with the key off no row carries any."""
    tp = tc.load_script("scripts/train_pql.py", "train_pql_diag")
    from pql_amd.utils.cfg import load_cfg
    for on in (True, False):
        log = tmp_path / f"log_{on}.jsonl"
        cfg = load_cfg(["task=swingup", *SMALL, "algo.num_gpus=1", f"max_step={64 * (32 + 48) - 1}", f"logging.jsonl={log}", "eval_num_envs=32",
                        "algo.eval_freq=24", *((ON, "algo.diag.every=4") if on else ())])
        out = tp.main(cfg)
        assert out["rollout_iterations"] == 48
        rows = [r for r in _jsonl(log) if "train/return" in r]
        assert len(rows) == 24
        if on:
            _check_rows(rows, 2, first_event=4)      # probe at hand-off 4, read one hand-off late; rows are logged every 2nd iteration
        else:
            assert not any(k.startswith("diag/") for r in rows for k in r)


def test_train_baselines_logs_the_diag_columns(tmp_path):
    tb = tc.load_script("scripts/train_baselines.py", "train_baselines_diag")
    from pql_amd.utils.cfg import load_cfg
    for on in (True, False):
        log = tmp_path / f"log_{on}.jsonl"
        cfg = load_cfg(["algo=ddpg_algo", "task=pointmass", *SMALL, f"max_step={64 * (32 + 48) - 1}", f"logging.jsonl={log}",
                        *((ON, "algo.diag.every=4") if on else ())])
        out = tb.main(cfg)
        assert out["iters"] == 48
        rows = _jsonl(log)
        if on:
            _check_rows(rows, 2, first_event=2)
        else:
            assert rows and not any(k.startswith("diag/") for r in rows for k in r)


def test_resume_with_diagnostics_on_is_bit_exact(tmp_path):
    """6 iterations + checkpoint + 6 resumed == 12 uninterrupted, diagnostics on in all three runs, and == the 12 with them off."""
    upto = lambda iters: f"max_step={64 * (32 + iters) - 1}"   # noqa: E731
    base = PQL_TOY + ["algo.graph=True", ON, "algo.diag.every=1"]
    a = child(PQL, base + [upto(12)], tmp_path)
    off = child(PQL, PQL_TOY + ["algo.graph=True", upto(12)], tmp_path)
    ck = tmp_path / "ck"
    b1 = child(PQL, base + [upto(6), f"checkpoint.dir={ck}"], tmp_path)
    b2 = child(PQL, base + [upto(12), f"resume={ck}"], tmp_path)
    assert (a["rollout_iterations"], b1["rollout_iterations"]) == (12, 6)
    assert b2["resumed_from"]["global_steps"] == b1["global_steps"]
    same(a, b2, PQL_KEYS)
    same(a, off, PQL_KEYS)
