"""`pqlk_lnmlp_pack_bf16` / `pqlk_lnmlp_forward_bf16` (pql_amd/csrc/fwd_ln_bf16.hip; `algo.critic_target_dtype=bfloat16`): the packed
copy against the layout law of include/pqlk.h, the forward against the bf16 LayerNorm law evaluated in float64, a row's bits against
its place in the batch, and AgentDDPG / AgentSAC running their target forward on it.

The forward's bar rests on two float64 references alone: o_law, the law on the bf16-rounded inputs and weights with the activations
rounded behind every ELU, and o_full, the unrounded network.  rms(Q - o_law) <= 1/8 rms(o_law - o_full): the kernel's distance from
its law (fp32 summation order, and a rounding it tips) against the law's own quantisation error."""
from copy import deepcopy

import pytest
import torch
import torch.nn.functional as F

import learner_harness as lh
from support import dev  # noqa: F401

pytestmark = pytest.mark.gpu

# hidden layers, obs + act, m.  [32]: one tile, seven idle waves; [160, 96]: ragged tiles per wave; [512, 512, 256]: two tiles per wave
# at 64 rows per block; [1024]: four tiles per wave at 32 rows per block; inputs padded to the k step (10 -> 16, 104 -> 112); m: one
# row, a partial only block, one row past a row tile, past a 64-row block, and three blocks with a partial last one
CASES = [([32], 10, 1), ([32], 104, 33), ([64, 32], 10, 31), ([64, 32], 104, 65), ([160, 96], 10, 33), ([160, 96], 104, 130),
         ([512, 512, 256], 10, 130), ([512, 512, 256], 104, 65), ([1024], 10, 130), ([1024], 104, 1), ([1024], 104, 33)]
IDS = lambda v: str(v).replace(" ", "")  # noqa: E731


def _critic(hidden, k, dev):
    from pql_amd.models.layernorm import DoubleQLayerNorm
    torch.manual_seed(len(hidden) * 1000 + k)
    q = DoubleQLayerNorm((k - 1,), 1, hidden, fused_forward=True, target_dtype="bfloat16").to(dev)
    for n in range(2):
        for l in range(len(hidden)):
            q.norm_param(n, l, "gamma").add_(0.2 * torch.randn(hidden[l], device=dev))
            q.norm_param(n, l, "beta").copy_(0.2 * torch.randn(hidden[l], device=dev))
    return q.refresh()


def _x(q, m, dev):
    from pql_amd import _lib as L
    from pql_amd.models.mlp import pad_cols
    return pad_cols(torch.randn(m, q.dims[0], device=dev), L.ld(q.dims[0]))


def _unpacked(q):
    """{(n, l): int16 bit patterns (out, in)} of the packed copy, read back through the layout law; the k padding must hold zeros."""
    out, per_net = {}, q.packed.numel() // 2
    for n in range(2):
        o = n * per_net
        for l in range(q.n_layers - 1):
            K, N = q.dims[l], q.dims[l + 1]
            KS = (K + 15) // 16
            w = q.packed[o: o + N * KS * 16].view(N // 32, KS, 2, 32, 8).permute(0, 3, 1, 2, 4).reshape(N, KS * 16)
            assert not bool(w[:, K:].any())
            out[n, l], o = w[:, :K], o + N * KS * 16
        out[n, q.n_layers - 1] = q.packed[o: o + q.dims[-2]].view(1, -1)
        assert o + q.dims[-2] == (n + 1) * per_net
    return out


def _pack_is_rne_of_arena(q):
    got = _unpacked(q)
    return all(torch.equal(got[n, l], q.weight(n, l).to(torch.bfloat16).view(torch.int16)) for n in range(2) for l in range(q.n_layers))


def _q64(q, x, rounded):
    """Twin Q (2, m) in float64: the unrounded network, or (rounded) the bf16 law."""
    from pql_amd.models.layernorm import LN_EPS
    rnd = (lambda t: t.to(torch.bfloat16).double()) if rounded else (lambda t: t.double())
    out, H = [], q.n_layers - 1
    for n in range(2):
        a = rnd(x)
        for l in range(H):
            z = F.linear(a, rnd(q.weight(n, l)), q.bias(n, l).double())
            a = rnd(F.elu(F.layer_norm(z, z.shape[1:], q.norm_param(n, l, "gamma").double(), q.norm_param(n, l, "beta").double(), LN_EPS)))
        out.append(F.linear(a, rnd(q.weight(n, H)), q.bias(n, H).double())[:, 0])
    return torch.stack(out)


@pytest.mark.parametrize("hidden, k, m", CASES, ids=IDS)
def test_pack_and_forward_against_float64(hidden, k, m, dev):
    q = _critic(hidden, k, dev)
    assert _pack_is_rne_of_arena(q)
    x = _x(q, m, dev)
    out = q.forward_raw(x, stash=False)
    assert not bool(out[:, :, 1:].any())   # the pad columns of Q
    o_law, o_full = _q64(q, x[:, :k], True), _q64(q, x[:, :k], False)
    rms = lambda t: float(t.pow(2).mean().sqrt())  # noqa: E731
    e, bar = rms(out[:, :, 0].double() - o_law), rms(o_law - o_full)
    print(f"{hidden} k={k} m={m}: rms(Q - o_law) {e:.3e}, rms(o_law - o_full) {bar:.3e}, ratio {e / bar:.4f}")
    assert e <= bar / 8


@pytest.mark.parametrize("hidden, k", [([64, 32], 10), ([1024], 104)], ids=IDS)   # 64 and 32 rows per block
def test_a_rows_bits_do_not_depend_on_the_batch(hidden, k, dev):
    q = _critic(hidden, k, dev)
    x = _x(q, 130, dev)
    full = q.forward_raw(x, stash=False).clone()
    assert torch.equal(full, q.forward_raw(x, stash=False))   # two launches
    assert torch.equal(full[:, 97:], q.forward_raw(x[97:].contiguous(), stash=False))   # m = 33, other lanes and blocks
    for i in (0, 31, 32, 64, 129):
        assert torch.equal(full[:, i], q.forward_raw(x[i: i + 1].contiguous(), stash=False)[:, 0]), i
    x[40, 3] = float("nan")
    bad = q.forward_raw(x, stash=False)
    keep = torch.arange(130, device=dev) != 40
    assert bool(bad[:, 40, 0].isnan().all()) and torch.equal(bad[:, keep], full[:, keep])


# ---- the agents: (8, 2), B = 96, hidden [64, 32]
O, A, B = 8, 2, 96
KEY = "algo.critic_target_dtype"


def _agent(algo, dev, value):
    """value None: a config from before the key existed."""
    from pql_amd.envs.synthetic import create_task_env
    from pql_amd.replay.simple_replay import ReplayBuffer
    from pql_amd.utils.cfg import load_cfg
    cfg = load_cfg([f"algo={algo}_algo", "task.name=Toy", "num_envs=64", f"algo.batch_size={B}", "algo.memory_size=400", "device=cuda:0",
                    "sim_device=cuda:0", "algo.cri_class=DoubleQLayerNorm", "algo.hidden_layers=[64,32]", "algo.critic_fused_forward=True",
                    *([] if value is None else [f"{KEY}={value}"])])
    if value is None:
        cfg.algo.pop("critic_target_dtype")
    if algo == "ddpg":
        from pql_amd.algo.ddpg import AgentDDPG as Agent
    else:
        from pql_amd.algo.sac import AgentSAC as Agent
    torch.manual_seed(5)
    agent = Agent(create_task_env(cfg), cfg)
    memory = ReplayBuffer(400, (O,), A, device=dev)
    memory.add_to_buffer(tuple(t.to(dev) for t in lh._fill(O, A, 300, 810)))
    g = torch.Generator().manual_seed(100)
    draws = dict(indices=torch.randint(300, (B,), generator=g))
    draws.update({k: torch.randn(B, A, generator=g) for k in (("noise",) if algo == "ddpg" else ("eps_next", "eps_cur"))})
    return agent, memory, draws


@pytest.mark.parametrize("algo", ["ddpg", "sac"])
def test_the_target_forward_is_the_bf16_launch_and_its_pack_follows(algo, dev):
    agent, memory, draws = _agent(algo, dev, "bfloat16")
    assert agent.critic_target.packed is not None and _pack_is_rne_of_arena(agent.critic_target)
    before, seen, inner = deepcopy(agent.critic_target), {}, agent._critic_forward

    def spy(ws, net, x, slot, probe=False):
        out = inner(ws, net, x, slot, probe)
        if slot == "t":   # what the loss is about to consume (SAC lowers it in place afterwards)
            assert net is agent.critic_target
            seen.update(q=out[0].clone(), x=x.clone())
        return out

    agent._critic_forward = spy
    agent.update_once(memory, **draws)
    assert torch.equal(seen["q"], before.forward_raw(seen["x"], stash=False))
    assert not torch.equal(seen["q"], before.forward_raw(seen["x"]))   # (and not the fp32 launch's bits)
    assert not torch.equal(agent.critic_target.arena.data, before.arena.data) and _pack_is_rne_of_arena(agent.critic_target)


@pytest.mark.parametrize("algo", ["ddpg", "sac"])
def test_float32_is_the_config_without_the_key(algo, dev):
    states = []
    for value in ("float32", None):
        agent, memory, draws = _agent(algo, dev, value)
        assert agent.critic_target.packed is None
        agent.update_once(memory, **draws)
        states.append({k: v.clone() for k, v in agent._state_tensors().items()})
    assert set(states[0]) == set(states[1]) and all(torch.equal(states[0][k], states[1][k]) for k in states[0])
