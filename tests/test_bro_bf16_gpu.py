"""`pqlk_bro_pack_bf16` / `pqlk_bro_forward_bf16` (pql_amd/csrc/fwd_bro_bf16.hip; `algo.critic_target_dtype=bfloat16` with
`algo.cri_class=DoubleQBroNet`): the packed copy against the layout law of include/pqlk.h, the forward against the bf16 residual law
evaluated in float64, K = 0 against `pqlk_lnmlp_forward_bf16`, a row's bits against its place in the batch, and the agents on it.

Two float64 references alone: o_law, the law (inputs, weights and the input of every Linear rounded, the residual stream NOT), and
o_full, the unrounded network.  Bar: rms(Q - o_law) <= 1/2 rms(o_law - o_full) -- in a residual stack one bf16 rounding tipped by the
fp32 summation order propagates through every later block (the law in float32 with a shuffled k order stayed below 0.18 on these
shapes; a missing skip or a wrong layer gives >> 1).  With the closing layers' gamma and beta scaled by 2^-8 an fp32 stream keeps the
blocks' updates (that emulation: <= 0.035; bar 1/8), a stream rounded to bf16 per block loses them (>= 1.0)."""
from copy import deepcopy

import pytest
import torch
import torch.nn.functional as F

import learner_harness as lh
from support import dev  # noqa: F401

pytestmark = pytest.mark.gpu

# W, K, obs + act, m.  W 32: one tile, seven idle waves; K 16: 34 Linears, past PQLK_MAX_LAYERS; 160: ragged tiles per wave; 512: two
# tiles per wave at 64 rows per block; 544: three tiles at 32 rows per block; 1024: four; inputs padded to the k step (10 -> 16,
# 104 -> 112); m: one row, a partial only block, one row past a row tile, past a 64-row block, three blocks with a partial last one
CASES = [(32, 0, 10, 1), (32, 1, 104, 33), (32, 16, 10, 33), (64, 3, 10, 31), (160, 1, 10, 33), (160, 2, 104, 130), (512, 2, 104, 65),
         (512, 2, 10, 130), (544, 1, 104, 33), (1024, 1, 104, 1), (1024, 2, 10, 130)]


def _critic(w, blocks, k, dev, closing_scale=1.0):
    from pql_amd.models.bronet import DoubleQBroNet
    torch.manual_seed(w * 100 + blocks * 1000 + k)
    q = DoubleQBroNet((k - 1,), 1, w, blocks, fused_forward=True, target_dtype="bfloat16").to(dev)
    for n in range(2):
        for l in range(q.n_layers - 1):
            q.norm_param(n, l, "gamma").add_(0.2 * torch.randn(w, device=dev))
            q.norm_param(n, l, "beta").copy_(0.2 * torch.randn(w, device=dev))
            if l > 0 and l % 2 == 0:
                q.norm_param(n, l, "gamma").mul_(closing_scale)
                q.norm_param(n, l, "beta").mul_(closing_scale)
    return q.refresh()


def _x(q, m, dev):
    from pql_amd import _lib as L
    from pql_amd.models.mlp import pad_cols
    return pad_cols(torch.randn(m, q.dims[0], device=dev), L.ld(q.dims[0]))


def _pack_is_rne_of_arena(q):
    """The packed copy, read back through the layout law, is weight.to(bfloat16) bit for bit; the k padding holds zeros."""
    per_net, ok = q.packed.numel() // 2, True
    for n in range(2):
        o = n * per_net
        for l in range(q.n_layers - 1):
            K, N = q.dims[l], q.dims[l + 1]
            KS = (K + 15) // 16
            w = q.packed[o: o + N * KS * 16].view(N // 32, KS, 2, 32, 8).permute(0, 3, 1, 2, 4).reshape(N, KS * 16)
            ok = ok and not bool(w[:, K:].any()) and torch.equal(w[:, :K], q.weight(n, l).to(torch.bfloat16).view(torch.int16))
            o += N * KS * 16
        ok = ok and torch.equal(q.packed[o: o + q.width].view(1, -1), q.weight(n, q.n_layers - 1).to(torch.bfloat16).view(torch.int16))
        ok = ok and o + q.width == (n + 1) * per_net
    return ok


def _q64(q, x, rounded):
    """Twin Q (2, m) in float64: the unrounded network, or (rounded) the bf16 residual law with its stream unrounded."""
    from pql_amd.models.layernorm import LN_EPS
    rnd = (lambda t: t.to(torch.bfloat16).double()) if rounded else (lambda t: t.double())
    out = []
    for n in range(2):
        def ln(a, l):   # LayerNorm(Linear_l(the rounded copy of a))
            z = F.linear(rnd(a), rnd(q.weight(n, l)), q.bias(n, l).double())
            return F.layer_norm(z, z.shape[1:], q.norm_param(n, l, "gamma").double(), q.norm_param(n, l, "beta").double(), LN_EPS)
        h = F.elu(ln(x, 0))
        for k in range(1, q.blocks + 1):
            h = h + ln(F.elu(ln(h, 2 * k - 1)), 2 * k)   # the stream itself is never rounded
        out.append(F.linear(rnd(h), rnd(q.weight(n, q.n_layers - 1)), q.bias(n, q.n_layers - 1).double())[:, 0])
    return torch.stack(out)


def _ratio(q, x, out, what):
    k = q.dims[0]
    o_law, o_full = _q64(q, x[:, :k], True), _q64(q, x[:, :k], False)
    rms = lambda t: float(t.pow(2).mean().sqrt())  # noqa: E731
    e, bar = rms(out[:, :, 0].double() - o_law), rms(o_law - o_full)
    print(f"{what}: rms(Q - o_law) {e:.3e}, rms(o_law - o_full) {bar:.3e}, ratio {e / bar:.4f}")
    return e / bar


@pytest.mark.parametrize("w, blocks, k, m", CASES)
def test_pack_and_forward_against_float64(w, blocks, k, m, dev):
    q = _critic(w, blocks, k, dev)
    assert _pack_is_rne_of_arena(q)
    x = _x(q, m, dev)
    out = q.forward_raw(x, stash=False)
    assert not bool(out[:, :, 1:].any())   # the pad columns of Q
    assert _ratio(q, x, out, f"W={w} K={blocks} k={k} m={m}") <= 1 / 2


@pytest.mark.parametrize("w, k", [(32, 10), (64, 104)])
def test_the_residual_stream_is_fp32(w, k, dev):
    q = _critic(w, 16, k, dev, closing_scale=2.0 ** -8)
    x = _x(q, 33, dev)
    assert _ratio(q, x, q.forward_raw(x, stash=False), f"W={w} K=16 k={k}, closing gamma / beta x 2^-8") <= 1 / 8


@pytest.mark.parametrize("w, k", [(32, 10), (1024, 104)])
def test_no_blocks_is_the_layernorm_entry(w, k, dev):
    from pql_amd.models.layernorm import DoubleQLayerNorm
    q = _critic(w, 0, k, dev)
    ln = DoubleQLayerNorm((k - 1,), 1, [w], fused_forward=True, target_dtype="bfloat16").to(dev)
    ln.arena.data.copy_(q.arena.data)
    ln.refresh()
    x = _x(q, 130, dev)
    assert torch.equal(q.packed, ln.packed) and torch.equal(q.forward_raw(x, stash=False), ln.forward_raw(x, stash=False))


@pytest.mark.parametrize("w, blocks", [(64, 2), (1024, 1)])   # 64 and 32 rows per block
def test_a_rows_bits_do_not_depend_on_the_batch(w, blocks, dev):
    q = _critic(w, blocks, 10, dev)
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


# ---- the agents: (8, 2), B = 96, width 64, 1 block
O, A, B = 8, 2, 96
KEY = "algo.critic_target_dtype"


def _agent(algo, dev, value):
    """value None: a config from before the key existed."""
    from pql_amd.envs.synthetic import create_task_env
    from pql_amd.replay.simple_replay import ReplayBuffer
    from pql_amd.utils.cfg import load_cfg
    cfg = load_cfg([f"algo={algo}_algo", "task.name=Toy", "num_envs=64", f"algo.batch_size={B}", "algo.memory_size=400", "device=cuda:0",
                    "sim_device=cuda:0", "algo.cri_class=DoubleQBroNet", "algo.critic_width=64", "algo.critic_blocks=1",
                    "algo.hidden_layers=[64,32]", "algo.bronet_fused_forward=True", *([] if value is None else [f"{KEY}={value}"])])
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
