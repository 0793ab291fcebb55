"""The V-learner with `algo.target_dtype=bfloat16`: its two no-gradient forwards (target policy, target twin critic) on the
forward-only bf16-MFMA stack, everything else unchanged.  Batch 256, hidden [128, 128], O = 8, A = 2.  `pytest -m gpu`."""
import pytest
import torch

import bf16_model as M
import detdata as dd
from support import dev  # noqa: F401

pytestmark = pytest.mark.gpu

O, A, B, HIDDEN = 8, 2, 256, [128, 128]
T = lambda a: torch.from_numpy(a.copy())   # noqa: E731


def make_cfg(target_dtype="bfloat16", graph=False, distl=False, rng="auto", memory=3000, hidden=HIDDEN):
    from pql_amd.utils.cfg import load_cfg
    cfg = load_cfg([f"algo.batch_size={B}", f"algo.memory_size={memory}", f"algo.distl={distl}", "algo.v_learner_gpu=0", "algo.p_learner_gpu=0",
                    "algo.num_gpus=1", f"algo.graph={graph}", f"algo.rng={rng}", f"algo.target_dtype={target_dtype}", "task.name=Toy"])
    cfg.algo.hidden_layers = hidden
    return cfg


def _sd(state):
    return {k: T(v) for k, v in state.items()}


def _fill(rows, seed):
    return (T(dd.uniform((rows, O), seed, -3, 3)), T(dd.uniform((rows, A), seed + 1)), T(dd.uniform((rows, 1), seed + 2, -0.05, 0.05)),
            T(dd.uniform((rows, O), seed + 3, -3, 3)), T(dd.bernoulli((rows, 1), seed + 4, 0.1)))


def _norm(dev, k=0):
    return (T(dd.uniform((O,), 6 + 10 * k, -0.5, 0.5)).to(dev), T(dd.uniform((O,), 7 + 10 * k, 0.5, 2.0)).to(dev), 1e-4)


def _actor(dev):
    from pql_amd.models.mlp import TanhMLPPolicy
    actor = TanhMLPPolicy((O,), A, hidden_layers=HIDDEN).to(dev)
    actor.load_state_dict(_sd(dd.mlp_state(O, A, 11, hidden=tuple(HIDDEN))))
    return actor


def _learner(cfg, seed=1234):
    from pql_amd.algo.pql_v_learner import PQLVLearner
    v = PQLVLearner((O,), A, cfg)
    if not cfg.algo.distl:
        v.critic.load_state_dict(_sd(dd.doubleq_state(O, A, 1, 21, hidden=tuple(HIDDEN))))
        v.critic_target.arena.data.copy_(v.critic.arena.data)
    v.use_private_rng(seed)
    return v


def _state(v):
    torch.cuda.synchronize()
    out = [t.clone() for t in (v.critic.arena.data, v.critic_target.arena.data, v.opt.m, v.opt.v, v.loss_ring)]
    if v.pk_target_bf16 is not None:
        out.append(v.pk_target_bf16.tensor.clone())
    return out + [torch.tensor([v.gen.get_offset(), v.update_count])]


def _same(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


def _nets(module):
    lay, arena = module.layout, module.arena.data.cpu()
    W = [[lay.weight(arena, n, l).clone() for l in range(lay.n_layers)] for n in range(lay.n_nets)]
    b = [[lay.bias(arena, n, l).clone() for l in range(lay.n_layers)] for n in range(lay.n_nets)]
    return lay.dims, W, b


def _rms_ok(y, o64, fp32, what):
    got, dist = M.rms(y.double() - o64), M.rms(o64 - fp32)
    print(f"{what}: rms(y - o64) {got:.3e}, rms(o64 - fp32) {dist:.3e}, ratio {got / dist:.4f}")
    assert dist > 0 and got <= dist / 8, (what, got, dist)


def test_one_injected_step_takes_its_target_from_the_bf16_forwards(dev):
    """a' in the action columns of the target critic's tile and the target Q in the output block of `acts_t` meet the kernel
    criterion of realistic data (rms(y - o64) <= 1/8 rms(o64 - unrounded network)) against the model evaluated on the tile's own
    contents and on the target's weights from BEFORE the step's Polyak update; the step's loss is the twin MSE recomputed in
    torch from the learner's own Q and that target, to the rounding of an fp32 sum of B terms."""
    from pql_amd.models.mlp import output_view
    cfg = make_cfg()
    v, actor = _learner(cfg), _actor(dev)
    v.update(actor, tuple(t.to(dev) for t in _fill(900, 50)), _norm(dev), 0)
    tdims, tW, tb = _nets(v.critic_target)
    adims, aW, ab = _nets(v.actor)
    idx, draw = T(dd.integers((B,), 8, 900)), T(dd.uniform((B, A), 9, -2, 2))
    v.learn(indices=idx, noise=draw)
    torch.cuda.synchronize()
    ws, cl = v._ws, v.critic.layout
    tile = ws["xn_sa"].cpu()
    std, clip = float(cfg.algo.noise.tgt_pol_std), float(cfg.algo.noise.tgt_pol_noise_bound)
    a64 = M.forward(adims, aW, ab, tile, M.ACT_TANH_NOISE, draw, std=std, clip=clip)["out"][0]
    a32 = M.forward_fp32(adims, aW, ab, tile, M.ACT_TANH_NOISE, draw, std=std, clip=clip)[0]
    _rms_ok(tile[:, O:O + A], a64, a32, "a'")
    assert float(tile[:, O:O + A].abs().max()) <= 1.0 and not tile[:, O + A:].any()
    qt = output_view(cl, ws["acts_t"], B).cpu()
    _rms_ok(qt[:, :, :1], M.forward(tdims, tW, tb, tile)["out"], M.forward_fp32(tdims, tW, tb, tile), "target Q")
    assert not qt[:, :, 1:].any()
    q = output_view(cl, ws["acts_c"], B).cpu()[:, :, 0].double()
    gamma_n = float(cfg.algo.gamma) ** int(cfg.algo.nstep)
    y = ws["rew"].cpu().double() + (1.0 - ws["done"].cpu().double()) * gamma_n * torch.minimum(qt[0, :, 0], qt[1, :, 0]).double()
    loss = float(((q[0] - y) ** 2).mean() + ((q[1] - y) ** 2).mean())
    got = float(v.loss_ring[0])
    assert abs(got - loss) <= 2 * B * 2.0 ** -24 * loss, (got, loss)
    assert v.pk_actor_bf16 is not None and v.pk_target_bf16.tensor.dtype == torch.int16
    # the refreshed copy follows the Polyak step inside the same step
    want = M.unpack(v.pk_target_bf16.tensor.cpu(), cl.dims, 2)
    for n in range(2):
        for l in range(cl.n_layers):
            assert torch.equal(want[n][l], cl.weight(v.critic_target.arena.data.cpu(), n, l).to(torch.bfloat16).view(torch.int16))


def test_graph_replay_equals_eager(dev):
    outs = []
    actor = _actor(dev)
    for graph in (False, True):
        v = _learner(make_cfg(graph=graph))
        v.update(actor, tuple(t.to(dev) for t in _fill(2000, 5)), _norm(dev), 0)
        for _ in range(11):
            v.learn()
        outs.append(_state(v))
    _same(*outs)
    assert float(outs[0][4].abs().sum()) > 0


def test_learn_many_equals_the_per_step_calls(dev):
    from pql_amd.utils import rng as R
    assert R.verified(dev) is not None, "pqlk_philox_draws must reproduce torch's draws on this device"
    outs = []
    actor = _actor(dev)
    for many in (False, True):
        v = _learner(make_cfg(graph=True))
        K, runs = v._depth, 0
        for it in range(3):
            v.update(actor, tuple(t.to(dev) for t in _fill(700, 100 + it)), _norm(dev, it), 0)
            for n in ([K] if it != 1 else [3, K - 3]):   # iteration 1 begins with a partial run
                if many:
                    runs += v._run_in_one_graph(v._workspace(B), n)
                    v.learn_many(n)
                else:
                    for _ in range(n):
                        v.learn()
        if many:
            assert runs == 2 and v._run_graph is not None
        assert v.update_count == 3 * K
        outs.append(_state(v))
    _same(*outs)


@pytest.mark.parametrize("graph", [False, True])
def test_draws_ahead_equal_the_per_step_draws(dev, graph):
    """algo.rng=auto: the K steps' target actions come from ONE bf16 policy forward over K x B rows at prefetch time;
    algo.rng=torch: one bf16 policy forward inside every step.  Same seeds -> same bits, across `update()` calls in mid-run."""
    outs = []
    actor = _actor(dev)
    for mode in ("torch", "auto"):
        v = _learner(make_cfg(graph=graph, rng=mode))
        for phase, steps in enumerate((3, 8, 5)):
            v.update(actor, tuple(t.to(dev) for t in _fill(700, 50 + 10 * phase)), _norm(dev), 0)
            for _ in range(steps):
                v.learn()
        assert v.rng == ("philox" if mode == "auto" else "torch")
        assert v._ws["actor_ahead"] == (mode == "auto")
        outs.append(_state(v))
    _same(*outs)


def test_resume_from_a_checkpoint_equals_the_uninterrupted_run(dev, tmp_path):
    """Checkpoint after 12 of 24 steps through pql_amd.utils.checkpoint (state file + streamed ring rows), a NEW learner resumes:
    bit-identical to the run that never stopped.  The structural config refuses the other target dtype, naming both values."""
    from pql_amd.utils import checkpoint as CK
    actor = _actor(dev)

    def phase(v, k):
        v.update(actor, tuple(t.to(dev) for t in _fill(700, 200 + k)), _norm(dev, k), 0)
        for _ in range(6):
            v.learn()

    a = _learner(make_cfg(graph=True))
    for k in range(4):
        phase(a, k)
    b1 = _learner(make_cfg(graph=True))
    for k in range(2):
        phase(b1, k)
    torch.cuda.synchronize()
    cfg = make_cfg(graph=True)
    CK.save(str(tmp_path / "ck"), 12, {"v": b1.training_state(), "structure": CK.structure(cfg, O, A)}, rings={"v_ring": b1.memory.rows()})
    b2 = _learner(make_cfg(graph=True), seed=99)   # (another seed: the generator's state must come out of the checkpoint)
    ckpt, st = CK.load(str(tmp_path / "ck"))
    CK.check_structure(st["structure"], CK.structure(cfg, O, A))
    b2.load_training_state(st["v"])
    CK.load_ring(ckpt, st, "v_ring", b2.memory.rows())
    torch.cuda.synchronize()
    _same(_state(b1), _state(b2))
    for k in range(2, 4):
        phase(b2, k)
    _same(_state(a), _state(b2))
    with pytest.raises(ValueError, match=r"algo\.target_dtype='float32'.*algo\.target_dtype='bfloat16'"):
        CK.check_structure(st["structure"], CK.structure(make_cfg("float32"), O, A))
    with pytest.raises(ValueError, match=r"algo\.target_dtype='bfloat16'.*algo\.target_dtype='float32'"):
        CK.check_structure(CK.structure(make_cfg("float32"), O, A), CK.structure(cfg, O, A))


def test_c51_critic_takes_the_bf16_target_forward_and_trains_finite(dev):
    calls = []
    v = _learner(make_cfg(distl=True))
    assert v.critic.layout.dims[-1] == 51 and v.pk_target_bf16 is not None
    v.update(_actor(dev), tuple(t.to(dev) for t in _fill(2000, 5)), _norm(dev), 0)
    import pql_amd.algo.pql_v_learner as VL
    real = VL.mlp_forward_bf16_raw
    VL.mlp_forward_bf16_raw = lambda lay, *a, **k: (calls.append(lay.dims[-1]), real(lay, *a, **k))[1]
    try:
        before = v.critic.arena.data.clone()
        for _ in range(10):
            v.learn()
        torch.cuda.synchronize()
    finally:
        VL.mlp_forward_bf16_raw = real
    assert calls.count(51) == 10 and calls.count(A) == 2   # ten target forwards; two prefetches of 8 steps' target actions
    assert bool(torch.isfinite(v.critic.arena.data).all()) and bool(torch.isfinite(v.loss_ring).all()) and float(v.loss_ring.abs().sum()) > 0
    assert not torch.equal(before, v.critic.arena.data)


class _Calls:
    """Records the libpqlk entry points a block of code calls, in order."""
    QUERIES = ("_parts", "_offsets", "_offset", "_floats", "_stride", "_elems", "_ok", "_ld", "_version", "_strerror")

    def __init__(self):
        from pql_amd import _lib as L
        self.L, self.names = L, []

    def __enter__(self):
        L = self.L
        self.real = L.lib

        class Proxy:
            def __getattr__(_, name):
                fn = getattr(self.real, name)
                if not name.startswith("pqlk_") or name.endswith(self.QUERIES):   # (host-side size / offset queries launch nothing)
                    return fn

                def wrapped(*a):
                    self.names.append(name)
                    return fn(*a)
                return wrapped
        L.lib = Proxy()
        return self

    def __exit__(self, *exc):
        self.L.lib = self.real


def test_float32_builds_no_bf16_buffers_and_keeps_its_launch_sequence(dev):
    """The default: no bf16 buffer exists and a step calls the four entry points it called before (target forward, critic
    forward, backward, optimiser: the 9 launches of DESIGN 4.2 at the BASELINE shape), none of them a bf16 one.  bfloat16: the
    same calls with the target forward swapped for the bf16 one and ONE pack launch behind the optimiser (10 launches)."""
    actor = _actor(dev)
    seqs = {}
    for dt in ("float32", "bfloat16"):
        v = _learner(make_cfg(dt))
        v.update(actor, tuple(t.to(dev) for t in _fill(2000, 5)), _norm(dev), 0)
        v.learn()
        torch.cuda.synchronize()
        assert (v.pk_target_bf16 is None and v.pk_actor_bf16 is None) == (dt == "float32")
        assert v._ahead.valid > 0   # the next step finds its tiles and target actions prepared
        with _Calls() as c:
            v.learn()
        torch.cuda.synchronize()
        seqs[dt] = c.names
    print(seqs)
    f32 = seqs["float32"]   # target forward, critic forward, backward with the TD head, optimiser
    assert len(f32) == 4 and f32[0] == "pqlk_mlp_forward" and f32[-1] == "pqlk_adamw_polyak_fused" and not any("bf16" in n for n in f32)
    assert seqs["bfloat16"] == ["pqlk_mlp_forward_bf16"] + f32[1:] + ["pqlk_mlp_pack_bf16"]


def test_bad_values_and_shapes_are_errors_at_construction(dev):
    from pql_amd.algo.pql_v_learner import PQLVLearner
    with pytest.raises(ValueError, match=r"algo\.target_dtype"):
        PQLVLearner((O,), A, make_cfg("float16"))
    with pytest.raises(ValueError, match=r"algo\.target_dtype=bfloat16.*critic"):
        PQLVLearner((O,), A, make_cfg(hidden=[100, 64]))
    with pytest.raises(ValueError, match=r"algo\.target_dtype=bfloat16.*actor"):
        PQLVLearner((O,), 70, make_cfg())          # 70 actions: past the 64 output columns of the bf16 stack
    cfg = make_cfg()
    cfg.algo.fused = False
    with pytest.raises(ValueError, match=r"algo\.target_dtype=bfloat16.*fused"):
        PQLVLearner((O,), A, cfg)
