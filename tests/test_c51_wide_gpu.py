"""Categorical critics with 65 ... 256 atoms on the GPU: the three loss entry points on their wide kernels, the MLP path with an
output layer wider than 64, both learners against the oracle at 101 atoms (eager, and hipGraph replay bit-equal to eager), and
scripts/train_pql.py.  Shapes and inputs: tests/c51_wide_cases.py (proved without a GPU in tests/test_c51_wide_cpu.py).

Every buffer a kernel writes has SLACK floats of poison behind it and poison pad columns, which must come back intact, or zero
where include/pqlk.h says "written as zero"; every input has slack that would move the result.  The bars are those of the
existing test each section names (tests/test_reductions_gpu.py, tests/test_kernels_gpu.py, tests/test_learners_gpu.py)."""
import ctypes as C

import numpy as np
import pytest
import torch

import c51_wide_cases as wc
import detdata as dd
import reduction_cases as rc
from guarded import Guarded
from learner_harness import _compare_nets, _sd
from support import dev  # noqa: F401

pytestmark = pytest.mark.gpu

T = rc.T
POISON, SLACK = rc.POISON, rc.SLACK


@pytest.fixture(scope="module")
def ref():
    from oracle import pql_ref_cpu
    return pql_ref_cpu


def _g(dev, arr, fill):
    arr = arr if torch.is_tensor(arr) else T(np.asarray(arr))
    return Guarded(dev, tuple(arr.shape), fill, arr)


# =========================================================================== projection
_PROJECT_CASES = [(wc.PROJECT_B, K) for K in wc.KS] + [(rc.PROJECT_B, 101)]


@pytest.mark.parametrize("B,K", _PROJECT_CASES)
def test_c51_project_wide(dev, ref, B, K):
    """Terminal rows (one bin collects all K atoms), terminal rows with the reward on an atom, non-terminal rows with rewards past
    both ends; B = 263 and past the grid cap.  Bars of test_c51_project_past_the_grid_cap."""
    from pql_amd import _lib as L
    p, rew, done, gn, _ = wc.project_inputs(B, K)
    want = ref.c51_project_ref(p, rew, done, gn, -10, 10, K).numpy()
    pd, rd, dd_ = _g(dev, p, rc.IN_BIG), _g(dev, rew.view(-1), rc.IN_BIG), _g(dev, done.view(-1), rc.IN_BIG)
    zd = _g(dev, torch.linspace(-10, 10, K), rc.IN_BIG)
    out = Guarded(dev, (B, K), POISON)
    L.check(L.lib.pqlk_c51_project(pd.ptr, rd.ptr, dd_.ptr, zd.ptr, gn, -10.0, 10.0, K, B, out.ptr, L.stream(dev)))
    got = out.t.cpu().numpy()
    print(f"project B={B} K={K}: max |got - want| = {np.abs(got - want).max():.3e}")
    np.testing.assert_allclose(got, want, atol=1e-7)
    assert np.array_equal(got != 0, want != 0)
    assert out.intact()


# =========================================================================== BCE
_C51_REF = {}


def _c51_case(ref, B, K, saturated):
    """(inputs, reference) computed once per case and shared; nobody writes to them."""
    key = (B, K, saturated)
    if key not in _C51_REF:
        inp = wc.bce_inputs(B, K, saturated)
        _C51_REF[key] = (inp, rc.c51_reference(ref, *inp, K))
    return _C51_REF[key]


def _c51_check(dev, ref, B, K, ld, saturated=False):
    """tests/test_reductions_gpu.py's _c51_check on the inputs of c51_wide_cases.bce_inputs, bars unchanged."""
    from pql_amd import _lib as L
    (lg, lt, rew, done, gn), (tgt, loss, grad) = _c51_case(ref, B, K, saturated)

    def padded(x):
        g = Guarded(dev, (2, B, ld), rc.IN_BIG)
        g.t[:, :, :K] = x.to(dev)
        return g

    lgd, ltd = padded(lg), padded(lt)
    rd, dd_ = _g(dev, rew.view(-1), rc.IN_BIG), _g(dev, done.view(-1), rc.IN_BIG)
    zd = _g(dev, torch.linspace(-10.0, 10.0, K), rc.IN_BIG)
    parts = int(L.lib.pqlk_loss_parts(B, K))
    outs = []
    for with_proj in (True, False):
        dy, lo, scr = Guarded(dev, (2, B, ld), POISON), Guarded(dev, (1,), POISON), Guarded(dev, (parts,), POISON)
        pj = Guarded(dev, (B, K), POISON)
        L.check(L.lib.pqlk_c51_bce_loss(lgd.ptr, ltd.ptr, ld, K, rd.ptr, dd_.ptr, zd.ptr, gn, -10.0, 10.0, B, dy.ptr, lo.ptr, None, 0,
                                        pj.ptr if with_proj else None, scr.ptr, L.stream(dev)))
        for b in (dy, lo, scr, pj):
            assert b.intact()
        outs.append((dy.t.clone(), lo.t.clone()))
        if not with_proj:
            assert bool((pj.t == POISON).all())
            continue
        g = dy.t[:, :, :K].cpu().numpy()
        print(f"bce B={B} K={K} ld={ld} sat={saturated}: proj {np.abs(pj.t.cpu().numpy() - tgt.numpy()).max():.3e}  "
              f"loss rel {abs(lo.t.item() - loss.item()) / abs(loss.item()):.3e}  "
              f"grad worst (|d| - 2e-9) / |ref| {((np.abs(g - grad.numpy()) - 2e-9) / np.maximum(np.abs(grad.numpy()), 1e-30)).max():.3e}")
        np.testing.assert_allclose(pj.t.cpu().numpy(), tgt.numpy(), atol=2e-7)
        np.testing.assert_allclose(lo.t.item(), loss.item(), rtol=5e-6)
        np.testing.assert_allclose(g, grad.numpy(), rtol=2e-4, atol=2e-9)
        assert torch.count_nonzero(dy.t[:, :, K:]) == 0          # pads written as zero
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])      # proj_out = NULL changes nothing
    return outs[0][0]


@pytest.mark.parametrize("K,ld", wc.SHAPES)
def test_c51_bce_wide_shapes(dev, ref, K, ld):
    """One atom past a wave, a ragged last group, every lane of every group, pad columns past the last group; 10 of the 37 rows
    terminal."""
    _c51_check(dev, ref, wc.B_SMALL, K, ld)


@pytest.mark.parametrize("K", [101, 256])
@pytest.mark.parametrize("B", [1, 3, 5])
def test_c51_bce_wide_blocks_with_idle_waves(dev, ref, B, K):
    """Fewer rows than a block has waves, and a second block with one row: the waves of a block leave the row loop at different
    trips (nothing in it may wait for the whole block)."""
    _c51_check(dev, ref, B, K, 128 if K == 101 else 256)


def test_c51_bce_wide_past_the_grid_cap(dev, ref):
    """The third, ragged trip of the capped grid."""
    _c51_check(dev, ref, rc.C51_B_BIG, 101, 128)


@pytest.mark.parametrize("K", [101, 256])
def test_c51_bce_wide_saturated_rows(dev, ref, K):
    """As test_c51_bce_saturated_rows: rows whose softmax is 1.0 on one atom, where max(log p, -100) and max((1 - p) p, 1e-12) bind."""
    dy = _c51_check(dev, ref, wc.B_SMALL, K, 128 if K == 101 else 256, saturated=True)
    hard = [i for i, gap in enumerate(rc.SAT_GAPS) if gap >= 60]
    assert bool(torch.isfinite(dy).all()) and float(dy[:, hard].abs().max()) < 2e-9


# =========================================================================== distributional DPG
@pytest.mark.parametrize("B,K,ld", [(wc.B_SMALL, K, ld) for K, ld in wc.SHAPES] + [(rc.C51_B_BIG, 101, 128)])
def test_dpg_dist_wide(dev, B, K, ld):
    """Bars of test_dpg_dist_shapes; the tie rows (every seventh) split the gradient evenly between the nets."""
    from pql_amd import _lib as L
    q = rc.dpg_dist_inputs(B, K)
    z, loss, grad = rc.dpg_dist_reference(q, K)
    qd = Guarded(dev, (2, B, ld), rc.IN_BIG); qd.t[:, :, :K] = q.to(dev)
    zd = _g(dev, z, rc.IN_BIG)
    dy, lo = Guarded(dev, (2, B, ld), POISON), Guarded(dev, (1,), POISON)
    scr = Guarded(dev, (int(L.lib.pqlk_loss_parts(B, K)),), POISON)
    L.check(L.lib.pqlk_dpg_loss(qd.ptr, ld, K, zd.ptr, B, dy.ptr, lo.ptr, None, 0, scr.ptr, L.stream(dev)))
    print(f"dpg B={B} K={K} ld={ld}: loss rel {abs(lo.t.item() - loss.item()) / abs(loss.item()):.3e}")
    np.testing.assert_allclose(lo.t.item(), loss.item(), rtol=5e-6)
    np.testing.assert_allclose(dy.t[:, :, :K].cpu().numpy(), grad.numpy(), rtol=5e-5, atol=1e-9)
    assert torch.count_nonzero(dy.t[:, :, K:]) == 0
    assert dy.intact() and lo.intact() and scr.intact()
    ties = dy.t[:, ::7, :K]
    assert ties.shape[1] == (B + 6) // 7 and torch.equal(ties[0], ties[1]) and bool((ties[0] != 0).any(1).all())
    if B == wc.B_SMALL:
        assert ties.shape[1] == 6


# =========================================================================== MLP with an output layer wider than 64
_MLP = [
    # dims (in, hidden..., out), nets, B, fused?
    ([24, 64, 64, 101], 2, 96, True),
    ([104, 128, 128, 256], 2, 130, True),
    ([48, 100, 36, 129], 1, 65, False),
]


@pytest.mark.parametrize("dims,nets,B,fused", _MLP)
def test_mlp_with_a_wide_output_layer_vs_oracle(dev, ref, dims, nets, B, fused):
    """Method and bars of test_mlp_shape_sweep_vs_oracle: forward (every stashed activation block the oracle exposes: the output)
    and backward (parameter + input gradients) against the oracle's torch-CPU autograd."""
    from pql_amd import _lib as L
    from pql_amd.models.mlp import ArenaLayout, PackedWeights, default_splits, mlp_backward_raw, mlp_forward_raw, output_view
    lay = ArenaLayout(dims, nets)
    arena = torch.zeros(lay.total, device=dev)
    params = []
    for n in range(nets):
        net = []
        for l in range(lay.n_layers):
            bound = 1.0 / np.sqrt(dims[l])
            w = T(dd.uniform((dims[l + 1], dims[l]), 300 * n + l, -bound, bound)); b = T(dd.uniform((dims[l + 1],), 300 * n + l + 60, -bound, bound))
            lay.weight(arena, n, l).copy_(w); lay.bias(arena, n, l).copy_(b)
            net += [w.clone().requires_grad_(True), b.clone().requires_grad_(True)]
        params.append(net)
    xc = T(dd.uniform((B, dims[0]), 9, -2, 2)).requires_grad_(True)
    x = torch.zeros((B, lay.ld_in), device=dev); x[:, : dims[0]] = xc.detach().to(dev)
    pk = PackedWeights(lay, dev)
    assert (pk.tensor is not None) == fused
    if fused:
        pk.refresh(arena)
    acts = mlp_forward_raw(lay, arena, x, L.ACT_NONE, packed=pk if fused else None, stash_all=True)
    y = output_view(lay, acts, B)
    outs = [ref.mlp_forward_ref(params[n], xc) for n in range(nets)]
    for n in range(nets):
        np.testing.assert_allclose(y[n, :, : dims[-1]].cpu().numpy(), outs[n].detach().numpy(), rtol=1e-5, atol=1e-5)
        assert torch.all(y[n, :, dims[-1]:] == 0)
    # the hidden stashes: ELU of each hidden layer, against the same torch ops
    for n in range(nets):
        h = xc.detach()
        for l in range(lay.n_layers - 1):
            h = torch.nn.functional.elu(torch.nn.functional.linear(h, params[n][2 * l].detach(), params[n][2 * l + 1].detach()))
            off, ld = lay.act_offset(B, n, l)
            got = acts[off: off + B * ld].view(B, ld)
            np.testing.assert_allclose(got[:, : dims[l + 1]].cpu().numpy(), h.numpy(), rtol=1e-5, atol=1e-5, err_msg=f"stash net {n} layer {l}")
    wts = [T(dd.uniform((B, dims[-1]), 70 + n, -1, 1)) for n in range(nets)]
    dy = torch.zeros((nets, B, lay.ld_out), device=dev)
    for n in range(nets):
        dy[n, :, : dims[-1]] = wts[n].to(dev)
    splits = default_splits(B)
    grads = torch.empty_like(arena); dx = torch.empty((B, lay.ld_in), device=dev)
    ws = torch.empty(lay.bwd_ws_floats(B, splits), device=dev)
    mlp_backward_raw(lay, arena, x, acts, dy, ws, grads=grads, splits=splits, dx=dx)
    loss = sum((outs[n] * wts[n]).sum() for n in range(nets))
    gr = torch.autograd.grad(loss, [xc] + [p for net in params for p in net])
    gx = gr[0].numpy()
    np.testing.assert_allclose(dx[:, : dims[0]].cpu().numpy(), gx, rtol=1e-4, atol=2e-5 * (np.abs(gx).max() + 1e-12))
    k = 1
    for n in range(nets):
        for l in range(lay.n_layers):
            gw, gb = gr[k].numpy(), gr[k + 1].numpy(); k += 2
            scale = np.abs(gw).max() + 1e-12
            np.testing.assert_allclose(lay.weight(grads, n, l).cpu().numpy(), gw, rtol=1e-4, atol=2e-5 * scale, err_msg=f"dW net {n} layer {l}")
            np.testing.assert_allclose(lay.bias(grads, n, l).cpu().numpy(), gb, rtol=1e-4, atol=2e-5 * max(scale, np.abs(gb).max()), err_msg=f"db net {n} layer {l}")
    # data-parallel buckets (pqlk_mlp_backward_layers): the same chain run in layer ranges leaves the same gradient bits
    from pql_amd.utils.dp import layer_buckets
    for buckets in (layer_buckets(lay.n_layers), [(l, l) for l in range(lay.n_layers - 1, -1, -1)]):
        g2 = torch.zeros_like(arena)
        for hi, lo in buckets:
            L.check(L.lib.pqlk_mlp_backward_layers(C.byref(lay.desc), L.ptr(arena), L.ptr(x), lay.ld_in, B, L.ptr(acts), L.ptr(dy), None, None,
                                                   None, 0.0, None, L.ptr(g2), splits, L.ptr(ws), ws.numel(), hi, lo, L.stream(dev)))
        for n in range(nets):
            for l in range(lay.n_layers):
                assert torch.equal(lay.weight(g2, n, l), lay.weight(grads, n, l)) and torch.equal(lay.bias(g2, n, l), lay.bias(grads, n, l)), (buckets, n, l)


# =========================================================================== learners at 101 atoms
O_, A_, B_, CAP_, K_, HIDDEN_ = 8, 2, 64, 400, 101, [64, 64]


def _cfg(graph=False, extra=()):
    from pql_amd.utils.cfg import load_cfg
    cfg = load_cfg([f"algo.batch_size={B_}", f"algo.memory_size={CAP_}", "algo.distl=True", f"algo.num_atoms={K_}", "algo.v_learner_gpu=0",
                    "algo.p_learner_gpu=0", "algo.num_gpus=1", f"algo.graph={graph}", "algo.nstep=3", "algo.streams=False", *extra])
    cfg.algo.hidden_layers = list(HIDDEN_)
    return cfg


def _learner_data():
    rows = CAP_ - 100
    data = (T(dd.uniform((rows, O_), 177, -3, 3)), T(dd.uniform((rows, A_), 178)), T(dd.uniform((rows, 1), 179, -2.0, 2.0)),
            T(dd.uniform((rows, O_), 180, -3, 3)), T(dd.bernoulli((rows, 1), 181, 0.1)))
    return rows, data, T(dd.uniform((O_,), 811, -0.5, 0.5)), T(dd.uniform((O_,), 812, 0.5, 2.0))


def _make_learners(dev, graph):
    from pql_amd.algo.pql_p_learner import PQLPLearner
    from pql_amd.algo.pql_v_learner import PQLVLearner
    cfg = _cfg(graph)
    v = PQLVLearner((O_,), A_, cfg); p = PQLPLearner((O_,), A_, cfg)
    assert v.critic.num_atoms == K_ and v.critic.layout.dims == [O_ + A_, *HIDDEN_, K_] and v.critic.layout.ld_out == 128
    cst = dd.doubleq_state(O_, A_, K_, 41, hidden=tuple(HIDDEN_)); ast = dd.mlp_state(O_, A_, 43, hidden=tuple(HIDDEN_))
    v.critic.load_state_dict(_sd(cst)); v.critic_target.arena.data.copy_(v.critic.arena.data)
    p.actor.load_state_dict(_sd(ast))
    rows, data, mean, var = _learner_data()
    norm = (mean.to(dev), var.to(dev), 1e-4)
    critic, _, _ = v.update(p.actor, tuple(t.to(dev) for t in data), norm, 0)
    p.update(critic, data[0].to(dev), norm, 0)
    return v, p, cst, ast


def test_learners_at_101_atoms_vs_oracle(dev, ref):
    """Pattern and tolerances of test_cfg4_pqld_shadowhand_shape_learner_steps_vs_oracle at O = 8, A = 2, B = 64, hidden [64, 64],
    ring 400: two V steps and two P steps against the CPU oracle on identical indices and noise."""
    v, p, cst, ast = _make_learners(dev, graph=False)
    rows, data, mean, var = _learner_data()
    hp = ref.HyperRef(batch_size=B_, distl=True, num_atoms=K_)
    vr = ref.VLearnerRef(O_, A_, hp, CAP_, ref.params_from_state(cst, "net_q1.net."), ref.params_from_state(cst, "net_q2.net."))
    pr = ref.PLearnerRef(O_, A_, hp, CAP_, ref.params_from_state(ast))
    vr.update(ref.params_from_state(ast), data, (mean, var, 1e-4))
    pr.update(vr.q1, vr.q2, data[0], (mean, var, 1e-4))
    for s in range(2):
        idx = T(dd.integers((B_,), 920 + s, rows)); draw = T(dd.uniform((B_, A_), 970 + s, -2, 2))
        lv = vr.learn(idx=idx, draw=draw)
        v.learn(indices=idx, noise=draw)
        v.synchronize()
        np.testing.assert_allclose(v.loss_ring[s % 5].item(), lv, rtol=2e-5)
        lp = pr.learn(idx=idx)
        p.learn(indices=idx)
        p.synchronize()
        np.testing.assert_allclose(p.loss_ring[s % 5].item(), lp, rtol=2e-5, atol=1e-6)
    _compare_nets(v.critic, (vr.q1, vr.q2))
    _compare_nets(v.critic_target, (vr.t1, vr.t2))
    _compare_nets(p.actor, (pr.actor,))


def test_learners_at_101_atoms_graph_replay_equals_eager(dev):
    """algo.graph=True replays the same launch sequence: bit-equal arenas and loss rings after two V and two P steps."""
    outs = []
    for graph in (False, True):
        v, p, _, _ = _make_learners(dev, graph)
        v.use_private_rng(1234); p.use_private_rng(4321)
        for _ in range(2):
            v.learn()
            p.learn()
        torch.cuda.synchronize()
        assert bool(torch.isfinite(v.loss_ring[:2]).all()) and bool(torch.isfinite(p.loss_ring[:2]).all())
        outs.append((v.critic.arena.data.clone(), v.critic_target.arena.data.clone(), v.loss_ring.clone(), p.actor.arena.data.clone(),
                     p.loss_ring.clone()))
    for a, b in zip(*outs):
        assert torch.equal(a, b)
    assert not torch.equal(outs[0][0], outs[0][1])      # the critic moved away from its target: steps were taken


def test_bf16_targets_refuse_more_than_64_atoms_at_construction(dev):
    from pql_amd.algo.pql_v_learner import PQLVLearner
    with pytest.raises(ValueError, match="64"):
        PQLVLearner((O_,), A_, _cfg(extra=["algo.target_dtype=bfloat16"]))


# =========================================================================== entry point
def test_train_pql_entry_point_at_101_atoms(dev):
    """scripts/train_pql.py on SwingUp with a 101-atom critic (method of test_train_pql_entry_point): it ran to the end, kept the
    design ratios, and both losses are finite."""
    import importlib.util
    import os
    from pql_amd.utils.cfg import load_cfg
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("train_pql", os.path.join(root, "scripts", "train_pql.py"))
    mod = importlib.util.module_from_spec(spec); spec.loader.exec_module(mod)
    cfg = load_cfg(["task=swingup", "num_envs=64", "algo.batch_size=256", "algo.hidden_layers=[128, 128]", "algo.memory_size=20000",
                    "algo.num_gpus=1", "algo.distl=True", "algo.num_atoms=101", "max_step=6000", "algo.graph=True"])
    out = mod.main(cfg)
    iters = (out["global_steps"] - 64 * 32) // 64
    assert iters > 0 and out["critic_updates"] == 8 * iters and out["actor_updates"] == 4 * iters
    assert np.isfinite(out["critic_loss"]) and np.isfinite(out["actor_loss"])
