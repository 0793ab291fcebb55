"""Loss, optimiser and statistics kernels past their grid caps, at the shapes where they take another path, and on inputs that
reach their clamps.  Inputs, references and the table of shapes: tests/reduction_cases.py (what they guarantee is proved
without a GPU in tests/test_reduction_cases_cpu.py).

Every buffer a kernel writes has SLACK floats of poison behind it (and poison pad columns where it has a leading dimension):
the poison must come back bit-identical where include/pqlk.h leaves the place alone and as zero where it says "written as
zero".  Every input has the same slack, filled with a value that would move the result (1.0 under the exact-integer designs,
1e6 elsewhere), so an over-read is a wrong number.  Section A asserts equality: the library is built with -ffp-contract=off
and the sums are exact in fp32 in any order.  Section B uses the bars of the existing test each one names."""
import ctypes as C

import numpy as np
import pytest
import torch

import detdata as dd
import reduction_cases as rc
from guarded import Guarded
from support import dev  # noqa: F401

pytestmark = pytest.mark.gpu

T = rc.T
F32 = np.float32
POISON, SLACK = rc.POISON, rc.SLACK


@pytest.fixture(scope="module")
def ref():
    from oracle import pql_ref_cpu
    return pql_ref_cpu


def _g(dev, arr, fill, off=0):
    arr = arr if torch.is_tensor(arr) else T(np.asarray(arr))
    return Guarded(dev, tuple(arr.shape), fill, arr, off)


def _col0(dev, vals, ld, fill):
    """(2, B) values -> guarded (2, B, ld) with the values in column 0 and `fill` in the other columns."""
    g = Guarded(dev, (*vals.shape, ld), fill)
    g.t[..., 0] = T(vals).to(dev)
    return g


def _step(dev):
    return torch.zeros(1, dtype=torch.int32, device=dev)


# =========================================================================== A. exact sums
@pytest.mark.parametrize("B", rc.TD_B)
def test_td_mse_exact(dev, B):
    """A1: every row counted once -> the loss is fp32(S) / B to the bit, dy the fp32 expression, pads still zero; the partials
    left for the optimiser (loss_out = NULL) sum to S; the ring slot is *slot_dev % ring_len."""
    from pql_amd import _lib as L
    q, qt, rew, done, gn = rc.td_inputs(B)
    terms, S, loss, dy_ref = rc.td_reference(q, qt, rew, done, gn, B)
    ld = 32
    qd, qtd = _col0(dev, q, ld, rc.IN_ONE), _col0(dev, qt, ld, rc.IN_ONE)
    rd, dd_ = _g(dev, rew, rc.IN_ONE), _g(dev, done, rc.IN_ONE)
    parts = int(L.lib.pqlk_loss_parts(B, 1))

    def run(lo, slot, ring_len):
        dy = Guarded(dev, (2, B, ld), POISON); dy.t.zero_()
        scr = Guarded(dev, (parts,), POISON)
        L.check(L.lib.pqlk_td_mse_loss(qd.ptr, qtd.ptr, ld, rd.ptr, dd_.ptr, gn, B, dy.ptr, lo.ptr if lo else None,
                                       L.ptr(slot), ring_len, scr.ptr, L.stream(dev)))
        assert torch.equal(dy.t[:, :, 0].cpu(), T(dy_ref)), "dy column 0"
        assert torch.count_nonzero(dy.t[:, :, 1:]) == 0 and dy.intact() and scr.intact()
        assert scr.t.double().sum().item() == S, "per-block partials"
        return scr

    lo = Guarded(dev, (1,), POISON)
    run(lo, None, 0)
    assert lo.t.item() == float(loss) and lo.intact()
    run(None, None, 0)
    ring = Guarded(dev, (3,), POISON)
    run(ring, torch.tensor([7], dtype=torch.int32, device=dev), 3)
    assert ring.t.cpu().tolist() == [POISON, float(loss), POISON] and ring.intact()


@pytest.mark.parametrize("B", rc.TD_B)
def test_dpg_scalar_exact(dev, B):
    """A2: loss, gradient (g, g / 2 on a tie, 0) and the owner byte of every row; owner = NULL changes nothing else."""
    from pql_amd import _lib as L
    q = rc.dpg_scalar_inputs(B)
    mins, S, loss, dy_ref, owner_ref = rc.dpg_scalar_reference(q, B)
    ld = 32
    qd = _col0(dev, q, ld, rc.IN_ONE)
    parts = int(L.lib.pqlk_loss_parts(B, 1))
    outs = []
    for with_owner in (True, False):
        dy = Guarded(dev, (2, B, ld), POISON); dy.t.zero_()
        lo, scr = Guarded(dev, (1,), POISON), Guarded(dev, (parts,), POISON)
        owner = Guarded(dev, (B,), 0xAA, dtype=torch.uint8)
        if with_owner:
            L.check(L.lib.pqlk_dpg_loss_owner(qd.ptr, ld, 1, None, B, dy.ptr, lo.ptr, None, 0, scr.ptr, owner.ptr, L.stream(dev)))
            assert torch.equal(owner.t.cpu(), T(owner_ref))
        else:
            L.check(L.lib.pqlk_dpg_loss(qd.ptr, ld, 1, None, B, dy.ptr, lo.ptr, None, 0, scr.ptr, L.stream(dev)))
            assert bool((owner.t == 0xAA).all())
        assert lo.t.item() == float(loss)
        assert torch.equal(dy.t[:, :, 0].cpu(), T(dy_ref))
        assert torch.count_nonzero(dy.t[:, :, 1:]) == 0
        assert dy.intact() and lo.intact() and scr.intact() and owner.intact()
        assert scr.t.double().sum().item() == S
        outs.append((dy.t.clone(), lo.t.clone(), scr.t.clone()))
    for a, b in zip(*outs):
        assert torch.equal(a, b)


def test_adamw_norm_pass_counts_every_element_once(dev, ref):
    """A3: sixteen ones at the seams of k_sumsq's three trips, of k_adamw's two and in the 3-element tail -> ||g|| = 4 exactly;
    then the whole update against the oracle at test_clip_adamw_polyak_trace's bars."""
    from pql_amd import _lib as L
    n = rc.ADAM_N_EXACT
    g = T(rc.adam_exact_grad(n))
    p0 = T(dd.uniform((n,), 61, -0.1, 0.1)); t0 = T(dd.uniform((n,), 62, -0.1, 0.1))
    opt = ref.AdamWRef([p0.clone()], lr=5e-4); tgt = [t0.clone()]
    opt.apply([g.clone()], 2.0)
    ref.polyak_ref(tgt, opt.params, 0.05)
    gd = _g(dev, g, rc.IN_ONE)
    p, tg = _g(dev, p0, POISON), _g(dev, t0, POISON)
    m, v = Guarded(dev, (n,), POISON), Guarded(dev, (n,), POISON)
    m.t.zero_(); v.t.zero_()
    step, gn, scr = _step(dev), Guarded(dev, (1,), POISON), Guarded(dev, (2048,), POISON)
    L.check(L.lib.pqlk_clip_adamw_polyak(p.ptr, gd.ptr, m.ptr, v.ptr, tg.ptr, n, 1.0, 2.0, 5e-4, 0.9, 0.999, 1e-8, 1e-2, 0.05,
                                         L.ptr(step), gn.ptr, scr.ptr, L.stream(dev)))
    assert gn.t.item() == 4.0 and step.item() == 1
    np.testing.assert_allclose(p.t.cpu().numpy(), opt.params[0].numpy(), rtol=2e-6, atol=1e-8)
    np.testing.assert_allclose(m.t.cpu().numpy(), opt.m[0].numpy(), rtol=1e-5, atol=1e-9)
    np.testing.assert_allclose(v.t.cpu().numpy(), opt.v[0].numpy(), rtol=1e-5, atol=1e-12)
    np.testing.assert_allclose(tg.t.cpu().numpy(), tgt[0].numpy(), rtol=2e-6, atol=1e-8)
    assert np.array_equal(m.t.cpu().numpy() != 0, g.numpy() != 0)        # the sixteen, where they were put
    for b in (p, m, v, tg, gn, scr, gd):
        assert b.intact()


@pytest.mark.parametrize("tau", [0.05, 1.0, 0.0])
@pytest.mark.parametrize("n", rc.POLYAK_N)
def test_polyak_exact(dev, n, tau):
    """A4: bit-equal to cur * fp32(tau) + target * fp32(1 - tau), through the second, ragged trip."""
    from pql_amd import _lib as L
    cur, tgt = dd.uniform((n,), 871, -1, 1), dd.uniform((n,), 872, -1, 1)
    want = rc.polyak_reference(cur, tgt, tau)
    cd, td = _g(dev, cur, rc.IN_BIG), _g(dev, tgt, POISON)
    L.check(L.lib.pqlk_polyak(td.ptr, cd.ptr, n, tau, L.stream(dev)))
    assert torch.equal(td.t.cpu(), T(want)) and td.intact() and cd.intact()
    if tau == 1.0:
        assert torch.equal(td.t, cd.t)


@pytest.mark.parametrize("b", rc.ALPHA_B)
def test_sac_alpha_terms_exact(dev, b):
    """A5: integer logp and log_alpha = 0 (alpha exactly 1): both outputs are -(sum / b) - target_entropy to the bit, the ring
    slot gains sum / b, the other slots stay; either output pointer may be NULL.  Then log_alpha = log 0.2 against float64."""
    from pql_amd import _lib as L
    logp = rc.ints((b,), 851 + b, -8, 8)
    te, prev = -6.0, 2.5
    S, g_ref, ring_ref = rc.alpha_reference(logp, b, te, prev)
    lpd = _g(dev, logp, rc.IN_ONE)
    la = torch.zeros(1, device=dev)
    slot = torch.tensor([7], dtype=torch.int32, device=dev)
    for with_grad, with_loss, with_ring, with_slot in ((1, 1, 1, 1), (0, 1, 1, 0), (1, 0, 1, 1), (1, 1, 0, 0)):
        go, ao = Guarded(dev, (1,), POISON), Guarded(dev, (1,), POISON)
        ring = Guarded(dev, (3,), POISON); ring.t.fill_(prev)
        L.check(L.lib.pqlk_sac_alpha_terms(lpd.ptr, b, L.ptr(la), te, go.ptr if with_grad else None, ao.ptr if with_loss else None,
                                           ring.ptr if with_ring else None, L.ptr(slot) if with_slot else None, 3, L.stream(dev)))
        assert go.full[0].item() == (float(g_ref) if with_grad else POISON)
        assert ao.full[0].item() == (float(g_ref) if with_loss else POISON)
        want = [prev] * 3
        if with_ring:
            want[1 if with_slot else 0] = float(ring_ref)
        assert ring.t.cpu().tolist() == want
        assert go.intact() and ao.intact() and ring.intact()
    la.fill_(float(np.log(0.2)))
    go, ao, ring = Guarded(dev, (1,), POISON), Guarded(dev, (1,), POISON), Guarded(dev, (3,), POISON)
    ring.t.fill_(prev)
    L.check(L.lib.pqlk_sac_alpha_terms(lpd.ptr, b, L.ptr(la), te, go.ptr, ao.ptr, ring.ptr, None, 3, L.stream(dev)))
    alpha, mean = np.exp(np.float64(F32(np.log(0.2)))), S / b
    # three or four fp32 roundings and a 1-ulp expf; one dropped row moves the mean by at least 1 / b >= 3e-4
    np.testing.assert_allclose(go.t.item(), alpha * (-mean - te), rtol=1e-6)
    assert ao.t.item() == go.t.item()
    np.testing.assert_allclose(ring.t[0].item(), prev + alpha * mean, rtol=1e-6)
    assert ring.t[1:].cpu().tolist() == [prev, prev]


@pytest.mark.parametrize("b", rc.SHIFT_B)
def test_sac_entropy_shift_exact(dev, b):
    """A5: column 0 of both nets becomes qt - logp to the bit; columns 1..31 keep their poison."""
    from pql_amd import _lib as L
    ld = 32
    qt, logp = rc.ints((2, b), 881 + b, -8, 8), rc.ints((b,), 882 + b, -8, 8)
    qd = _col0(dev, qt, ld, POISON)
    lpd = _g(dev, logp, rc.IN_ONE)
    la = torch.zeros(1, device=dev)
    L.check(L.lib.pqlk_sac_entropy_shift(qd.ptr, ld, b * ld, 2, lpd.ptr, L.ptr(la), b, L.stream(dev)))
    assert torch.equal(qd.t[:, :, 0].cpu(), T(qt - logp[None, :]))
    assert bool((qd.t[:, :, 1:] == POISON).all()) and qd.intact()


# =========================================================================== B. shape sweeps
_C51_REF = {}


def _c51_case(ref, B, K, v_min, v_max, saturated):
    """(inputs, reference) computed once per case and shared; nobody writes to them."""
    key = (B, K, v_min, v_max, saturated)
    if key not in _C51_REF:
        inp = rc.c51_inputs(B, K, v_min, v_max, saturated)
        _C51_REF[key] = (inp, rc.c51_reference(ref, *inp, K, v_min, v_max))
    return _C51_REF[key]


def _c51_check(dev, ref, B, K, ld, v_min=-10.0, v_max=10.0, saturated=False):
    from pql_amd import _lib as L
    (lg, lt, rew, done, gn), (tgt, loss, grad) = _c51_case(ref, B, K, v_min, v_max, saturated)

    def padded(x):
        g = Guarded(dev, (2, B, ld), rc.IN_BIG)
        g.t[:, :, :K] = x.to(dev)
        return g

    lgd, ltd = padded(lg), padded(lt)
    rd, dd_ = _g(dev, rew.view(-1), rc.IN_BIG), _g(dev, done.view(-1), rc.IN_BIG)
    zd = _g(dev, torch.linspace(v_min, v_max, K), rc.IN_BIG)
    parts = int(L.lib.pqlk_loss_parts(B, K))
    outs = []
    for with_proj in (True, False):
        dy, lo, scr = Guarded(dev, (2, B, ld), POISON), Guarded(dev, (1,), POISON), Guarded(dev, (parts,), POISON)
        pj = Guarded(dev, (B, K), POISON)
        L.check(L.lib.pqlk_c51_bce_loss(lgd.ptr, ltd.ptr, ld, K, rd.ptr, dd_.ptr, zd.ptr, gn, v_min, v_max, B, dy.ptr, lo.ptr, None, 0,
                                        pj.ptr if with_proj else None, scr.ptr, L.stream(dev)))
        for b in (dy, lo, scr, pj):
            assert b.intact()
        outs.append((dy.t.clone(), lo.t.clone()))
        if not with_proj:
            assert bool((pj.t == POISON).all())
            continue
        np.testing.assert_allclose(pj.t.cpu().numpy(), tgt.numpy(), atol=2e-7)
        np.testing.assert_allclose(lo.t.item(), loss.item(), rtol=5e-6)
        np.testing.assert_allclose(dy.t[:, :, :K].cpu().numpy(), grad.numpy(), rtol=2e-4, atol=2e-9)
        assert torch.count_nonzero(dy.t[:, :, K:]) == 0          # pads written as zero
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])      # proj_out = NULL changes nothing
    return outs[0][0]


@pytest.mark.parametrize("K,ld", rc.C51_SHAPES)
def test_c51_bce_shapes(dev, ref, K, ld):
    """B1: K = 2, every lane valid (64, and 32 under ld = 32), and the c >= 64 pad loop (ld = 128), at the bars of test_c51_bce_loss."""
    _c51_check(dev, ref, 37, K, ld)


def test_c51_bce_other_support(dev, ref):
    _c51_check(dev, ref, 37, 33, 64, -2.0, 6.0)


@pytest.mark.parametrize("K", [51, 64])
@pytest.mark.parametrize("B", rc.C51_B)
def test_c51_bce_batches(dev, ref, B, K):
    """B1: fewer rows than a block has waves, and a third, ragged trip of the capped grid."""
    _c51_check(dev, ref, B, K, 64)


@pytest.mark.parametrize("K", [51, 64])
def test_c51_bce_saturated_rows(dev, ref, K):
    """B2: rows whose softmax is 1.0 on one atom and 8.76e-27 (gap 60) or 0 (gap 120) elsewhere: max(log p, -100) and
    max((1 - p) p, 1e-12) bind.  The reference's gradient there is below 1e-16; without the second clamp the kernel would return
    t / (B K) ~ 1e-5 or NaN, without the first Inf."""
    dy = _c51_check(dev, ref, 37, K, 64, saturated=True)
    hard = [i for i, gap in enumerate(rc.SAT_GAPS) if gap >= 60]
    assert bool(torch.isfinite(dy).all()) and float(dy[:, hard].abs().max()) < 2e-9


@pytest.mark.parametrize("B,K,ld", [(37, K, ld) for K, ld in rc.C51_SHAPES] + [(rc.C51_B_BIG, 51, 64)])
def test_dpg_dist_shapes(dev, B, K, ld):
    """B3: the distributional DPG loss over the same (K, ld) list and past the grid cap, at the bars of test_dpg_loss."""
    from pql_amd import _lib as L
    q = rc.dpg_dist_inputs(B, K)
    z, loss, grad = rc.dpg_dist_reference(q, K)
    qd = Guarded(dev, (2, B, ld), rc.IN_BIG); qd.t[:, :, :K] = q.to(dev)
    zd = _g(dev, z, rc.IN_BIG)
    dy, lo = Guarded(dev, (2, B, ld), POISON), Guarded(dev, (1,), POISON)
    scr = Guarded(dev, (int(L.lib.pqlk_loss_parts(B, K)),), POISON)
    L.check(L.lib.pqlk_dpg_loss(qd.ptr, ld, K, zd.ptr, B, dy.ptr, lo.ptr, None, 0, scr.ptr, L.stream(dev)))
    np.testing.assert_allclose(lo.t.item(), loss.item(), rtol=5e-6)
    np.testing.assert_allclose(dy.t[:, :, :K].cpu().numpy(), grad.numpy(), rtol=5e-5, atol=1e-9)
    assert torch.count_nonzero(dy.t[:, :, K:]) == 0
    assert dy.intact() and lo.intact() and scr.intact()


def test_c51_project_past_the_grid_cap(dev, ref):
    """B4: 16,384 + 7 rows; half of them terminal, a quarter with the reward on an atom (lo == up before the fix-up)."""
    from pql_amd import _lib as L
    p, rew, done, gn, grid = rc.project_inputs()
    B, K = p.shape
    want = ref.c51_project_ref(p, rew, done, gn, -10, 10, K).numpy()
    pd, rd, dd_ = _g(dev, p, rc.IN_BIG), _g(dev, rew.view(-1), rc.IN_BIG), _g(dev, done.view(-1), rc.IN_BIG)
    zd = _g(dev, torch.linspace(-10, 10, K), rc.IN_BIG)
    out = Guarded(dev, (B, K), POISON)
    L.check(L.lib.pqlk_c51_project(pd.ptr, rd.ptr, dd_.ptr, zd.ptr, gn, -10.0, 10.0, K, B, out.ptr, L.stream(dev)))
    got = out.t.cpu().numpy()
    np.testing.assert_allclose(got, want, atol=1e-7)
    assert np.array_equal(got != 0, want != 0)
    assert out.intact()


@pytest.mark.parametrize("cols", rc.MOMENTS_COLS)
@pytest.mark.parametrize("n", rc.MOMENTS_N)
def test_batch_moments_shapes(dev, n, cols):
    """B5: one, two, three and 64 chunks, a last chunk of one and of two rows, column counts around the 32-wide tile, ldx > cols;
    float64 statistics of the same fp32 inputs at the bars of test_batch_moments."""
    from pql_amd import _lib as L
    ldx = cols + 5
    x = rc.moments_inputs(n, cols, ldx)
    mean_ref, var_ref = rc.moments_reference(x, cols)
    xd = _g(dev, x, rc.IN_BIG)
    mo, vo, scr = Guarded(dev, (cols,), POISON), Guarded(dev, (cols,), POISON), Guarded(dev, (64 * cols * 3,), POISON)
    L.check(L.lib.pqlk_batch_moments(xd.ptr, ldx, n, cols, mo.ptr, vo.ptr, scr.ptr, L.stream(dev)))
    np.testing.assert_allclose(mo.t.cpu().numpy(), mean_ref, rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(vo.t.cpu().numpy(), var_ref, rtol=1e-5)
    assert mo.intact() and vo.intact() and scr.intact()


def test_batch_moments_constant_and_offset_columns(dev):
    """B5: a constant column (mean 3.0 to the bit, variance exactly 0) and a column 1000 + 0.01 U(-1, 1), whose bar is eight
    times the error of torch's own fp32 CPU x.var(0) on it (the kernel's 64-way Chan tree and torch's cascade round differently
    but are the same class of algorithm), or rtol 1e-5 if that is larger.
    Measured relative errors of the variance of that column: torch fp32 on the CPU 8.0e-6, the kernel 9.4e-9
    (7.4e-4 before k_moments_stage1 subtracted the column's first row: every chunk mean was rounded to the ulp of 1000)."""
    from pql_amd import _lib as L
    n = 4097
    x, cols = rc.moments_extra_inputs(n)
    mean_ref, var_ref = rc.moments_reference(x, cols)
    xd = _g(dev, x, rc.IN_BIG)
    mo, vo, scr = Guarded(dev, (cols,), POISON), Guarded(dev, (cols,), POISON), Guarded(dev, (64 * cols * 3,), POISON)
    L.check(L.lib.pqlk_batch_moments(xd.ptr, x.shape[1], n, cols, mo.ptr, vo.ptr, scr.ptr, L.stream(dev)))
    mean, var = mo.t.cpu().numpy(), vo.t.cpu().numpy()
    np.testing.assert_allclose(mean[:-2], mean_ref[:-2], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(var[:-2], var_ref[:-2], rtol=1e-5)
    assert mean[-2] == 3.0 and var[-2] == 0.0
    torch_err = abs(T(x[:, cols - 1]).var(0).item() - var_ref[-1]) / var_ref[-1]
    kernel_err = abs(float(var[-1]) - var_ref[-1]) / var_ref[-1]
    print(f"offset column: torch fp32 var rel err {torch_err:.3e}, kernel {kernel_err:.3e}")
    assert kernel_err <= max(8 * torch_err, 1e-5)
    np.testing.assert_allclose(mean[-1], mean_ref[-1], rtol=1e-5, atol=1e-6)
    assert mo.intact() and vo.intact() and scr.intact()


@pytest.mark.parametrize("cols", rc.BN_COLS)
@pytest.mark.parametrize("m", rc.BN_M)
def test_bn_elu_forward_shapes(dev, m, cols):
    """B6: fewer rows than row chunks, ragged chunks, widths around the 64-column block, ld > cols; training mode at the bar of
    test_batchnorm_critic_forward_golden with the running statistics updated from non-trivial values, then eval mode on
    statistics it must not touch."""
    from pql_amd import _lib as L
    ld = cols + 3
    z, zz, gamma, beta, mean, var, rm0, rv0 = rc.bn_inputs(m, cols, ld)
    zd, gd, bd = _g(dev, z, rc.IN_BIG), _g(dev, gamma, rc.IN_BIG), _g(dev, beta, rc.IN_BIG)
    md, vd = _g(dev, mean, rc.IN_BIG), _g(dev, var, rc.IN_BIG)
    rm, rv, y = _g(dev, rm0, POISON), _g(dev, rv0, POISON), Guarded(dev, (m, ld), POISON)
    L.check(L.lib.pqlk_bn_elu_forward(zd.ptr, ld, m, cols, md.ptr, vd.ptr, gd.ptr, bd.ptr, 1e-5, 1, 0.1, rm.ptr, rv.ptr, y.ptr,
                                      L.stream(dev)))
    np.testing.assert_allclose(y.t[:, :cols].cpu().numpy(), rc.bn_reference(zz, gamma, beta), rtol=1e-5, atol=5e-6)
    z64 = zz.astype(np.float64)
    np.testing.assert_allclose(rm.t.cpu().numpy(), 0.9 * rm0 + 0.1 * z64.mean(0), rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(rv.t.cpu().numpy(), 0.9 * rv0 + 0.1 * z64.var(0, ddof=1), rtol=1e-5, atol=1e-6)
    assert bool((y.t[:, cols:] == POISON).all()) and y.intact() and rm.intact() and rv.intact()
    # eval: the (given) running statistics normalise and stay as they are; mean / var are not read
    rm, rv, y = _g(dev, rm0, POISON), _g(dev, rv0, POISON), Guarded(dev, (m, ld), POISON)
    L.check(L.lib.pqlk_bn_elu_forward(zd.ptr, ld, m, cols, None, None, gd.ptr, bd.ptr, 1e-5, 0, 0.1, rm.ptr, rv.ptr, y.ptr, L.stream(dev)))
    np.testing.assert_allclose(y.t[:, :cols].cpu().numpy(), rc.bn_reference(zz, gamma, beta, running=(rm0, rv0)), rtol=1e-5, atol=5e-6)
    assert torch.equal(rm.t.cpu(), T(rm0)) and torch.equal(rv.t.cpu(), T(rv0))
    assert bool((y.t[:, cols:] == POISON).all()) and y.intact() and rm.intact() and rv.intact()


def _bn_backward(dev, m, cols, dy, beta_shift=0.0, alias=False, no_param_grads=False):
    from pql_amd import _lib as L
    ld = cols + 3
    z, zz, gamma, beta, mean, var, rm0, rv0 = rc.bn_inputs(m, cols, ld, beta_shift)
    y_ref, dz_ref, dg_ref, db_ref = rc.bn_reference(zz, gamma, beta, dy=dy)
    zd, gd, md, vd = _g(dev, z, rc.IN_BIG), _g(dev, gamma, rc.IN_BIG), _g(dev, mean, rc.IN_BIG), _g(dev, var, rc.IN_BIG)
    yd, dyd = Guarded(dev, (m, ld), rc.IN_BIG), Guarded(dev, (m, ld), POISON)
    yd.t[:, :cols] = T(y_ref.astype(F32)).to(dev); dyd.t[:, :cols] = T(dy).to(dev)
    dz = dyd if alias else Guarded(dev, (m, ld), POISON)
    dg, db, scr = Guarded(dev, (cols,), POISON), Guarded(dev, (cols,), POISON), Guarded(dev, (128 * cols,), POISON)
    L.check(L.lib.pqlk_bn_elu_backward(dyd.ptr, yd.ptr, zd.ptr, ld, m, cols, md.ptr, vd.ptr, gd.ptr, 1e-5, dz.ptr,
                                       None if no_param_grads else dg.ptr, None if no_param_grads else db.ptr, scr.ptr, L.stream(dev)))
    bar = lambda r: dict(rtol=2e-5, atol=2e-5 * float(np.abs(r).max()))  # noqa: E731  the gradient bar of tests/test_ppo_gpu.py
    np.testing.assert_allclose(dz.t[:, :cols].cpu().numpy(), dz_ref, **bar(dz_ref))
    if no_param_grads:
        assert bool((dg.t == POISON).all()) and bool((db.t == POISON).all())
    else:
        np.testing.assert_allclose(dg.t.cpu().numpy(), dg_ref, **bar(dg_ref))
        np.testing.assert_allclose(db.t.cpu().numpy(), db_ref, **bar(db_ref))
    assert bool((dz.t[:, cols:] == POISON).all())
    for b in (dz, dg, db, scr, dyd):
        assert b.intact()
    return db.t.cpu().numpy(), y_ref


@pytest.mark.parametrize("cols", rc.BN_COLS)
@pytest.mark.parametrize("m", rc.BN_M)
def test_bn_elu_backward_shapes(dev, m, cols):
    """B6: dz, dgamma, dbeta against float64 autograd of F.elu(F.batch_norm(z, training=True))."""
    _bn_backward(dev, m, cols, dd.uniform((m, cols), 37 + m + cols, -1, 1))


def test_bn_elu_backward_in_place_and_without_parameter_gradients(dev):
    _bn_backward(dev, 65, 130, dd.uniform((65, 130), 38, -1, 1), alias=True)
    _bn_backward(dev, 65, 130, dd.uniform((65, 130), 38, -1, 1), no_param_grads=True)


def test_bn_elu_backward_integer_dbeta_is_exact(dev):
    """B6: every y > 0 (beta ~ 20) and integer dy: dbeta is an integer column sum, exact in any order."""
    dy = rc.ints((257, 65), 861, -4, 4)
    db, y_ref = _bn_backward(dev, 257, 65, dy, beta_shift=20.0)
    assert y_ref.min() > 0
    assert np.array_equal(db.astype(np.float64), dy.astype(np.float64).sum(0))


@pytest.mark.parametrize("B", rc.SG_B)
@pytest.mark.parametrize("A", rc.SG_A)
def test_sg_head_shapes(dev, A, B):
    """B7: the squashed-Gaussian head forward and backward against float64 of the formula in include/pqlk.h and its autograd:
    A below, between and at powers of two, a row group straddling blocks, |u| in the hundreds, raw log_std outside +-5."""
    from pql_amd import _lib as L
    ld_y, ld_act, ld_da = 2 * A + 3, A + 2, A + 5
    y, mu, ls, eps = rc.sg_inputs(B, A, ld_y)
    a_ref, logp_ref, u = rc.sg_reference(mu, ls, eps)
    yd, ed = _g(dev, y, rc.IN_BIG), _g(dev, eps, rc.IN_BIG)
    act, logp = Guarded(dev, (B, ld_act), POISON), Guarded(dev, (B,), POISON)
    L.check(L.lib.pqlk_sg_head_forward(yd.ptr, ld_y, ed.ptr, B, A, act.ptr, ld_act, logp.ptr, L.stream(dev)))
    np.testing.assert_allclose(act.t[:, :A].cpu().numpy(), a_ref, rtol=1e-6)
    got = logp.t.cpu().numpy()
    assert np.isfinite(got).all()
    np.testing.assert_allclose(got, logp_ref, rtol=1e-5, atol=1e-5 * A)
    assert bool((act.t[:, A:] == POISON).all()) and act.intact() and logp.intact()
    # deterministic action: eps = NULL, logp not written
    act2, logp2 = Guarded(dev, (B, ld_act), POISON), Guarded(dev, (B,), POISON)
    L.check(L.lib.pqlk_sg_head_forward(yd.ptr, ld_y, None, B, A, act2.ptr, ld_act, logp2.ptr, L.stream(dev)))
    np.testing.assert_allclose(act2.t[:, :A].cpu().numpy(), np.tanh(mu.astype(np.float64)), rtol=1e-6)
    assert bool((logp2.t == POISON).all()) and bool((act2.t[:, A:] == POISON).all()) and act2.intact() and logp2.intact()
    # backward of sum(da * a) + glp * sum(logp), glp = glp_scale * exp(log_alpha)
    da = dd.uniform((B, A), 44 + A + B, -1, 1)
    la = F32(np.log(0.5)); glp_scale = 0.3
    _, dmu_ref, dls_ref = rc.sg_reference(mu, ls, eps, da=da, glp=glp_scale * np.exp(np.float64(la)))
    dad = Guarded(dev, (B, ld_da), rc.IN_BIG); dad.t[:, :A] = T(da).to(dev)
    lad = torch.tensor([float(la)], device=dev)
    dy = Guarded(dev, (B, ld_y), POISON)
    L.check(L.lib.pqlk_sg_head_backward(yd.ptr, ld_y, ed.ptr, act.ptr, ld_act, dad.ptr, ld_da, L.ptr(lad), glp_scale, B, A, dy.ptr,
                                        L.stream(dev)))
    g = dy.t.cpu().numpy()
    np.testing.assert_allclose(g[:, :A], dmu_ref, rtol=2e-5, atol=2e-5 * np.abs(dmu_ref).max())
    np.testing.assert_allclose(g[:, A:2 * A], dls_ref, rtol=2e-5, atol=2e-5 * np.abs(dls_ref).max())
    outside = (ls < -5) | (ls > 5)
    assert np.all(g[:, A:2 * A][outside] == 0) and np.all(dls_ref[outside] == 0)
    assert np.all(g[:, 2 * A:] == 0) and dy.intact()          # pads written as zero


def _adam_run(dev, n, g_list, p0, t0, off=0, grad_scale=1.0, max_norm=0.5, with_target=True, with_gnorm=True):
    from pql_amd import _lib as L
    p, tg = _g(dev, p0, POISON, off), _g(dev, t0, POISON, off)
    m, v = Guarded(dev, (n,), POISON, off=off), Guarded(dev, (n,), POISON, off=off)
    m.t.zero_(); v.t.zero_()
    step, gn, scr = _step(dev), Guarded(dev, (1,), POISON), Guarded(dev, (2048,), POISON)
    norms = []
    for g in g_list:
        gd = _g(dev, g, rc.IN_BIG)
        L.check(L.lib.pqlk_clip_adamw_polyak(p.ptr, gd.ptr, m.ptr, v.ptr, tg.ptr if with_target else None, n, grad_scale, max_norm,
                                             5e-4, 0.9, 0.999, 1e-8, 1e-2, 0.05, L.ptr(step), gn.ptr if with_gnorm else None, scr.ptr,
                                             L.stream(dev)))
        norms.append(gn.t.item())
    for b in (p, tg, m, v, gn, scr):
        assert b.intact()
    assert step.item() == len(g_list)
    return p.t, m.t, v.t, tg.t, norms


@pytest.mark.parametrize("variant", ["grad_scale", "no_clip", "no_target", "no_gnorm"])
def test_adamw_arguments(dev, ref, variant):
    """B8: grad_scale = 0.5, max_norm = 0, target = NULL and gnorm_out = NULL, two dense steps with a 3-element tail, against the
    oracle at test_clip_adamw_polyak_trace's bars."""
    n = rc.ADAM_N_DENSE
    p0 = T(dd.uniform((n,), 61, -0.1, 0.1)); t0 = T(dd.uniform((n,), 62, -0.1, 0.1))
    gs = [T(dd.uniform((n,), 63 + s, -1, 1)) * (10.0 if s == 0 else 1e-3) for s in range(2)]
    scale = 0.5 if variant == "grad_scale" else 1.0
    max_norm = 0.0 if variant == "no_clip" else 0.5
    p, m, v, tg, norms = _adam_run(dev, n, gs, p0, t0, grad_scale=scale, max_norm=max_norm, with_target=variant != "no_target",
                                   with_gnorm=variant != "no_gnorm")
    opt = ref.AdamWRef([p0.clone()], lr=5e-4); tgt = [t0.clone()]
    for s, g in enumerate(gs):
        opt.apply([g * scale], max_norm if max_norm > 0 else None)      # g * 0.5 is exact
        ref.polyak_ref(tgt, opt.params, 0.05)
    np.testing.assert_allclose(p.cpu().numpy(), opt.params[0].numpy(), rtol=2e-6, atol=1e-8)
    np.testing.assert_allclose(m.cpu().numpy(), opt.m[0].numpy(), rtol=1e-5, atol=1e-9)
    np.testing.assert_allclose(v.cpu().numpy(), opt.v[0].numpy(), rtol=1e-5, atol=1e-12)
    if variant == "no_target":
        assert torch.equal(tg.cpu(), t0)
    else:
        np.testing.assert_allclose(tg.cpu().numpy(), tgt[0].numpy(), rtol=2e-6, atol=1e-8)
    if variant == "no_gnorm":
        assert norms == [POISON, POISON]
    else:
        np.testing.assert_allclose(norms[-1], torch.linalg.vector_norm(gs[-1] * scale).item(), rtol=1e-5)


def test_adamw_scalar_path_equals_the_16_byte_path(dev):
    """B8: p, m, v and target one float past a 16-byte boundary (g aligned) send every element through the scalar loop, here into
    its second, ragged trip; the arithmetic is per element, so the bits are those of the aligned run."""
    n = rc.ADAM_N_MISALIGNED
    p0 = T(dd.uniform((n,), 61, -0.1, 0.1)); t0 = T(dd.uniform((n,), 62, -0.1, 0.1))
    gs = [T(dd.uniform((n,), 63 + s, -1, 1)) * (10.0 if s == 0 else 1e-3) for s in range(2)]
    a = _adam_run(dev, n, gs, p0, t0, off=0)
    b = _adam_run(dev, n, gs, p0, t0, off=1)
    for x, y in zip(a[:4], b[:4]):
        assert torch.equal(x, y)
    assert a[4] == b[4]


def test_adamw_pack_scalar_path_refreshes_the_packed_copies(dev):
    """B8: the packed_index branch: with the arena one float off alignment the re-pack goes element by element; the copies must
    equal pqlk_mlp_pack of the new parameters / target, and everything must equal the aligned run."""
    from pql_amd import _lib as L
    from pql_amd.models.mlp import ArenaLayout, PackedWeights
    lay = ArenaLayout(rc.PACK_DIMS, rc.PACK_NETS)
    n = lay.total
    p0 = T(dd.uniform((n,), 1, -0.1, 0.1)); t0 = T(dd.uniform((n,), 2, -0.1, 0.1)); g = T(dd.uniform((n,), 3, -1, 1))
    outs = []
    for off in (0, 1):
        p, tg = _g(dev, p0, POISON, off), _g(dev, t0, POISON, off)
        m, v = Guarded(dev, (n,), POISON, off=off), Guarded(dev, (n,), POISON, off=off)
        m.t.zero_(); v.t.zero_()
        gd, step, scr = _g(dev, g, rc.IN_BIG), _step(dev), Guarded(dev, (2048,), POISON)
        npk = PackedWeights(lay, dev).tensor.numel()
        pk_p, pk_t = Guarded(dev, (npk,), POISON), Guarded(dev, (npk,), POISON)
        L.check(L.lib.pqlk_clip_adamw_polyak_pack(C.byref(lay.desc), p.ptr, gd.ptr, m.ptr, v.ptr, tg.ptr, pk_p.ptr, pk_t.ptr, 1.0, 0.5,
                                                  5e-4, 0.9, 0.999, 1e-8, 1e-2, 0.05, L.ptr(step), None, scr.ptr, L.stream(dev)))
        want_p = PackedWeights(lay, dev).refresh(p.t.clone()).tensor           # clone: an aligned copy
        want_t = PackedWeights(lay, dev).refresh(tg.t.clone()).tensor
        filled = PackedWeights(lay, dev).refresh(torch.ones(n, device=dev)).tensor != 0      # the slots a pack writes
        assert torch.equal(pk_p.t[filled], want_p[filled]) and torch.equal(pk_t.t[filled], want_t[filled])
        assert bool((pk_p.t[~filled] == POISON).all()) and bool((pk_t.t[~filled] == POISON).all())
        for b in (p, tg, m, v, scr, pk_p, pk_t):
            assert b.intact()
        outs.append((p.t, tg.t, m.t, v.t, pk_p.t, pk_t.t))
    for x, y in zip(*outs):
        assert torch.equal(x, y)
