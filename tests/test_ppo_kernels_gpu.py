"""The PPO kernels (pql_amd/csrc/ppo.hip) and the rollout's elementwise kernels at their group, horizon and grid-cap edges,
through the C entry points.  Inputs, references and the table of shapes: tests/ppo_cases.py (what they guarantee is proved
without a GPU in tests/test_ppo_cases_cpu.py).

Every buffer a kernel writes is Guarded: SLACK floats of poison behind it and poison pad columns, which must come back
bit-identical where include/pqlk.h leaves the place alone and as zero where it says "written as zero".  Every input has the
same slack and pad columns, filled with a value that would move the result.  The exact sections assert equality: the library
is built with -ffp-contract=off, the cross-row sums are exact in fp32 in any order and the per-row quantities are fp32 numpy
restatements, op by op.  The dense sections compare with float64 at the bars of the test in tests/test_ppo_gpu.py each one
names, and print the largest error they saw."""
import warnings

import numpy as np
import pytest
import torch

import ppo_cases as pc
from guarded import Guarded
from support import dev  # noqa: F401

pytestmark = pytest.mark.gpu

T, F32 = pc.T, np.float32
POISON, IN_ONE, IN_BIG = pc.POISON, pc.IN_ONE, pc.IN_BIG


def _g(dev, arr, fill, dtype=torch.float32):
    arr = arr if torch.is_tensor(arr) else T(np.asarray(arr))
    return Guarded(dev, tuple(arr.shape), fill, arr, dtype=dtype)


def _padded(dev, arr, ld, fill):
    """(rows, cols) values -> guarded (rows, ld) with `fill` in the pad columns."""
    g = Guarded(dev, (arr.shape[0], ld), fill)
    g.t[:, :arr.shape[1]] = T(np.asarray(arr)).to(dev)
    return g


def _np(t):
    return t.cpu().numpy()


def _all(t, value):
    return bool((t == value).all())


def _err(name, got, want):
    """Largest absolute error, and largest error relative to the reference's largest magnitude."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    e = float(np.abs(got - want).max())
    print(f"{name}: max abs err {e:.3e}, / max|ref| {e / max(float(np.abs(want).max()), 1e-300):.3e}")


# =========================================================================== GAE
@pytest.mark.parametrize("with_timeout", [False, True])
@pytest.mark.parametrize("gae", [True, False])
@pytest.mark.parametrize("Tn", pc.GAE_T)
def test_gae_exact_at_the_unroll_limits(dev, Tn, gae, with_timeout):
    """T on both sides of 8, 16 and 32 and T = 1, each with one column, a ragged block and two blocks, an all-done and a
    never-done column: bit-equal to the reference loop in fp32; the slack behind adv and ret keeps its poison."""
    from pql_amd import _lib as L
    for n in pc.GAE_N:
        c = pc.gae_inputs(Tn, n)
        tmo = c["tmo"] if with_timeout else None
        want = pc.gae_reference(c["rew"], c["done"], c["val"], c["nv"], c["nd"], 0.99, 0.95, gae, tmo)
        ins = {k: _g(dev, c[k], IN_BIG) for k in ("rew", "done", "val", "nv", "nd", "tmo")}
        adv, ret = Guarded(dev, (Tn, n), POISON), Guarded(dev, (Tn, n), POISON)
        L.check(L.lib.pqlk_gae(ins["rew"].ptr, ins["done"].ptr, ins["val"].ptr, ins["nv"].ptr, ins["nd"].ptr,
                               ins["tmo"].ptr if with_timeout else None, Tn, n, 0.99, 0.95, int(gae), adv.ptr, ret.ptr, L.stream(dev)))
        assert torch.equal(adv.t.cpu(), T(want[0])), (n, "adv")
        assert torch.equal(ret.t.cpu(), T(want[1])), (n, "ret")
        assert adv.intact() and ret.intact(), n


# =========================================================================== Gaussian head
@pytest.mark.parametrize("B", pc.HEAD_B)
@pytest.mark.parametrize("A", pc.HEAD_A)
def test_gauss_head_exact(dev, A, B):
    """logstd = 0: act == mean + eps, logp the index-order fp32 row sum, ent A additions of the constant; eps = NULL gives the
    mean; logp = NULL / ent = NULL leave their buffers alone; the pad columns of act (ld_act > A) are never written."""
    from pql_amd import _lib as L
    c = pc.head_inputs(A, B)
    mu, eps = c["mu"], c["eps"]
    ld_y, ld_act = A + 3, A + 2
    yd, ed, lsd = _padded(dev, mu, ld_y, IN_BIG), _g(dev, eps, IN_BIG), _g(dev, np.zeros(A, dtype=F32), IN_BIG)
    act_ref, logp_ref, ent_ref = pc.head_exact_reference(mu, eps)

    def run(with_eps, with_logp, with_ent):
        act, logp, ent = Guarded(dev, (B, ld_act), POISON), Guarded(dev, (B,), POISON), Guarded(dev, (B,), POISON)
        L.check(L.lib.pqlk_ppo_gauss_head(yd.ptr, ld_y, lsd.ptr, ed.ptr if with_eps else None, B, A, act.ptr, ld_act,
                                          logp.ptr if with_logp else None, ent.ptr if with_ent else None, L.stream(dev)))
        assert _all(act.t[:, A:], POISON) and act.intact() and logp.intact() and ent.intact()
        if not with_logp:
            assert _all(logp.t, POISON)
        if not with_ent:
            assert _all(ent.t, POISON)
        return _np(act.t[:, :A]), _np(logp.t), _np(ent.t)

    act, logp, ent = run(True, True, True)
    assert np.array_equal(act, act_ref) and np.array_equal(logp, logp_ref) and np.array_equal(ent, np.full(B, ent_ref))
    act, logp, ent = run(False, True, True)
    assert np.array_equal(act, mu) and np.array_equal(logp, pc.row_logp(np.zeros_like(mu))) and np.array_equal(ent, np.full(B, ent_ref))
    act, logp, ent = run(True, False, True)
    assert np.array_equal(act, act_ref) and np.array_equal(ent, np.full(B, ent_ref))
    act, logp, ent = run(True, True, False)
    assert np.array_equal(act, act_ref) and np.array_equal(logp, logp_ref)


@pytest.mark.parametrize("B", pc.HEAD_B)
@pytest.mark.parametrize("A", pc.HEAD_A)
def test_gauss_head_dense(dev, A, B):
    """logstd U(-1, 0.3) against float64 at the bars of test_gaussian_head_and_module_methods (act rtol 2e-5 atol 2e-6, logp and
    ent rtol 2e-5 atol 2e-5)."""
    from pql_amd import _lib as L
    c = pc.head_inputs(A, B)
    mu, eps, ls = c["mu"], c["eps"], c["logstd"]
    ld_y, ld_act = A + 3, A + 2
    yd, ed, lsd = _padded(dev, mu, ld_y, IN_BIG), _g(dev, eps, IN_BIG), _g(dev, ls, IN_BIG)
    act, logp, ent = Guarded(dev, (B, ld_act), POISON), Guarded(dev, (B,), POISON), Guarded(dev, (B,), POISON)
    L.check(L.lib.pqlk_ppo_gauss_head(yd.ptr, ld_y, lsd.ptr, ed.ptr, B, A, act.ptr, ld_act, logp.ptr, ent.ptr, L.stream(dev)))
    a = _np(act.t[:, :A])
    want_act = mu.astype(np.float64) + eps.astype(np.float64) * np.exp(ls.astype(np.float64))
    lp_ref, ent_ref = pc.head_dense_reference(mu, ls, a)
    _err(f"gauss head A={A} B={B} act", a, want_act); _err("  logp", _np(logp.t), lp_ref); _err("  ent", _np(ent.t), [ent_ref])
    np.testing.assert_allclose(a, want_act, rtol=2e-5, atol=2e-6)
    np.testing.assert_allclose(_np(logp.t), lp_ref, rtol=2e-5, atol=2e-5)
    np.testing.assert_allclose(_np(ent.t), np.full(B, ent_ref), rtol=2e-5, atol=2e-5)
    assert _all(act.t[:, A:], POISON) and act.intact() and logp.intact() and ent.intact()


# =========================================================================== gather
@pytest.mark.parametrize("O,A", pc.GATHER_OA)
@pytest.mark.parametrize("mb", pc.GATHER_MB)
def test_gather_exact(dev, mb, O, A):
    """x, the actions and the four scalars bit-equal to indexing with duplicate, negative and too-large indices (clamped into
    the trajectory); pad columns of x written as zero; all three columns of every advantage partial by equality, the partials
    past pqlk_ppo_gather_parts(mb) untouched; mean = var = NULL gives a raw copy."""
    from pql_amd import _lib as L
    c = pc.gather_inputs(mb, O, A)
    tr, k, rows = c["traj"], c["k"], c["rows"]
    ldx = O + 3
    parts = int(L.lib.pqlk_ppo_gather_parts(mb))
    idx = _g(dev, c["idx"], 0, dtype=torch.int64)
    ins = {n: _g(dev, tr[n], IN_BIG) for n in tr}
    md, vd = _g(dev, c["mean"], IN_BIG), _g(dev, c["var"], IN_BIG)
    want_part = pc.adv_partials(c["want_adv"])
    for normalise in (True, False):
        x, act = Guarded(dev, (mb, ldx), POISON), Guarded(dev, (mb, A), POISON)
        outs = [Guarded(dev, (mb,), POISON) for _ in range(4)]
        part = Guarded(dev, (parts + 2, 3), POISON)
        L.check(L.lib.pqlk_ppo_gather(idx.ptr, mb, rows, ins["obs"].ptr, O, md.ptr if normalise else None, vd.ptr if normalise else None,
                                      float(c["eps"]), x.ptr, ldx, ins["act"].ptr, A, act.ptr, ins["logp"].ptr, ins["adv"].ptr,
                                      ins["ret"].ptr, ins["val"].ptr, *[o.ptr for o in outs], part.ptr, L.stream(dev)))
        want_x = pc.normalize_reference(tr["obs"][k], c["mean"], c["var"], c["eps"]) if normalise else tr["obs"][k]
        assert np.array_equal(_np(x.t[:, :O]), want_x), "x"
        assert torch.count_nonzero(x.t[:, O:]) == 0, "pad columns written as zero"
        assert np.array_equal(_np(act.t), tr["act"][k]), "act"
        for got, name in zip(outs, ("logp", "adv", "ret", "val")):
            assert np.array_equal(_np(got.t), tr[name][k]), name
        assert np.array_equal(_np(part.t[:parts]), want_part), "advantage partials { rows, sum, squared deviations }"
        assert _all(part.t[parts:], POISON), "partials past the block count"
        for b in (x, act, part, *outs):
            assert b.intact()


# =========================================================================== policy head
def _policy(dev, A, b, yd, ld_y, lsd, actd, oldd, advd, partd, n_parts, clip, lam, with_logp=True, with_ring=True):
    from pql_amd import _lib as L
    dy, dls, logp = Guarded(dev, (b, ld_y), POISON), Guarded(dev, (A,), POISON), Guarded(dev, (b,), POISON)
    nsc = int(L.lib.pqlk_ppo_scratch_floats(b, A))
    scr, ring = Guarded(dev, (nsc,), POISON), Guarded(dev, (3,), POISON)
    slot = torch.tensor([7], dtype=torch.int32, device=dev)          # 7 % 3 = slot 1
    L.check(L.lib.pqlk_ppo_policy_loss(yd.ptr, ld_y, lsd.ptr, actd.ptr, oldd.ptr, advd.ptr, partd.ptr, n_parts, b, A, float(clip), float(lam),
                                       dy.ptr, dls.ptr, logp.ptr if with_logp else None, scr.ptr, nsc, ring.ptr if with_ring else None,
                                       L.ptr(slot), 3, L.stream(dev)))
    assert _all(dy.t[:, A:], POISON), "pad columns of dy untouched"
    for buf in (dy, dls, logp, scr, ring):
        assert buf.intact()
    if with_ring:
        assert ring.t[0].item() == POISON and ring.t[2].item() == POISON
    else:
        assert _all(ring.t, POISON)
    if not with_logp:
        assert _all(logp.t, POISON)
    return ring.t[1].item(), _np(dy.t[:, :A]), _np(dls.t), _np(logp.t), _np(scr.t)


def _policy_exact_buffers(dev, A, b):
    c = pc.policy_exact_inputs(A, b)
    ld_y = A + 3
    return c, ld_y, dict(yd=_padded(dev, c["mu"], ld_y, IN_BIG), ld_y=ld_y, lsd=_g(dev, c["logstd"], IN_BIG), actd=_g(dev, c["act"], IN_BIG),
                         advd=_g(dev, c["adv"], IN_ONE), partd=_g(dev, c["part"], IN_ONE), n_parts=c["part"].shape[0])


@pytest.mark.parametrize("clip,lam", [(0.2, 0.01), (0.0, 0.0)])
@pytest.mark.parametrize("A,b", [c for c in pc.POLICY_CASES if c[1] > 1])
def test_policy_head_exact(dev, A, b, clip, lam):
    """Every row on the max tie with ratio exactly 1 (clip = 0: on both clamp bounds as well): logp_out, dy = -adv g d (zero on
    the markers), dlogstd = (signed marker count) g - lambda_ent and the loss 0 / b - lambda_ent h, all by equality; the
    per-block partials sum to the exact totals; a run without logp_out and loss_ring changes nothing else."""
    c, ld_y, buf = _policy_exact_buffers(dev, A, b)
    r = pc.policy_exact_reference(A, b, lam)
    zero = _g(dev, np.zeros(b, dtype=F32), IN_ONE)
    _, _, _, logp0, _ = _policy(dev, A, b, oldd=zero, clip=clip, lam=lam, **buf)
    assert np.array_equal(logp0, r["logp"]), "logp_out: index-order fp32 row sum"
    old = _g(dev, logp0, IN_ONE)
    loss, dy, dls, logp, scr = _policy(dev, A, b, oldd=old, clip=clip, lam=lam, **buf)
    assert np.array_equal(logp, r["logp"])
    assert np.array_equal(dy, r["dy"]), "dy"
    assert np.array_equal(dls, r["dlogstd"]), "dlogstd"
    assert loss == float(r["loss"]), "loss"
    scr = scr.reshape(-1, 1 + A).astype(np.float64)
    assert scr[:, 0].sum() == 0 and np.array_equal(scr[:, 1:].sum(0), r["ls_terms"].astype(np.float64).sum(0)), "per-block partials"
    _, dy2, dls2, _, _ = _policy(dev, A, b, oldd=old, clip=clip, lam=lam, with_logp=False, with_ring=False, **buf)
    assert np.array_equal(dy2, dy) and np.array_equal(dls2, dls)


@pytest.mark.parametrize("A", pc.HEAD_A)
def test_policy_head_one_row_is_nan_as_torch(dev, A):
    """b = 1: the unbiased std of one advantage is NaN, and so are the loss and both gradients (include/pqlk.h); logp_out is
    still the row's log-prob, and nothing past the row is written."""
    c, ld_y, buf = _policy_exact_buffers(dev, A, 1)
    zero = _g(dev, np.zeros(1, dtype=F32), IN_ONE)
    loss, dy, dls, logp, _ = _policy(dev, A, 1, oldd=zero, clip=0.2, lam=0.01, **buf)
    assert np.array_equal(logp, pc.row_logp(c["d"]))
    assert np.isnan(loss) and np.isnan(dy).all() and np.isnan(dls).all()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")          # torch warns about the degrees of freedom
        assert np.isnan(T(c["adv"]).std().item())


@pytest.mark.parametrize("clip,lam", [(0.2, 0.01), (0.0, 0.0)])
@pytest.mark.parametrize("A,b", pc.POLICY_CROSS)
def test_policy_head_dense(dev, A, b, clip, lam):
    """Random data past the grid cap, the partials from pqlk_ppo_gather, against float64 autograd at the bars of
    test_policy_head_matches_autograd: loss rtol 2e-5 atol 1e-7; dy and dlogstd rtol 2e-5, atol 2e-5 of the reference's largest
    magnitude."""
    from pql_amd import _lib as L
    c = pc.policy_dense_inputs(A, b)
    ld_y = A + 3
    parts = int(L.lib.pqlk_ppo_gather_parts(b))
    obs, idx = _g(dev, np.zeros((b, 1), dtype=F32), IN_BIG), _g(dev, np.arange(b), 0, dtype=torch.int64)
    traj = {n: _g(dev, c[n] if n in c else np.zeros(b, dtype=F32), IN_BIG) for n in ("act", "logp", "adv", "ret", "val")}
    x, actd, advd = Guarded(dev, (b, 4), POISON), Guarded(dev, (b, A), POISON), Guarded(dev, (b,), POISON)
    junk = [Guarded(dev, (b,), POISON) for _ in range(3)]
    partd = Guarded(dev, (parts, 3), POISON)
    L.check(L.lib.pqlk_ppo_gather(idx.ptr, b, b, obs.ptr, 1, None, None, 0.0, x.ptr, 4, traj["act"].ptr, A, actd.ptr, traj["logp"].ptr,
                                  traj["adv"].ptr, traj["ret"].ptr, traj["val"].ptr, junk[0].ptr, advd.ptr, junk[1].ptr, junk[2].ptr,
                                  partd.ptr, L.stream(dev)))
    assert np.array_equal(_np(advd.t), c["adv"]) and np.array_equal(_np(actd.t), c["act"]) and partd.intact()
    buf = dict(yd=_padded(dev, c["y"], ld_y, IN_BIG), ld_y=ld_y, lsd=_g(dev, c["logstd"], IN_BIG), actd=actd, advd=advd, partd=partd,
               n_parts=parts)
    zero = _g(dev, np.zeros(b, dtype=F32), IN_BIG)
    _, _, _, logp0, _ = _policy(dev, A, b, oldd=zero, clip=clip, lam=lam, **buf)
    old = (logp0 - c["shift"]).astype(F32)
    loss, dy, dls, logp, _ = _policy(dev, A, b, oldd=_g(dev, old, IN_BIG), clip=clip, lam=lam, **buf)
    assert np.array_equal(logp, logp0)
    l_r, dmu_r, dls_r, ratio = pc.policy_dense_reference(c["y"], c["logstd"], c["act"], old, c["adv"], clip, lam, logp)
    assert bool((ratio == 1).any()) and bool((ratio > 1 + clip).any()) and bool((ratio < 1 - clip).any())
    print(f"policy head A={A} b={b} clip={clip}: loss {loss:.8g} ref {l_r:.8g} rel err {abs(loss - l_r) / abs(l_r):.3e}")
    _err("  dy", dy, dmu_r); _err("  dlogstd", dls, dls_r)
    np.testing.assert_allclose(loss, l_r, rtol=2e-5, atol=1e-7)
    np.testing.assert_allclose(dy, dmu_r, rtol=2e-5, atol=2e-5 * np.abs(dmu_r).max())
    np.testing.assert_allclose(dls, dls_r, rtol=2e-5, atol=2e-5 * np.abs(dls_r).max())


# =========================================================================== value head
def _value(dev, v, R, V, b, clip_on, clip, ld_v, ld_dy, with_ring=True):
    from pql_amd import _lib as L
    vd = _padded(dev, v[:, None], ld_v, IN_BIG)
    Rd, Vd = _g(dev, R, IN_BIG), _g(dev, V, IN_BIG)
    dy = Guarded(dev, (b, ld_dy), POISON)
    nsc = int(L.lib.pqlk_ppo_scratch_floats(b, 1)) // 2          # (1 + A) floats per block at A = 1; the value head needs one
    scr, ring = Guarded(dev, (nsc,), POISON), Guarded(dev, (3,), POISON)
    slot = torch.tensor([5], dtype=torch.int32, device=dev)      # 5 % 3 = slot 2
    L.check(L.lib.pqlk_ppo_value_loss(vd.ptr, ld_v, Rd.ptr, Vd.ptr if clip_on else None, b, int(clip_on), float(clip), dy.ptr, ld_dy, scr.ptr,
                                      nsc, ring.ptr if with_ring else None, L.ptr(slot), 3, L.stream(dev)))
    assert _all(dy.t[:, 1:], POISON), "the other columns of dy"
    assert dy.intact() and scr.intact() and ring.intact()
    assert _all(ring.t[:2], POISON) and (with_ring or _all(ring.t, POISON))
    return ring.t[2].item(), _np(dy.t[:, 0]), _np(scr.t)


@pytest.mark.parametrize("clip_on", [1, 0])
@pytest.mark.parametrize("b", pc.VALUE_B)
def test_value_head_exact(dev, b, clip_on):
    """Quarter-integer v, R, V and clip = 0.25: rows exactly on both clamp bounds, inside and outside, lu == lc ties; the loss, dy
    column 0 and the per-block partials by equality with ld_dy != ld_v, in a second, ragged trip of the capped grid; loss_ring =
    NULL leaves the ring alone and dy as it was."""
    v, R, V = pc.value_exact_inputs(b)
    terms, S, loss, dy_ref = pc.value_reference(v, R, V, b, clip_on)
    for ld_v, ld_dy in ((3, 5), (4, 4)):
        got, dy, scr = _value(dev, v, R, V, b, clip_on, pc.VALUE_CLIP, ld_v, ld_dy)
        assert got == float(loss), "loss"
        assert np.array_equal(dy, dy_ref), "dy column 0"
        assert scr.astype(np.float64).sum() == S, "per-block partials"
    _, dy, scr = _value(dev, v, R, V, b, clip_on, pc.VALUE_CLIP, 3, 5, with_ring=False)
    assert np.array_equal(dy, dy_ref) and scr.astype(np.float64).sum() == S


@pytest.mark.parametrize("clip_on", [1, 0])
def test_value_head_dense(dev, clip_on):
    """Random data past the grid cap against float64 autograd at the bars of test_value_head_matches_autograd: loss rtol 2e-5,
    dy rtol 2e-5 atol 1e-12."""
    b = pc.VALUE_B[-1]
    v, R, V = pc.value_dense_inputs(b)
    loss_r, grad_r = pc.value_autograd(v, R, V, clip_on, pc.VALUE_DENSE_CLIP)
    loss, dy, _ = _value(dev, v, R, V, b, clip_on, pc.VALUE_DENSE_CLIP, 3, 5)
    nz = grad_r != 0
    print(f"value head b={b} clip_on={clip_on}: loss rel err {abs(loss - loss_r) / loss_r:.3e}, "
          f"dy max rel err {np.abs(dy[nz] / grad_r[nz] - 1).max():.3e}, max abs err where the reference is 0 {np.abs(dy[~nz]).max():.3e}")
    np.testing.assert_allclose(loss, loss_r, rtol=2e-5)
    np.testing.assert_allclose(dy, grad_r, rtol=2e-5, atol=1e-12)


# =========================================================================== rollout elementwise kernels
def test_rms_normalize_past_the_grid_cap(dev):
    """4096 x 256 elements and a ragged second trip, 13 columns into rows of stride 16: bit-equal to the CPU expression (the sqrt
    through numpy, see test_rms_merge_normalize_and_action_noise_kernels_match_the_cpu_expressions); pad columns untouched."""
    from pql_amd import _lib as L
    c = pc.elementwise_inputs()
    rows, cols, ld = pc.ELEMENTWISE_ROWS, pc.ELEMENTWISE_COLS, pc.ELEMENTWISE_LD_OUT
    xd, md, vd = _g(dev, c["x"], IN_BIG), _g(dev, c["mean"], IN_BIG), _g(dev, c["var"], IN_BIG)
    out = Guarded(dev, (rows, ld), POISON)
    L.check(L.lib.pqlk_rms_normalize(xd.ptr, rows, cols, md.ptr, vd.ptr, 1e-4, out.ptr, ld, L.stream(dev)))
    assert np.array_equal(_np(out.t[:, :cols]), pc.normalize_reference(c["x"], c["mean"], c["var"], 1e-4))
    assert _all(out.t[:, cols:], POISON) and out.intact()


@pytest.mark.parametrize("per_row", [True, False])
def test_action_noise_past_the_grid_cap(dev, per_row):
    """The same element count with one sigma per row and with the scalar sigma: clamp(act + draw * sigma, -1, 1) to the bit."""
    from pql_amd import _lib as L
    c = pc.elementwise_inputs()
    rows, cols = pc.ELEMENTWISE_ROWS, pc.ELEMENTWISE_COLS
    ad, dd_, sd = _g(dev, c["act"], IN_BIG), _g(dev, c["draw"], IN_BIG), _g(dev, c["std_rows"], IN_BIG)
    out = Guarded(dev, (rows, cols), POISON)
    L.check(L.lib.pqlk_action_noise(ad.ptr, dd_.ptr, sd.ptr if per_row else None, 0.3, rows, cols, -1.0, 1.0, out.ptr, L.stream(dev)))
    sigma = c["std_rows"][:, None] if per_row else F32(0.3)
    want = pc.noise_reference(c["act"], c["draw"], sigma, -1.0, 1.0)
    assert np.array_equal(_np(out.t), want) and out.intact()
    assert 0 < int((want == 1).sum()) and 0 < int((want == -1).sum()) and int((np.abs(want) < 1).sum()) > rows
