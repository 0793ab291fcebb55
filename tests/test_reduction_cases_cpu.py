"""The inputs of tests/test_reductions_gpu.py mean what the GPU tests assume: the shapes cross the kernels' grid caps, the
exact-sum designs are exact in any order, the saturated rows saturate, and no case is skipped.  No GPU needed."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import reduction_cases as rc

F32 = np.float32


@pytest.fixture(scope="module")
def ref():
    from oracle import pql_ref_cpu
    return pql_ref_cpu


# --------------------------------------------------------------------------- shapes cross the caps
def test_loss_shapes_cross_the_block_cap():
    """Through the host entry point: if LOSS_MAX_BLOCKS or a rows-per-block figure moves, this names the shape to move."""
    from pql_amd import _lib as L
    B = rc.TD_B[-1]
    assert L.lib.pqlk_loss_parts(B, 1) == rc.LOSS_MAX_BLOCKS and B > rc.LOSS_MAX_BLOCKS * rc.TD_ROWS_PER_BLOCK, "TD_B[-1]"
    assert B - rc.LOSS_MAX_BLOCKS * rc.TD_ROWS_PER_BLOCK not in (0, 256), "TD_B[-1]: second trip must end ragged"
    for K in (51, 64):
        B = rc.C51_B_BIG
        assert L.lib.pqlk_loss_parts(B, K) == rc.LOSS_MAX_BLOCKS and B > 2 * rc.LOSS_MAX_BLOCKS * rc.C51_ROWS_PER_BLOCK, "C51_B_BIG"
    assert rc.C51_B[-1] == rc.C51_B_BIG and B % 4 != 0
    for B in rc.TD_B[:-1]:                     # below the cap the partial count follows the batch
        assert L.lib.pqlk_loss_parts(B, 1) == (B + 255) // 256
    for B in rc.C51_B[:-1] + [37]:
        assert L.lib.pqlk_loss_parts(B, 51) == (B + 3) // 4
    assert rc.PROJECT_B > rc.PROJECT_MAX_BLOCKS * rc.PROJECT_ROWS_PER_BLOCK and rc.PROJECT_B % 4 != 0, "PROJECT_B"


def test_optimiser_shapes_cross_the_trip_sizes():
    n = rc.ADAM_N_EXACT
    assert 2 * rc.SUMSQ_TRIP < n < 3 * rc.SUMSQ_TRIP, "ADAM_N_EXACT: third, ragged trip of k_sumsq"
    assert rc.ADAMW_VEC_TRIP < n < 2 * rc.ADAMW_VEC_TRIP, "ADAM_N_EXACT: second, ragged trip of k_adamw's 16-byte path"
    assert n % 4 == 3 and (n // 4) % 256 != 0, "ADAM_N_EXACT: 3-element tail, ragged last block"
    assert rc.ADAM_N_DENSE % 4 == 3
    assert rc.ADAMW_SCALAR_TRIP < rc.ADAM_N_MISALIGNED < 2 * rc.ADAMW_SCALAR_TRIP and rc.ADAM_N_MISALIGNED % 256 != 0, "ADAM_N_MISALIGNED"
    assert rc.POLYAK_TRIP < rc.POLYAK_N[-1] < 2 * rc.POLYAK_TRIP and rc.POLYAK_N[-1] % 256 != 0, "POLYAK_N[-1]"


def test_pack_layout_is_fused_capable_and_takes_a_second_scalar_trip():
    from pql_amd import _lib as L
    d = L.mlp_desc(rc.PACK_DIMS, rc.PACK_NETS)
    n = int(L.lib.pqlk_mlp_param_floats(C.byref(d)))
    assert int(L.lib.pqlk_mlp_packed_floats(C.byref(d))) > 0, "PACK_DIMS: no fragment-ordered copy for this layout"
    blocks = min(2048, ((n + 3) // 4 + 255) // 256)      # k_adamw's grid; misaligned, every element goes through the scalar loop
    assert n > blocks * 256, "PACK_DIMS: the scalar loop would finish in one trip"


def test_moments_and_bn_shapes_hit_the_chunk_edges():
    chunks = lambda n: min(64, (n + 63) // 64)  # noqa: E731
    assert sorted({chunks(n) for n in rc.MOMENTS_N}) == [1, 2, 3, 64]
    last = lambda n: n - (chunks(n) - 1) * -(-n // chunks(n))  # noqa: E731  rows of the last chunk
    assert last(4033) == 1 and last(4097) == 2 and last(129) == 43
    assert any(c % 32 for c in rc.MOMENTS_COLS) and any(c > 32 for c in rc.MOMENTS_COLS)
    assert any(m < 64 for m in rc.BN_M) and any(m > 64 and m % 64 for m in rc.BN_M)      # empty chunks; ragged chunks
    assert any(c > 64 and c % 64 for c in rc.BN_COLS)


# --------------------------------------------------------------------------- exact sums are exact
def _assert_exact(x, unit, what):
    x = np.asarray(x, dtype=F32).reshape(-1)
    assert np.all(x / F32(unit) == np.round(x / F32(unit))), what
    sums, s64 = rc.sums_three_orders(x)
    assert float(np.abs(x.astype(np.float64)).sum()) / unit < 2 ** 24, what     # every partial sum stays exactly representable
    assert all(s == s64 for s in sums), (what, sums, s64)


@pytest.mark.parametrize("B", rc.TD_B)
def test_td_terms_sum_exactly(B):
    q, qt, rew, done, gn = rc.td_inputs(B)
    terms, S, loss, dy = rc.td_reference(q, qt, rew, done, gn, B)
    assert terms.max() <= 6.25 and set(np.unique(done)) <= {0.0, 1.0} and set(np.unique(q)) <= {-1.0, 0.0, 1.0}
    _assert_exact(terms, 0.25, f"td B={B}")
    assert S <= 12.5 * B < 2 ** 22
    if B > 1000:
        assert terms.min() == 0 and terms.max() == 6.25 and len(np.unique(dy)) > 5      # the design is not degenerate


@pytest.mark.parametrize("B", rc.TD_B)
def test_dpg_scalar_mins_sum_exactly(B):
    q = rc.dpg_scalar_inputs(B)
    mins, S, loss, dy, owner = rc.dpg_scalar_reference(q, B)
    _assert_exact(mins, 1.0, f"dpg B={B}")
    if B > 255:
        ties = float((q[0] == q[1]).mean())
        assert 0.1 < ties < 0.25 and set(np.unique(owner)) == {1, 2, 3}
        assert set(np.unique(dy)) == {float(F32(-1) / F32(B)), float(F32(0.5) * (F32(-1) / F32(B))), 0.0}


def test_adam_exact_gradient_has_norm_four_in_any_order():
    g = rc.adam_exact_grad()
    _assert_exact(g * g, 1.0, "adam exact")
    assert float((g.astype(np.float64) ** 2).sum()) == 16.0
    pos = np.array(rc.adam_exact_positions())
    trip = pos // rc.SUMSQ_TRIP
    assert [int((trip == t).sum()) >= 4 for t in range(3)] == [True] * 3           # every trip of k_sumsq sees some
    assert int((pos >= (rc.ADAM_N_EXACT // 4) * 4).sum()) == 3                       # the tail


@pytest.mark.parametrize("b", rc.ALPHA_B)
def test_alpha_logp_sums_exactly(b):
    _assert_exact(rc.ints((b,), 851 + b, -8, 8), 1.0, f"alpha b={b}")


def test_bn_integer_dy_sums_exactly():
    dy = rc.ints((257, 65), 861, -4, 4)
    for c in (0, 31, 64):
        _assert_exact(dy[:, c], 1.0, f"bn dbeta col {c}")
    z, zz, gamma, beta, mean, var, rm0, rv0 = rc.bn_inputs(257, 65, 68, beta_shift=20.0)
    assert rc.bn_reference(zz, gamma, beta).min() > 1.0        # every y > 0: ELU' == 1 and dbeta is the plain integer sum


# --------------------------------------------------------------------------- inputs reach the branches
@pytest.mark.parametrize("K", [51, 64])
def test_saturated_rows_are_classified_as_intended(ref, K):
    B = 37
    lg, lt, rew, done, gn = rc.c51_inputs(B, K, saturated=True)
    p = torch.softmax(lg, 2)                                   # torch fp32 on the CPU
    for i, gap in enumerate(rc.SAT_GAPS):
        for net in range(2):
            top = (7 * i + 3 * net) % K
            others = torch.cat([p[net, i, :top], p[net, i, top + 1:]])
            if gap == 60:
                assert p[net, i, top].item() == 1.0 and bool(((others > 0) & (others < 1e-12)).all())
                np.testing.assert_allclose(others.numpy(), 8.76e-27, rtol=1e-2)
            elif gap == 120:
                assert p[net, i, top].item() == 1.0 and bool((others == 0).all())
            else:
                assert 0.9 < p[net, i, top].item() < 1.0 and bool((others > 1e-6).all())
    tgt, loss, grad = rc.c51_reference(ref, lg, lt, rew, done, gn, K)
    assert bool(torch.isfinite(loss)) and bool(torch.isfinite(grad).all())
    hard = [i for i, gap in enumerate(rc.SAT_GAPS) if gap >= 60]
    assert float(grad[:, hard].abs().max()) < 1e-16
    # what a kernel without the 1e-12 clamp would return on those rows, t / (B K), is far above the dy bar (atol 2e-9)
    assert float(tgt[hard].max(1).values.min()) / (B * K) > 1e-6


@pytest.mark.parametrize("K,v_min,v_max", [(51, -10.0, 10.0), (33, -2.0, 6.0), (2, -10.0, 10.0)])
def test_c51_rewards_clamp_at_both_ends(K, v_min, v_max):
    lg, lt, rew, done, gn = rc.c51_inputs(37, K, v_min, v_max)
    tz = rew + (1 - done) * gn * torch.linspace(v_min, v_max, K)
    assert bool((tz < v_min).any()) and bool((tz > v_max).any()) and bool(((tz > v_min) & (tz < v_max)).any())
    assert 0 < done.sum() < 37


def test_projection_rows_are_terminal_and_on_the_grid():
    p, rew, done, gn, grid = rc.project_inputs()
    B, K = p.shape
    assert done.sum().item() >= B // 4 and int(grid.sum()) >= B // 4
    b = (rew.clamp(-10, 10) - (-10.0)) / ((10.0 - -10.0) / (K - 1))      # the oracle's position of a terminal row
    g = torch.from_numpy(grid)
    assert bool((b[g].floor() == b[g].ceil()).all()), "lo == up before the fix-up on every grid row"
    on = torch.unique(b[g])
    assert len(on) >= K // 4 and on[0] == 0 and on[-1] == K - 1           # many atoms, both ends included
    free = ~g & (done.view(-1) == 0)
    assert bool((rew.view(-1)[free] > 10.5).any()) and bool((rew.view(-1)[free] < -10.5).any())


def test_sg_inputs_saturate_tanh_and_leave_the_clamp():
    for A in rc.SG_A:
        y, mu, ls, eps = rc.sg_inputs(257, A, 2 * A + 3)
        a, logp, u = rc.sg_reference(mu, ls, eps)
        assert np.abs(u).max() > 12 and np.isfinite(logp).all()
        assert (ls > 5).any() and (ls < -5).any()
        assert np.all(np.sign(eps) == np.sign(mu)) and np.abs(a).min() > 0


def test_bn_inputs_have_no_tiny_variance():
    for m in rc.BN_M:
        for cols in rc.BN_COLS:
            z, zz, gamma, beta, mean, var, rm0, rv0 = rc.bn_inputs(m, cols, cols + 3)
            vb = var.astype(np.float64) * (m - 1) / m
            if m > 2:
                assert vb.min() > 0.3, (m, cols)
            else:       # two rows: 1 - xhat^2 = eps / (var + eps) must not vanish, and z * w must stay O(1)
                assert (1e-5 / (vb + 1e-5)).min() > 0.05 and (np.abs(zz) * gamma / np.sqrt(vb + 1e-5)).max() < 10, cols


# --------------------------------------------------------------------------- every case is asserted
def test_gpu_module_skips_nothing():
    src = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "test_reductions_gpu.py")).read()
    for word in ("skip", "xfail", "importorskip"):
        assert word not in src, word
