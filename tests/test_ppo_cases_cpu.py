"""The inputs of tests/test_ppo_kernels_gpu.py mean what the GPU tests assume: the shapes cross the kernels' caps and end ragged,
the exact designs are exact in any order, the advantage design has mean 0 and std 1 under an fp32 model of the kernels, the
ties, bounds and markers are there, and no case is empty or skipped.  No GPU needed."""
import os

import numpy as np
import pytest
import torch

import ppo_cases as pc

F32, F64 = np.float32, np.float64
ALL_B = sorted({b for _, b in pc.POLICY_CASES if b > 1})


# --------------------------------------------------------------------------- shapes cross the caps
@pytest.mark.parametrize("A,b", pc.POLICY_CROSS)
def test_policy_shapes_cross_the_block_cap_and_end_ragged(A, b):
    """Through the host entry point: if PPO_HEAD_BLOCKS or the rows per block move, this names the shape to move."""
    from pql_amd import _lib as L
    what = f"POLICY_CROSS_B[{A}] = {b}"
    g, rpg = pc.groups_per_block(A), pc.rows_per_grid(A)
    assert L.lib.pqlk_ppo_scratch_floats(b, A) == pc.PPO_HEAD_BLOCKS * (1 + A), what
    assert L.lib.pqlk_ppo_scratch_floats(rpg, A) // (1 + A) == pc.PPO_HEAD_BLOCKS == L.lib.pqlk_ppo_scratch_floats(rpg - g, A) // (1 + A) + 1, what
    last = b - ((b - 1) // rpg) * rpg                      # rows of the last trip
    assert b > rpg and b % 2 == 1, what
    assert g < last < rpg and last % g != 0, what + ": the last trip must be partly empty and end in a partial block"
    assert b % pc.PPO_GATHER_ROWS != 0, what + ": the last gather block must be ragged"
    if A == 21:
        assert b > 2 * rpg, what + ": a third trip"


def test_policy_shapes_below_the_cap_follow_the_batch():
    from pql_amd import _lib as L
    for A in pc.HEAD_A:
        g, small = pc.groups_per_block(A), pc.POLICY_SMALL_B[A]
        assert 1 < small < g and small % 2 == 1, f"POLICY_SMALL_B[{A}]"
        for b in (1, small, g, g + 1, 5 * g + 1):
            assert L.lib.pqlk_ppo_scratch_floats(b, A) == -(-b // g) * (1 + A), (A, b)
    assert sorted({pc.group_of(A) for A in pc.HEAD_A}) == [1, 4, 32, 64] and pc.group_of(33) == pc.group_of(64) == 64
    assert (16, 8229) in pc.POLICY_CASES and len(pc.POLICY_CASES) == 16 and len(set(pc.POLICY_CASES)) == 16


def test_value_gather_gae_and_elementwise_shapes_hit_their_edges():
    from pql_amd import _lib as L
    b = pc.VALUE_B[-1]
    assert L.lib.pqlk_ppo_scratch_floats(b, 1) == 2 * pc.PPO_HEAD_BLOCKS, "VALUE_B[-1]"     # A = 1: (1 + A) floats per block
    assert pc.PPO_HEAD_BLOCKS * 256 < b < 2 * pc.PPO_HEAD_BLOCKS * 256 and (b - pc.PPO_HEAD_BLOCKS * 256) % 256 != 0, "VALUE_B[-1]"
    assert [(-(-x // 256)) for x in pc.VALUE_B[:-1]] == [1, 1, 2]
    parts = [int(L.lib.pqlk_ppo_gather_parts(mb)) for mb in pc.GATHER_MB]
    assert parts == [-(-mb // pc.PPO_GATHER_ROWS) for mb in pc.GATHER_MB] == [1, 1, 1, 2, 65], "GATHER_MB"
    assert parts[-1] > 64 and pc.GATHER_MB[-1] % pc.PPO_GATHER_ROWS not in (0, 1), "GATHER_MB[-1]: > 64 partials and a ragged tail"
    assert pc.GATHER_MB[:4] == [1, pc.PPO_GATHER_ROWS - 1, pc.PPO_GATHER_ROWS, pc.PPO_GATHER_ROWS + 1]
    for lim in pc.GAE_UNROLL:
        assert lim in pc.GAE_T and lim + 1 in pc.GAE_T, f"GAE_T around {lim}"
    assert 1 in pc.GAE_T and 1 in pc.GAE_N and 255 in pc.GAE_N and 257 in pc.GAE_N
    cap = pc.ELEMENTWISE_MAX_BLOCKS * pc.ELEMENTWISE_THREADS
    total = pc.ELEMENTWISE_ROWS * pc.ELEMENTWISE_COLS
    assert cap + 257 <= total < cap + 257 + pc.ELEMENTWISE_COLS and (total - cap) % 256 != 0, "ELEMENTWISE_ROWS"
    assert pc.ELEMENTWISE_LD_OUT > pc.ELEMENTWISE_COLS and total < 1.1 * 2 ** 20


# --------------------------------------------------------------------------- exact sums are exact
def _assert_exact(x, unit, what):
    x = np.asarray(x, dtype=F32).reshape(-1)
    assert np.all(x / F32(unit) == np.round(x / F32(unit))), what
    sums, s64 = pc.sums_three_orders(x)
    assert float(np.abs(x.astype(F64)).sum()) / unit < 2 ** 24, what     # every partial sum stays exactly representable
    assert all(s == s64 for s in sums), (what, sums, s64)


@pytest.mark.parametrize("n", ALL_B + [37, 65] + [mb for mb in pc.GATHER_MB if mb > 1])
def test_advantage_design_is_exact_and_normalises_to_itself(n):
    """Every block's two sums in three fp32 orders; then ppo_adv_stats op by op in fp32 over shuffled partials: mean 0, and for
    odd n std 1 with std + 1e-8f == 1, so (adv - mean) / (std + 1e-8f) is adv to the bit."""
    a = pc.adv_design(n)
    assert set(np.unique(a)) <= {-1.0, 0.0, 1.0} and int((a == 1).sum()) == int((a == -1).sum()) == n // 2
    assert int((a == 0).sum()) == n % 2 and (n % 2 == 0 or a[-1] == 0)
    part = pc.adv_partials(a)
    for i in range(part.shape[0]):
        blk = a[i * pc.PPO_GATHER_ROWS:(i + 1) * pc.PPO_GATHER_ROWS]
        _assert_exact(blk, 1.0, f"adv n={n} block {i}")
        m = F32(part[i, 1] / F32(blk.size))
        assert float(m) * 64 == round(float(m) * 64) and float(m) == float(blk.astype(F64).mean()), (n, i)
        dv = (blk - m).astype(F32)
        _assert_exact(dv * dv, 1.0 / 4096, f"adv n={n} block {i} squared deviations")
        assert part[i, 0] == blk.size and part[i, 1] == blk.astype(F64).sum() and part[i, 2] == ((blk.astype(F64) - blk.astype(F64).mean()) ** 2).sum()
    if n % pc.PPO_GATHER_ROWS:
        assert part[-1, 1] == 0, "the ragged block is zero-sum"
    if n > 1000:
        assert len(np.unique(part[:-1, 1])) > 5, "the full blocks' means vary"
    rs = np.random.RandomState(n)
    for order in (None, np.arange(part.shape[0])[::-1], rs.permutation(part.shape[0]), rs.permutation(part.shape[0])):
        m, std, ad = pc.adv_stats_model(part, n, order)
        assert m == 0
        if n % 2:
            assert std == 1 and ad == 1
            assert np.array_equal(((a - m) / ad).astype(F32), a)


@pytest.mark.parametrize("A,b", [c for c in pc.POLICY_CASES if c[1] > 1])
def test_policy_exact_design_has_its_markers_and_exact_sums(A, b):
    c = pc.policy_exact_inputs(A, b)
    rows, cols, signs = c["markers"]
    d, adv = c["d"], c["adv"]
    g, rpg = pc.groups_per_block(A), pc.rows_per_grid(A)
    assert rows[0] == 0 and rows[-1] == b - 1 and len(rows) == len(set(rows)) >= 2
    for k in range(rpg, b, rpg):
        assert k - 1 in rows and k in rows, f"trip boundary {k}"
    if b > rpg:
        start = ((b - 1) // rpg) * rpg
        assert start + ((b - start) // g) * g - 1 in rows and start + ((b - start) // g) * g in rows
    assert int((d == 0).sum()) == len(rows) and bool((d[rows, cols] == 0).all()) and set(np.unique(d)) == {-1.0, 0.0, 1.0}
    assert [float(adv[r]) for r in rows] == [float(s) for s in signs]
    for j in range(A):
        on = [s for s, cj in zip(signs, cols) if cj == j]
        assert on.count(1) <= 2 and on.count(-1) <= 2, f"column {j}: at most two markers of each sign"
    assert sum(1 for s in signs if s) > 0
    for lam in (0.0, 0.01):
        r = pc.policy_exact_reference(A, b, lam)
        assert set(np.unique(r["ls_terms"] / r["g"])) <= {-1.0, 0.0, 1.0} and int((r["ls_terms"] != 0).sum()) == sum(1 for s in signs if s)
        for j in range(A):
            col = r["ls_terms"][:, j]
            sums, s64 = pc.sums_three_orders(col)
            assert all(s == s64 for s in sums), (A, b, j)
            count = sum(s for s, cj in zip(signs, cols) if cj == j)
            assert r["dlogstd"][j] == F32(F32(count) * r["g"]) - F32(lam)
        _assert_exact(r["loss_terms"], 1.0, f"policy loss terms A={A} b={b}")
        assert r["loss_terms"].astype(F64).sum() == 0 and r["loss"] == F32(0) - F32(F32(lam) * pc.entropy_sum(A))
        assert np.array_equal(r["dy"], (-adv[:, None] * r["g"] * d).astype(F32))
        assert set(np.unique(r["dy"] / r["g"])) == {-1.0, 0.0, 1.0}
        assert np.isfinite(r["logp"]).all() and len(np.unique(r["logp"])) == 2      # marker rows and the others
    # the model's ratio, clamp and tie at these inputs: clip 0.2 and clip 0 both keep ratio = 1 inside the closed interval
    for clip in (0.2, 0.0):
        lo, hi = F32(1.0 - float(F32(clip))), F32(1.0 + float(F32(clip)))
        assert lo <= F32(1) <= hi and (clip > 0 or lo == hi == 1)


def test_policy_exact_reference_is_torch_autograd():
    """The op-by-op model against float64 autograd of ppo.py:156-175 on the same exact data (old = the model's own logp)."""
    for A, b in ((3, 37), (21, 4109)):
        c = pc.policy_exact_inputs(A, b)
        r = pc.policy_exact_reference(A, b, 0.01)
        for clip in (0.2, 0.0):
            loss, dmu, dls, ratio = pc.policy_dense_reference(c["mu"], c["logstd"], c["act"], r["logp"], c["adv"], clip, 0.01, r["logp"])
            assert bool((ratio == 1).all())
            np.testing.assert_allclose(r["dy"], dmu, rtol=1e-6, atol=0)
            np.testing.assert_allclose(r["dlogstd"], dls, rtol=1e-6, atol=1e-9)
            np.testing.assert_allclose(float(r["loss"]), loss, rtol=1e-6)


@pytest.mark.parametrize("b", pc.VALUE_B)
def test_value_exact_design_sums_exactly_and_is_torch_autograd(b):
    v, R, V = pc.value_exact_inputs(b)
    clip = pc.VALUE_CLIP
    for x in (v, R, V):
        assert np.all(x * 4 == np.round(x * 4))
    assert np.abs(v - R).max() <= 2 and set(np.unique(v - V)) <= {-0.5, -0.25, 0.0, 0.25, 0.5}
    for clip_on in (1, 0):
        terms, S, loss, dy = pc.value_reference(v, R, V, b, clip_on)
        _assert_exact(terms, 1.0 / 16, f"value b={b} clip_on={clip_on}")
        assert S * 16 < 2 ** 24 and terms.max() <= 2.25 ** 2
        loss64, grad64 = pc.value_autograd(v, R, V, clip_on, clip)
        # float64 is exact on this data: loss64 = 0.5 S / b, grad64 = c / b with c a multiple of 1/8 -- the same ties and bounds
        S64 = round(loss64 * 2 * b * 16) / 16
        assert abs(S64 - loss64 * 2 * b) < 1e-6 and S64 == S
        c = np.round(grad64 * b * 8) / 8
        assert np.abs(c - grad64 * b).max() < 1e-9
        g = F32(F32(0.5) * (F32(1) / F32(b)))
        assert np.array_equal(dy, (F32(2) * c.astype(F32) * g).astype(F32)), "dy is g * (2 c): the tie and closed-interval rules are torch's"
    if b > 200:
        dd_, du = v - V, v - R
        lu = du * du
        lc = (V + np.clip(dd_, -clip, clip) - R) ** 2
        inside = np.abs(dd_) <= clip
        assert int((dd_ == clip).sum()) > 0 and int((dd_ == -clip).sum()) > 0 and int((dd_ == 0).sum()) > 0
        assert int((np.abs(dd_) > clip).sum()) > 0
        assert int((lu == lc).sum()) > 0 and bool((lu[inside] == lc[inside]).all())
        assert int(((lu > lc) & ~inside).sum()) > 0 and int(((lc > lu) & ~inside).sum()) > 0
        assert int((lu == 0).sum()) > 0


def test_value_dense_design_keeps_float64_a_valid_reference():
    b = pc.VALUE_B[-1]
    v, R, V = pc.value_dense_inputs(b)
    du = np.abs(v.astype(F64) - R)
    assert bool(((du >= pc.VALUE_DENSE_MIN_GAP) | (du == 0)).all()) and int((du == 0).sum()) == -(-b // 16)
    dd_ = np.abs(v.astype(F64) - V)
    assert np.abs(dd_ - pc.VALUE_DENSE_CLIP).min() > 0.04, "no row near the clamp bound"
    assert int((dd_ < pc.VALUE_DENSE_CLIP).sum()) > b // 2 and int((dd_ > pc.VALUE_DENSE_CLIP).sum()) > b // 4


def test_dense_policy_shifts_reach_both_clipped_sides_and_one():
    for A, b in pc.POLICY_CROSS:
        s = pc.policy_dense_inputs(A, b)["shift"]
        r = np.exp(s.astype(F64))
        assert int((s == 0).sum()) > 0 and int((r > 1.2).sum()) > 0 and int((r < 0.8).sum()) > 0 and int(((r > 1) & (r < 1.2)).sum()) > 0
        assert np.abs(r - 1.2).min() > 0.1 and np.abs(r - 0.8).min() > 0.1      # no ratio near a bound of clip 0.2


# --------------------------------------------------------------------------- gather, head, GAE
@pytest.mark.parametrize("mb", pc.GATHER_MB)
def test_gather_indices_clamp_repeat_and_gather_the_design(mb):
    O, A = pc.GATHER_OA[1]
    c = pc.gather_inputs(mb, O, A)
    idx, k, rows = c["idx"], c["k"], c["rows"]
    assert idx[0] == -5 and k[0] == 0
    if mb >= 2:
        assert idx[-1] == rows + 3 and k[-1] == rows - 1
    if mb >= 4:
        assert len(np.unique(idx)) == mb - 1, "one duplicate"
    want = c["want_adv"]
    assert np.array_equal(c["traj"]["adv"][k], want) and np.array_equal(want[:-1], pc.adv_design(mb)[:-1])
    assert want[-1] == (-1 if mb % pc.PPO_GATHER_ROWS == 1 else pc.adv_design(mb)[-1])
    part = pc.adv_partials(want)
    for i in range(part.shape[0]):
        blk = want[i * pc.PPO_GATHER_ROWS:(i + 1) * pc.PPO_GATHER_ROWS]
        m = F32(part[i, 1] / F32(blk.size))
        _assert_exact(blk, 1.0, f"gather mb={mb} block {i}")
        _assert_exact(((blk - m) * (blk - m)).astype(F32), 1.0 / 4096, f"gather mb={mb} block {i} squared deviations")
        assert float(m) == float(blk.astype(F64).mean()) and part[i, 2] == ((blk.astype(F64) - blk.astype(F64).mean()) ** 2).sum()
    if mb % pc.PPO_GATHER_ROWS == 1:
        assert part[-1].tolist() == [1.0, -1.0, 0.0], "a one-row block: mean = the row, no deviation"
    assert int((c["traj"]["adv"] == 3.0).sum()) >= 7, "unnamed trajectory rows would move a partial"
    x = pc.normalize_reference(c["traj"]["obs"][k], c["mean"], c["var"], c["eps"])
    assert x.dtype == F32 and np.isfinite(x).all()
    np.testing.assert_allclose(x, (c["traj"]["obs"][k].astype(F64) - c["mean"]) / np.sqrt(c["var"].astype(F64) + 1e-4), rtol=1e-6, atol=1e-6)


def test_head_references_agree_with_float64():
    for A in pc.HEAD_A:
        c = pc.head_inputs(A, 257)
        act, logp, ent = pc.head_exact_reference(c["mu"], c["eps"])
        lp64, ent64 = pc.head_dense_reference(c["mu"], np.zeros(A), act)
        np.testing.assert_allclose(logp, lp64, rtol=2e-6)
        np.testing.assert_allclose(float(ent), ent64, rtol=2e-6)
        assert ent == pc.seq_sum(np.full((1, A), pc.ENT_CONST))[0]


@pytest.mark.parametrize("gae", [True, False])
@pytest.mark.parametrize("with_timeout", [False, True])
def test_gae_reference_is_the_torch_loop_bit_for_bit(gae, with_timeout):
    """The numpy restatement against ppo_cases._gae_torch evaluated in fp32 on the CPU."""
    _gae_torch = pc._gae_torch
    for Tn in pc.GAE_T:
        for n in pc.GAE_N:
            c = pc.gae_inputs(Tn, n)
            if n > 1:
                assert bool((c["done"][:, 0] == 1).all()) and c["nd"][0] == 1 and bool((c["done"][:, 1] == 0).all()) and c["nd"][1] == 0
            tmo = c["tmo"] if with_timeout else None
            got = pc.gae_reference(c["rew"], c["done"], c["val"], c["nv"], c["nd"], 0.99, 0.95, gae, tmo)
            want = _gae_torch(pc.T(c["rew"]), pc.T(c["done"]), pc.T(c["val"]), pc.T(c["nv"]), pc.T(c["nd"]), 0.99, 0.95, gae,
                              pc.T(tmo).bool() if with_timeout else None)
            for g_, w in zip(got, want):
                assert torch.equal(pc.T(g_), w), (Tn, n)
    assert 0 < pc.gae_inputs(33, 257)["tmo"].sum() < 33 * 257 and 0 < pc.gae_inputs(33, 257)["done"][:, 2:].sum()


# --------------------------------------------------------------------------- every case is asserted
def test_no_parametrised_case_is_empty_and_the_gpu_module_skips_nothing():
    for name in ("HEAD_A", "HEAD_B", "POLICY_CASES", "POLICY_CROSS", "VALUE_B", "GATHER_MB", "GATHER_OA", "GAE_T", "GAE_N"):
        assert len(getattr(pc, name)) > 0, name
    assert set(pc.HEAD_A) == {1, 3, 21, 33, 64} and set(pc.HEAD_B) == {1, 5, 257}
    assert pc.VALUE_B == [1, 255, 257, 65536 + 257] and pc.GATHER_MB == [1, 63, 64, 65, 4097 + 36]
    assert pc.GATHER_OA == [(1, 1), (13, 3), (88, 21), (8, 64)]
    assert {b for _, b in pc.POLICY_CROSS} == {65793, 16449, 4109, 2055, 8229}
    src = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "test_ppo_kernels_gpu.py")).read()
    for word in ("skip", "xfail", "importorskip"):
        assert word not in src, word
