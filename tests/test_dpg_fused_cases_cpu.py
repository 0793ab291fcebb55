"""The table of tests/dpg_fused_cases.py means what tests/test_dpg_fused_paths_gpu.py assumes: the mirror of the fused DPG
backward's eligibility, workspace layout and launch geometry agrees with the library's host-only calls, the pairs the path must
refuse are refused, the table reaches all four k_dx_slice<D, QPW> instances, both weight-staging branches, both kinds of qc
words and every batch threshold (each the smallest batch that crosses it), every case keeps the data rules and its exactness or
bound condition, and the checks pass on a plain numpy backward and fail on each wrong result they are there to catch.  No GPU
needed."""
import ctypes as C

import numpy as np
import pytest

import backward_cases as bc
import dpg_fused_cases as fc

F32, F64 = np.float32, np.float64

# (critic dims, critic nets, actor dims, actor nets) on either side of each rule of dpg_fused_ok
_TAKEN = [(fc.pair(p, A)[0], 2, fc.pair(p, A)[1], 1) for p in (1, 2, 3, 4) for A in (1, 5, 16)] + [([104, 512, 512, 256, 1], 2, [88, 512, 512, 256, 16], 1)]
_REFUSED = {
    "A = 17": ([25, 128, 128, 1], 2, [8, 128, 17], 1),
    "actor last hidden 64": ([13, 128, 128, 1], 2, [8, 64, 5], 1),
    "actor last hidden 512": ([13, 128, 128, 1], 2, [8, 512, 5], 1),
    "critic dims[1] = 96": ([13, 96, 128, 1], 2, [8, 128, 5], 1),
    "a two-layer critic": ([13, 128, 1], 2, [8, 128, 5], 1),
    "a two-net actor": ([13, 128, 128, 1], 2, [8, 128, 5], 2),
    "a one-net critic": ([13, 128, 128, 1], 1, [8, 128, 5], 1),
    "a one-layer actor": ([13, 128, 128, 1], 2, [128, 5], 1),
    "a critic input narrower than the action": ([4, 128, 128, 1], 2, [8, 128, 5], 1),
}
_BATCHES = [1, 3, 12, 127, 128, 129, 2048, 2049, 8192, 8193, 16384, 131072, 131073]


def _ok(L, cd, cn, ad, an, B):
    return int(L.lib.pqlk_dpg_fused_ok(C.byref(L.mlp_desc(cd, cn)), C.byref(L.mlp_desc(ad, an)), B))


# --------------------------------------------------------------------------- the mirror against the library
def test_mirror_agrees_with_the_library():
    from pql_amd import _lib as L
    assert int(L.lib.pqlk_dpg_fused_loss_parts()) == fc.LOSS_PARTS
    assert L.E_UNSUPPORTED == fc.E_UNSUPPORTED and L.E_WORKSPACE == fc.E_WORKSPACE
    for cd, cn, ad, an in _TAKEN + list(_REFUSED.values()):
        for B in _BATCHES + [0, -1]:
            assert _ok(L, cd, cn, ad, an, B) == int(fc.dpg_fused_ok(cd, cn, ad, an, B)), (cd, cn, ad, an, B)
    for B in _BATCHES + [c.B for c in fc.CASES]:
        assert int(L.lib.pqlk_dpg_fused_head_parts(B)) == fc.head_parts(B), B
        for cd in {tuple(t[0]) for t in _TAKEN}:
            d = L.mlp_desc(list(cd), 2)
            ws = fc.compact_ws(bc.max_hidden_ld(list(cd)), B)
            assert int(L.lib.pqlk_dpg_fused_mn_offset(C.byref(d), B)) == ws["mn"] == fc.mn_offset(list(cd), B), (cd, B)
            total = int(L.lib.pqlk_dpg_backward_ws_floats(C.byref(d), B))
            assert total == max(bc.bwd_ws_floats(list(cd), 2, B, 1), ws["total"]) == bc.dpg_ws_floats(list(cd), 2, B), (cd, B)
            # perm, mn and tie0 lie behind the two dZ buffers, tie0 ends inside the workspace
            assert ws["perm"] == 2 * ws["rows_cap"] * bc.max_hidden_ld(list(cd)) and ws["tie0"] + ws["rows_cap"] == ws["total"] <= total
    assert int(L.lib.pqlk_dpg_fused_head_parts(0)) == 0 == fc.head_parts(0)


@pytest.mark.parametrize("why", list(_REFUSED))
def test_refused_pairs(why):
    from pql_amd import _lib as L
    cd, cn, ad, an = _REFUSED[why]
    for B in (1, 256, 8192):
        assert _ok(L, cd, cn, ad, an, B) == 0 and not fc.dpg_fused_ok(cd, cn, ad, an, B), why


def test_every_pair_of_the_table_is_taken_and_one_batch_past_the_limit_is_refused():
    from pql_amd import _lib as L
    for c in fc.CASES + [fc.CHAIN]:
        assert _ok(L, c.cdims, 2, c.adims, 1, c.B) == 1, c.name
        assert _ok(L, c.cdims, 2, c.adims, 1, fc.MAX_B + 1) == 0, c.name
        A = c.adims[-1]
        assert c.cdims[0] == 8 + A and c.adims[0] == 8 and 0 <= c.col0 and c.col0 + A <= c.cdims[0]
        assert c.splits == bc.default_splits(c.B) and 1 <= c.splits <= 64


# --------------------------------------------------------------------------- what the table reaches
def test_table_reaches_every_instance_branch_and_threshold():
    assert {fc.instance(c) for c in fc.CASES} == set(fc.INSTANCES)
    assert fc.slice_instance(*fc.pair(2, 16)) == (4, 16) and fc.pair(2, 16)[0][1] % 512 != 0 and fc.pair(2, 16)[1][-2] == 256
    # A in {1, 5, 16} against both staging branches
    assert {(c.adims[-1], fc.staging(c.col0)) for c in fc.CASES} >= {(A, s) for A in (1, 5, 16) for s in ("vec", "scalar")}
    Bs = {c.B for c in fc.CASES}
    assert Bs >= {1, 3, 12, 32, 127, 128, 129, 256, 257, 2048, 2049, 8192, 8193, 16384, 131072}
    assert sum(1 for c in fc.CASES if c.B == fc.MAX_B) == 1
    big = [c for c in fc.CASES if c.B == fc.MAX_B][0]
    assert (big.cdims, big.adims) == fc.pair(1, big.adims[-1])                  # the smallest pair
    # the qc reads: scalar alone, vector alone, one vector word and one scalar word
    assert fc.qc_words(3) == {"scalar"} and fc.qc_words(8192) == {"vec"} and fc.qc_words(12) == {"vec", "scalar"}
    assert fc.qc_words(129) == {"scalar"} and fc.qc_words(4) == {"scalar"}
    # S, the head launch's grid and rows_cap_blk on both sides of their switches; the limit
    assert (fc.samples_per_thread(8192), fc.samples_per_thread(8193), fc.samples_per_thread(fc.MAX_B)) == (8, 16, 128)
    assert fc.samples_per_thread(fc.MAX_B + 1) // 8 > 16                        # more words than a thread holds: refused
    assert fc.head_launch(1) == (16, 16) and fc.head_launch(2048) == (256, 16) and fc.head_launch(2049) == (256, 17)
    assert fc.head_launch(fc.MAX_B) == (256, 1024)
    # owner patterns and run boundaries
    assert {c.owner for c in fc.CASES} == set(fc.OWNERS)
    mns = {c.name: fc.partition(fc.owners(c)[0])[2].tolist() for c in fc.CASES}
    cap = {c.name: fc.compact_ws(0, c.B)["rows_cap"] for c in fc.CASES}
    assert any(m[1] == 0 and m[3] == m[2] for m in mns.values())               # run 1 empty
    assert any(m[0] == 0 and m[2] == 0 for m in mns.values())                  # run 0 empty
    assert any(m[0] == 129 for m in mns.values())
    for B in (128, 129):                                                       # both runs full: every row a tie
        assert any(c.B == B and c.owner == "ties" and mns[c.name][3] == cap[c.name] for c in fc.CASES), B
    both = [c for c in fc.CASES if c.B == 256 and mns[c.name][:2] == [128, 128]]
    assert {c.owner for c in both} == {"halves", "alternate"}                  # c0 exactly 128, no tie: blocked and interleaved
    assert all(not (fc.owners(c)[0] == 3).any() for c in both)
    assert any(c.B < 128 and c.owner == "ties" for c in fc.CASES)
    # ties among ordinary rows: one run-0 mark per run-1 back reference
    assert any((r["tie0"] >= 0).any() and (r["tie0"] == -2).sum() == (r["tie0"] >= 0).sum() for r in (fc.reference(c.name) for c in fc.CASES[:6]))


@pytest.mark.parametrize("what", [t[0] for t in fc.THRESHOLDS])
def test_thresholds_are_the_smallest(what):
    _, pred, B = [t for t in fc.THRESHOLDS if t[0] == what][0]
    assert bc.smallest(pred, hi=1 << 18) == B
    assert B in {c.B for c in fc.CASES} or what == "refused"
    assert B - 1 in {c.B for c in fc.CASES}


# --------------------------------------------------------------------------- the partition law
def _partition_slowly(own):
    run0 = [m for m, o in enumerate(own) if o & 1]
    run1 = [m for m, o in enumerate(own) if o & 2]
    base1 = (len(run0) + 127) // 128 * 128
    used = base1 + (len(run1) + 127) // 128 * 128
    perm, tie0 = [-1] * used, [-1] * used
    for i, m in enumerate(run0):
        perm[i] = m
        if own[m] == 3:
            tie0[i] = -2
    for i, m in enumerate(run1):
        perm[base1 + i] = m
        if own[m] == 3:
            tie0[base1 + i] = run0.index(m)
    return perm, tie0, [len(run0), len(run1), base1, used]


@pytest.mark.parametrize("name", [c.name for c in fc.CASES if c.B <= 2049])
def test_partition_model_follows_the_law(name):
    c = fc.BY_NAME[name]
    own, q = fc.owners(c)
    perm, tie0, mn = fc.partition(own)
    sp, st, sm = _partition_slowly(own.tolist())
    assert perm.tolist() == sp and tie0.tolist() == st and mn.tolist() == sm
    assert mn[3] <= fc.compact_ws(0, c.B)["rows_cap"] and mn[2] % 128 == 0 and mn[3] % 128 == 0


# --------------------------------------------------------------------------- the data rules and the conditions of the checks
@pytest.mark.parametrize("name", fc.NAMES)
def test_case_keeps_the_data_rules_and_its_condition(name):
    c = fc.BY_NAME[name]
    p = fc.problem(name)
    A = c.adims[-1]
    hvals = bc.HVALS if c.data == "std" else bc.HINT
    for net in p.Hc + [p.Ha]:
        for h in net:
            assert np.isin(h, hvals).all()
    if c.data == "std" and p.rows >= 3:
        for h in (p.Hc[0][-1], p.Hc[1][-1], p.Ha[-1]):                          # every branch of ELU': 1, a fraction, 0
            f = bc.elu_prime(h)
            assert (f == 1).any() and ((f > 0) & (f < 1)).any() and (f == 0).any()
    for net in p.Wc + [p.Wa]:
        for w in net:
            assert np.isin(w, [-1, 0, 1]).all() and (w != 0).any()
    assert np.isin(p.tanh, bc.TVALS).all() and p.tanh.shape == (p.rows, A)
    assert np.array_equal(np.round(p.q), p.q) and np.abs(p.q).max() <= 4
    own = (p.q[0] <= p.q[1]).astype(np.uint8) | ((p.q[1] <= p.q[0]).astype(np.uint8) << 1)
    assert np.array_equal(own, p.own)
    assert p.rows == (fc.PERIOD if c.B % fc.PERIOD == 0 else c.B) and p.xa.shape == (p.rows, 64)
    ref = fc.reference(name)
    assert np.abs(ref["loss"]).max() <= 2 ** 24 and (ref["loss"] != 0).any()
    assert (ref["dz_a"] != 0).mean() > 0.05 and (ref["dxh"] != 0).any() and (ref["grads"] != 0).mean() > 0.03
    if bc.is_pow2(c.B):
        assert ref["exact"] and ref["bits"] <= 24, (name, ref["bits"])
        for k in ("dz_a", "dxh", "grads"):                                      # ... so every value is an fp32 number
            assert np.array_equal(ref[k].astype(F32).astype(F64), ref[k]), k
    else:
        assert not ref["exact"] and p.g == F64(F32(-1.0) / F32(c.B))
        assert ref["sharp"]["dz_a"] and ref["sharp"]["dxh"], (name, ref["sharp"])
        for k in ("dz_a", "dxh", "grads"):
            assert np.all(ref["E"][k][ref[k] != 0] > 0) and np.all(ref["E"][k] <= 2.0 ** -8 * np.abs(ref[k]).max()), k
        if not ref["sharp"]["grads"]:                                           # the row sums: exact at the neighbouring power of two
            twins = [t for t in fc.CASES if (t.cdims, t.adims, t.col0, t.owner) == (c.cdims, c.adims, c.col0, c.owner)
                     and bc.is_pow2(t.B) and c.B < 2 * t.B and t.B < 2 * c.B]
            assert twins, name


def test_norm_case_has_exact_squares():
    ref = fc.reference(fc.NORM_NAME)
    bits, k = bc.sumsq_bits(ref["grads"])
    assert bits <= 24 and (ref["grads"] != 0).sum() > 50, (bits, k)


def test_chained_case_is_exact_and_has_ties():
    p, (case, W, bias, x, H, q) = fc.chain_problem()
    ref = fc.reference_of(p)
    assert ref["exact"] and ref["bits"] <= 24 and (p.own == 3).any() and ref["mn"][0] > 0 and ref["mn"][1] > 0
    assert np.array_equal(x[:, fc.QC_O: fc.QC_O + fc.QC_A], p.tanh) and np.isin(p.tanh, bc.TVALS).all()
    for twin in (False, True):
        for B in fc.QC_BATCHES:
            case, W, bias, x, H, q = fc.qc_problem(B, twin)
            Z, _, _ = bc.exact_forward(case, W, bias, x)
            for n in range(2):
                for z in Z[n]:
                    assert ((z >= 0) | (z <= -32)).all() and np.array_equal(z * 2, np.round(z * 2))
            assert np.array_equal(q, np.round(q * 2) / 2) and (not twin or np.array_equal(q[1], q[0] + 4))


# --------------------------------------------------------------------------- the checks catch what they are there to catch
_FAULT_CASE = {f: "p1-A5-c7-B128-mixed" for f in fc.FAULTS}
_FAULT_CASE["fold_one_more"] = _FAULT_CASE["fold_one_less"] = "p3-A5-c8-B256-net0"    # tiles behind the rows in use; a live last tile


@pytest.mark.parametrize("name", sorted(set(_FAULT_CASE.values())) + ["p1-A5-c7-B3-ties", "p1-A5-c7-B127-mixed"])
def test_checks_pass_on_a_plain_numpy_backward(name):
    assert fc.check_all(fc.model_backward(name), fc.reference(name), name) <= 1.0


@pytest.mark.parametrize("fault", fc.FAULTS)
def test_checks_catch_the_planted_fault(fault):
    name = _FAULT_CASE[fault]
    with pytest.raises(AssertionError):
        fc.check_all(fc.model_backward(name, fault), fc.reference(name), f"{name} {fault}")


def test_checks_catch_a_wrong_partition_and_a_wrong_loss():
    name = "p1-A5-c7-B128-mixed"
    ref = fc.reference(name)
    for key, at, val in (("perm", 3, 5), ("tie0", int(np.flatnonzero(ref["tie0"] >= 0)[0]), -1), ("mn", 3, 384), ("loss", 0, 1.0), ("loss", 40, 0.0)):
        out = fc.model_backward(name)
        out[key] = out[key].copy()
        out[key][at] = val
        with pytest.raises(AssertionError):
            fc.check_all(out, ref, key)
