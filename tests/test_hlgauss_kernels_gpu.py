"""pqlk_hlgauss_ce_loss and pqlk_hlgauss_ce_loss_per (k_hlgauss_ce<NJ, PER>) on the GPU against tests/hlgauss_cases.py: the exact
design bit for bit at every NJ, at one row, at a ragged block, at several blocks and past the grid cap; the generic design within the
derived forward bound of the float64 reference; the weighted entry's identity with the plain one; reproducibility; the loss ring;
the error codes; non-finite rows.

Every buffer a kernel writes has SLACK floats of poison behind it and poison pad columns, which must come back intact, or zero where
include/pqlk.h says "written as zero"; every input has IN_BIG in its slack and its pad columns, which would move the result."""
import numpy as np
import pytest
import torch

import hlgauss_cases as hc
import reduction_cases as rc
from guarded import Guarded
from support import T, bits, dev  # noqa: F401

pytestmark = pytest.mark.gpu

POISON = rc.POISON
_CASES = {}


def _exact(B, K, per):
    if (B, K, per) not in _CASES:
        _CASES[(B, K, per)] = hc.exact_case(B, K, per)
    return _CASES[(B, K, per)]


def _generic(K, per):
    """(case, float64 reference, bounds), computed once and shared; nobody writes to them."""
    key = ("generic", K, per)
    if key not in _CASES:
        case = hc.generic_case(hc.GENERIC_B, K, 100 + K, per=per)
        ref = hc.ref_of(case, per)
        _CASES[key] = (case, ref, hc.hl_bounds(ref, hc.loss_blocks(hc.GENERIC_B)))
    return _CASES[key]


def _ld(K):
    from pql_amd import _lib as L
    return int(L.lib.pqlk_ld(K))


def _launch(dev, case, ld, per, target=True, ring=False, slot=None, ring_len=5):
    """One launch on guarded buffers -> dict of host arrays (dy without its pad columns, pad, target, parts, loss, abs_td, ring)."""
    from pql_amd import _lib as L
    B, K = case["B"], case["K"]

    def padded(x):
        g = Guarded(dev, (2, B, ld), rc.IN_BIG)
        g.t[:, :, :K] = T(x).to(dev)
        return g

    def vec(x):
        return Guarded(dev, x.shape, rc.IN_BIG, x)

    lg, lt = padded(case["logits"]), padded(case["logits_t"])
    rew, done, z = vec(case["rew"]), vec(case["done"]), vec(case["z"])
    parts = int(L.lib.pqlk_loss_parts(B, K))
    assert parts == hc.loss_blocks(B)
    dy, scr, tgt = Guarded(dev, (2, B, ld), POISON), Guarded(dev, (parts,), POISON), Guarded(dev, (B, K), POISON)
    lo, td = Guarded(dev, (ring_len if slot is not None else 1,), POISON), Guarded(dev, (B,), POISON)
    slot_dev = None if slot is None else torch.tensor([slot], dtype=torch.int32, device=dev)
    head = (lg.ptr, lt.ptr, ld, K, rew.ptr, done.ptr, z.ptr, case["gamma_n"], case["v_min"], case["v_max"], case["sigma"], B, dy.ptr,
            lo.ptr if (ring or slot is not None) else None, L.ptr(slot_dev), ring_len if slot is not None else 0, tgt.ptr if target else None,
            scr.ptr)
    if per:
        w, wmax = vec(case["w"]), vec(case["wmax"])
        L.check(L.lib.pqlk_hlgauss_ce_loss_per(*head, w.ptr, wmax.ptr, td.ptr, L.stream(dev)))
    else:
        L.check(L.lib.pqlk_hlgauss_ce_loss(*head, L.stream(dev)))
    torch.cuda.synchronize()
    for name, g in (("dy", dy), ("scratch", scr), ("target_out", tgt), ("loss_out", lo), ("abs_td_out", td)):
        assert g.intact(), f"a guard word behind {name} was overwritten"
    return dict(dy=dy.host()[:, :, :K].copy(), pad=dy.host()[:, :, K:].copy(), t=tgt.host(), parts=scr.host(), loss=lo.host(), abs_td=td.host())


def _same(a, b):
    return np.array_equal(bits(np.asarray(a, np.float32)), bits(np.asarray(b, np.float32)))


# =========================================================================== the exact design: bits
@pytest.mark.parametrize("B", hc.EXACT_B)
@pytest.mark.parametrize("K", hc.EXACT_KS)
def test_exact_design_bitwise(dev, K, B):
    """dy, target_out, the per-block partials, the folded loss and |TD| are the closed form's bits: at ld = pqlk_ld(K) and one wider,
    on the plain entry and on the weighted one with w in {0.25, 0.5, 1}, wmax = 1."""
    for per in (False, True):
        case = _exact(B, K, per)
        for ld in (_ld(K), _ld(K) + 64):
            got = _launch(dev, case, ld, per, ring=True)
            where = f"K={K} B={B} ld={ld} per={per}"
            assert _same(got["t"], case["t"]), where
            assert _same(got["dy"], case["dy"]), where
            assert (got["pad"] == 0).all(), where
            assert _same(got["parts"], case["parts"]), where
            assert _same(got["loss"], [case["loss"]]), where
            if per:
                assert _same(got["abs_td"], case["abs_td"]), where      # exact here: |z_h - y|
            else:
                assert (got["abs_td"] == POISON).all(), where           # the plain entry never touches abs_td_out
        # loss_out = NULL leaves exactly pqlk_loss_parts(b, k) partials and no loss; target_out = NULL changes nothing else
        bare = _launch(dev, case, _ld(K), per, target=False, ring=False)
        assert (bare["t"] == POISON).all() and (bare["loss"] == POISON).all()
        assert _same(bare["parts"], case["parts"]) and _same(bare["dy"], case["dy"])


# =========================================================================== the generic design: the derived bound
@pytest.mark.parametrize("per", [False, True])
@pytest.mark.parametrize("K", hc.GENERIC_KS)
def test_generic_design_within_the_bound(dev, K, per):
    """target_out, dy, the loss and |TD| within hl_bounds of the float64 reference; the largest observed error is printed beside
    the bound (DESIGN 10 f25 records both)."""
    case, ref, bound = _generic(K, per)
    got = _launch(dev, case, _ld(K), per, ring=True)
    err_t, err_dy = np.abs(got["t"] - ref["t"]), np.abs(got["dy"] - ref["dy"])
    err_loss = abs(float(got["loss"][0]) - ref["loss"])
    line = (f"hlgauss generic K={K} per={per}: t {err_t.max():.3e} (bound at that element {bound['t'].flat[err_t.argmax()]:.3e}, worst ratio "
            f"{(err_t / bound['t']).max():.3e})  dy {err_dy.max():.3e} (ratio {(err_dy / bound['dy']).max():.3e})  "
            f"loss {err_loss:.3e} (bound {bound['loss']:.3e})")
    if per:
        err_td = np.abs(got["abs_td"] - ref["abs_td"])
        line += f"  abs_td {err_td.max():.3e} (ratio {(err_td / bound['abs_td']).max():.3e})"
    print(line)
    assert np.isfinite(got["dy"]).all() and np.isfinite(got["t"]).all() and (got["pad"] == 0).all()
    assert (err_t <= bound["t"]).all()
    assert (err_dy <= bound["dy"]).all()
    assert err_loss <= bound["loss"]
    if per:
        assert (err_td <= bound["abs_td"]).all()
    assert np.abs(got["t"].astype(np.float64).sum(axis=1) - 1.0).max() <= K * bound["t"].max()


@pytest.mark.parametrize("K", hc.GENERIC_KS)
def test_gradient_against_float64_autograd(dev, K):
    """dy against torch.autograd of the soft-target cross-entropy in float64, same bound."""
    case, ref, bound = _generic(K, True)
    t64 = lambda a: torch.from_numpy(np.asarray(a, np.float64))   # noqa: E731
    x = t64(case["logits"]).requires_grad_(True)
    loss = hc.hl_torch(x, t64(case["logits_t"]), t64(case["rew"]), t64(case["done"]), t64(case["z"]), case["gamma_n"], case["v_min"],
                       case["v_max"], case["sigma"], wh=t64(ref["wh"]))
    (grad,) = torch.autograd.grad(loss, x)
    got = _launch(dev, case, _ld(K), True, ring=True)
    err = np.abs(got["dy"] - grad.numpy())
    print(f"hlgauss autograd K={K}: dy {err.max():.3e} (worst ratio to the bound {(err / bound['dy']).max():.3e})")
    assert (err <= bound["dy"]).all()
    assert abs(float(got["loss"][0]) - float(loss.detach())) <= bound["loss"]


# =========================================================================== identities
@pytest.mark.parametrize("K", hc.GENERIC_KS)
def test_unit_weights_give_the_plain_entrys_bits_and_launches_repeat(dev, K):
    case, _, _ = _generic(K, False)
    ones = dict(case, w=np.ones(case["B"], np.float32), wmax=np.ones(1, np.float32))
    plain, again, weighted = (_launch(dev, case, _ld(K), False, ring=True), _launch(dev, case, _ld(K), False, ring=True),
                              _launch(dev, ones, _ld(K), True, ring=True))
    for name in ("dy", "t", "parts", "loss"):
        assert _same(plain[name], again[name]), name        # two launches, the same bits
        assert _same(plain[name], weighted[name]), name     # every w and wmax 1.0: the plain entry's bits
    two = [_launch(dev, _generic(K, True)[0], _ld(K), True, ring=True) for _ in range(2)]
    for name in ("dy", "t", "parts", "loss", "abs_td"):
        assert _same(two[0][name], two[1][name]), name


def test_ring_slot(dev):
    """slot_dev[0] % ring_len names the ring's slot; the others stay as they were."""
    case = _exact(5, 5, False)
    for slot, want in ((0, 0), (3, 3), (7, 2)):
        got = _launch(dev, case, 32, False, slot=slot)
        assert _same(got["loss"][want: want + 1], [case["loss"]])
        assert (np.delete(got["loss"], want) == POISON).all()


def test_non_finite_rows_are_nan_and_stay_in_their_rows(dev):
    """A non-finite reward, done flag or logit (current or target) makes the row's dy, target_out, |TD| and the loss NaN; the rows
    beside it keep their bits and no guard word moves."""
    K, B = 101, 37
    base = hc.generic_case(B, K, 9, per=True)
    clean = _launch(dev, base, _ld(K), True, ring=True)
    spoil = [("rew", (3,), np.nan), ("rew", (8,), np.inf), ("done", (12,), np.nan), ("logits", (0, 17, 100), np.nan), ("logits", (1, 21, 64), np.inf),
             ("logits", (0, 23, 5), -np.inf), ("logits_t", (1, 29, 70), np.nan), ("logits_t", (0, 33, 0), -np.inf)]
    case = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in base.items()}
    rows = []
    for name, at, value in spoil:
        case[name][at] = value
        rows.append(at[0] if len(at) == 1 else at[1])
    got = _launch(dev, case, _ld(K), True, ring=True)
    ok = np.setdiff1d(np.arange(B), rows)
    for name in ("t", "abs_td"):
        assert np.isnan(got[name][rows]).all(), name
        assert _same(got[name][ok], clean[name][ok]), name
    assert np.isnan(got["dy"][:, rows]).all() and _same(got["dy"][:, ok], clean["dy"][:, ok])
    assert (got["pad"] == 0).all() and np.isnan(got["loss"]).all()


# =========================================================================== errors, before any launch
def test_error_codes_and_no_launch(dev):
    from pql_amd import _lib as L
    B, K, ld = 5, 5, 32
    f = lambda n, v=POISON: torch.full((n,), v, device=dev)   # noqa: E731
    bufs = dict(logits=f(2 * B * ld), logits_t=f(2 * B * ld), rew=f(B), done=f(B), z=f(K), dy=f(2 * B * ld), lo=f(1), tgt=f(B * K), scr=f(8),
                w=f(B), wmax=f(1), td=f(B))
    slot = torch.zeros(1, dtype=torch.int32, device=dev)

    def call(per, **kw):
        a = dict(ld=ld, k=K, v_min=-10.0, v_max=10.0, sigma=0.75, b=B, slot=None, ring_len=0, null=())
        a.update(kw)
        p = {n: (None if n in a["null"] else L.ptr(t)) for n, t in bufs.items()}
        head = (p["logits"], p["logits_t"], a["ld"], a["k"], p["rew"], p["done"], p["z"], 0.97, a["v_min"], a["v_max"], a["sigma"], a["b"], p["dy"],
                p["lo"], a["slot"], a["ring_len"], p["tgt"], p["scr"])
        if per:
            return L.lib.pqlk_hlgauss_ce_loss_per(*head, p["w"], p["wmax"], p["td"], L.stream(dev))
        return L.lib.pqlk_hlgauss_ce_loss(*head, L.stream(dev))

    for per in (False, True):
        for name in ("logits", "logits_t", "rew", "done", "z", "dy", "scr") + (("w", "wmax", "td") if per else ()):
            assert call(per, null=(name,)) == L.E_NULL, name
        for kw in (dict(b=0), dict(b=-3), dict(k=1), dict(sigma=0.0), dict(sigma=-0.75), dict(sigma=float("nan")), dict(v_max=-10.0),
                   dict(v_min=10.0, v_max=-10.0), dict(slot=L.ptr(slot), ring_len=0)):
            assert call(per, **kw) == L.E_SHAPE, kw
        assert call(per, k=L.C51_MAX_ATOMS + 1, ld=512) == L.E_UNSUPPORTED
        for kw in (dict(ld=48), dict(ld=0), dict(k=33, ld=32)):
            assert call(per, **kw) == L.E_ALIGN, kw
    torch.cuda.synchronize()
    for name in ("dy", "lo", "tgt", "scr", "td"):
        assert bool((bufs[name] == POISON).all()), name      # nothing was launched on an error
    assert call(False, null=("w", "wmax", "td", "lo", "tgt")) == L.OK      # optional on the plain entry (and never read)
    torch.cuda.synchronize()
    assert bool((bufs["dy"].view(2, B, ld)[:, :, K:] == 0).all()) and bool((bufs["scr"][2:] == POISON).all())
    for name in ("lo", "tgt", "td"):
        assert bool((bufs[name] == POISON).all()), name
