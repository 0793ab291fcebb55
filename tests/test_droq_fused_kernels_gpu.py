"""`pqlk_lnmlp_drop_forward{, _bf16}` (csrc/fwd_ln.hip, fwd_ln_bf16.hip) against float64 torch under the numpy mask model (droq_cases.py).
fp32: the per-layer dropout forward's own error against that model is the bar, e_new <= 4 e_parent (they differ in fp32 summation order).
bf16: rms(Q - o_law) <= 1/8 rms(o_law - o_full): the bf16 law and the unrounded network under the same masks (test_lnmlp_bf16_gpu.py's margin)."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

import droq_cases as dc
from support import T, dev  # noqa: F401

pytestmark = pytest.mark.gpu

# hidden, obs + act, m: one tile, idle waves; a row past a tile / a 64-row block; ragged tiles, VPL 2 and 4; R = 2 edge, VPL 8; R = 1, VPL 16
SHAPES = [([32], 3, 1), ([32], 3, 33), ([64, 32], 40, 65), ([160, 96], 104, 129), ([512, 512, 256], 104, 65), ([1024], 104, 33)]
CASES = [(*s, p) for s in SHAPES for p in (0.01, 0.5)]
CALL, STREAM = (0xA5 << 24) | 70001, 1            # the tag's high word in play; dc.SEED has both key words in play
TAG_BASE = dc.make_tag(CALL, STREAM, 0, 0)
TAIL = 64   # sentinel floats behind every output block


def _critic(hidden, k, m, p, dev, **kw):
    """The critic at call CALL of stream STREAM, and an input of m rows."""
    from pql_amd.models.droq import DoubleQDropoutLayerNorm
    from pql_amd.models.mlp import pad_cols
    torch.manual_seed(len(hidden) * 1000 + k)
    q = DoubleQDropoutLayerNorm((k - 1,), 1, hidden, dropout=p, seed=dc.SEED, **kw).to(dev)
    for n in range(2):
        for l in range(len(hidden)):
            q.norm_param(n, l, "gamma").add_(0.2 * torch.randn(hidden[l], device=dev))
            q.norm_param(n, l, "beta").copy_(0.2 * torch.randn(hidden[l], device=dev))
    q.drop_calls, q.drop_stream = CALL, STREAM
    return (q.refresh() if q.packed is not None else q), pad_cols(torch.randn(m, k, device=dev), (k + 31) // 32 * 32)


def _reference(q, x, p, rounded=False):
    """{("y", n, l): (m, w), ("q", n): (m,)} in float64 under the model's masks; rounded: the bf16 law."""
    rnd = (lambda t: t.to(torch.bfloat16).double()) if rounded else (lambda t: t.double())
    out, H, s = {}, q.n_layers - 1, float(dc.scale(p))
    for n in range(2):
        a = rnd(x)
        for l in range(H):
            z = F.linear(a, rnd(q.weight(n, l)), q.bias(n, l).double())
            keep = T(dc.keep_mask(dc.SEED, dc.make_tag(CALL, STREAM, n, l), p, *z.shape)).to(x.device)
            u = torch.where(keep, z * s, torch.zeros_like(z))
            a = rnd(F.elu(F.layer_norm(u, u.shape[1:], q.norm_param(n, l, "gamma").double(), q.norm_param(n, l, "beta").double(), 1e-5)))
            out["y", n, l] = a
        out["q", n] = F.linear(a, rnd(q.weight(n, H)), q.bias(n, H).double())[:, 0]
    return out


def _launch(q, x, drop, stash=False, bf16=False, want=0):
    """The entry itself on sentinel-filled blocks -> (Q, slab); drop None: the plain entry; an error must leave the outputs untouched."""
    from pql_amd import _lib as L
    m, st = x.shape[0], L.stream(x.device)
    qb = torch.full((2 * m * 32 + TAIL,), 7.0, device=x.device)
    slab = torch.full((int(L.lib.pqlk_lnmlp_stash_floats(C.byref(q.fused), m)) + TAIL,), 7.0, device=x.device) if stash else None
    args = (C.byref(q.fused), L.ptr(q.arena.data), *((L.ptr(q.packed),) if bf16 else ()), L.ptr(x), x.stride(0), m, 1e-5, *(drop or ()),
            *(() if bf16 else (L.ptr(slab),)), L.ptr(qb), st)
    assert getattr(L.lib, "pqlk_lnmlp" + ("_drop" if drop else "") + "_forward" + ("_bf16" if bf16 else ""))(*args) == want
    assert bool((qb[-TAIL:] == 7.0).all()) and (slab is None or bool((slab[-TAIL:] == 7.0).all()))   # nothing past row m is touched
    assert bool((qb[:-TAIL] != 7.0).all()) if want == 0 else bool((qb == 7.0).all()) and (slab is None or bool((slab == 7.0).all()))
    return qb[:-TAIL].view(2, m, 32), slab


@pytest.mark.parametrize("hidden, k, m, p", CASES, ids=str)
def test_fp32_launch(hidden, k, m, p, dev):
    from pql_amd import _lib as L
    (per, x), (fus, _) = _critic(hidden, k, m, p, dev), _critic(hidden, k, m, p, dev, fused_forward=True)
    fus.arena.data.copy_(per.arena.data)
    H, drop = len(hidden), (p, dc.SEED, TAG_BASE)
    ref = _reference(per, x[:, :k], p)
    q_per = per.forward_raw(x)
    ws = per._workspace(m, dev)
    qf, _ = _launch(fus, x, drop, stash=True)
    assert bool((qf[:, :, 1:] == 0).all())             # pad columns of Q
    assert torch.equal(fus.forward_raw(x), qf) and fus.drop_calls == CALL + 1   # the module's launch is this one; its stash, by its views:
    wf = fus._workspace(m, dev)
    got, old = ({("q", n): t[n, :, 0] for n in range(2)} for t in (qf, q_per))
    for n in range(2):
        for l in range(H):
            z, y = wf["z"][(n, l)], wf["y"][(n, l)]
            got["y", n, l], old["y", n, l] = y, ws["y"][(n, l)][:, :hidden[l]]
            # the stash is the pre-dropout z: ln.hip's dropout row kernel on it, with the tag of (n, l), gives the stashed y, mean, rstd
            y2, mean, rstd = torch.empty_like(y), torch.empty(m, device=dev), torch.empty(m, device=dev)
            L.check(L.lib.pqlk_drop_ln_elu_forward(L.ptr(z), hidden[l], m, hidden[l], L.ptr(fus.norm_param(n, l, "gamma")),
                                                   L.ptr(fus.norm_param(n, l, "beta")), 1e-5, p, dc.SEED, dc.make_tag(CALL, STREAM, n, l),
                                                   L.ptr(y2), L.ptr(mean), L.ptr(rstd), L.stream(dev)))
            assert torch.equal(y2, y) and torch.equal(mean, wf["mean"][(n, l)]) and torch.equal(rstd, wf["rstd"][(n, l)])
    for kind in [("q",), *(("y", l) for l in range(H))]:   # e_new <= 4 e_parent per quantity, both nets together
        keys = [(kind[0], n, *kind[1:]) for n in range(2)]
        e_new, e_parent = (max(float((d[key].double() - ref[key]).abs().max()) for key in keys) for d in (got, old))
        print(f"{hidden} k={k} m={m} p={p} {kind}: e_new {e_new:.3e} e_parent {e_parent:.3e}")
        assert e_new <= 4.0 * e_parent, (kind, e_new, e_parent)
    assert torch.equal(_launch(fus, x, drop)[0], qf)    # no stash: the same Q
    (q0, slab0), (q1, slab1) = _launch(fus, x, (0.0, dc.SEED, TAG_BASE), stash=True), _launch(fus, x, None, stash=True)
    assert torch.equal(q0, q1) and torch.equal(slab0, slab1)   # p = 0: the plain entry's bits


@pytest.mark.parametrize("hidden, k, m, p", CASES, ids=str)
def test_bf16_launch(hidden, k, m, p, dev):
    (q, x), drop = _critic(hidden, k, m, p, dev, fused_forward=True, target_dtype="bfloat16"), (p, dc.SEED, TAG_BASE)
    out = q.forward_raw(x, stash=False).clone()
    assert q.drop_calls == CALL + 1 and torch.equal(out, _launch(q, x, drop, bf16=True)[0]) and not bool(out[:, :, 1:].any())
    o_law, o_full = (torch.stack([r["q", 0], r["q", 1]]) for r in (_reference(q, x[:, :k], p, rounded) for rounded in (True, False)))
    rms = lambda t: float(t.pow(2).mean().sqrt())  # noqa: E731
    e, bar = rms(out[:, :, 0].double() - o_law), rms(o_law - o_full)
    print(f"{hidden} k={k} m={m} p={p}: rms(Q - o_law) {e:.3e}, rms(o_law - o_full) {bar:.3e}, ratio {e / bar:.4f}")
    assert e <= bar / 8
    assert torch.equal(_launch(q, x, (0.0, dc.SEED, TAG_BASE), bf16=True)[0], _launch(q, x, None, bf16=True)[0])   # p = 0
    bad_row, x2 = m // 2, x.clone()
    x2[bad_row, 1] = float("nan")
    bad = _launch(q, x2, drop, bf16=True)[0]
    others = torch.arange(m, device=dev) != bad_row
    assert bool(bad[:, bad_row, 0].isnan().all()) and torch.equal(bad[:, others], out[:, others])


def test_refusals_leave_the_outputs_alone(dev):
    from pql_amd import _lib as L
    q, x = _critic([64, 32], 40, 33, 0.01, dev, fused_forward=True, target_dtype="bfloat16")
    for drop in ((1.0, dc.SEED, TAG_BASE), (float("nan"), dc.SEED, TAG_BASE), (0.01, dc.SEED, 1)):   # p = 1, p = NaN, tag_base = 1
        _launch(q, x, drop, stash=True, want=L.E_SHAPE)
        _launch(q, x, drop, bf16=True, want=L.E_SHAPE)
