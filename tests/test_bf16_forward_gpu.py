"""The forward-only bf16-MFMA stack (pqlk_mlp_pack_bf16 / pqlk_mlp_forward_bf16) against the CPU model of its law
(tests/bf16_model.py).  Exact data: every row that is not ambiguous must meet the forward error bound of ONE fp32 dot product --
the output layer's -- because its hidden activations are the model's bit for bit.  Realistic data: the rms criterion.  Plus the
packed copy element for element, repeatability, independence of a row from its batch, and NaN containment.  `pytest -m gpu`."""
import functools

import pytest
import torch

import bf16_model as M
from support import dev  # noqa: F401

pytestmark = pytest.mark.gpu

TANH_ATOL = 1e-5   # the absolute bar of the fp32 actor forward: tests/test_kernels_gpu.py:369 (test_actor_module)


def build(dims, n_nets, W, b, dev):
    """-> (layout, arena on `dev` filled from W / b, refreshed PackedWeightsBf16)."""
    from pql_amd.models.mlp import ArenaLayout, PackedWeightsBf16
    lay = ArenaLayout(dims, n_nets)
    arena = torch.zeros(lay.total, device=dev)
    for n in range(n_nets):
        for l in range(lay.n_layers):
            lay.weight(arena, n, l).copy_(W[n][l])
            lay.bias(arena, n, l).copy_(b[n][l])
    return lay, arena, PackedWeightsBf16(lay, dev).refresh(arena)


@functools.lru_cache(maxsize=None)
def on_device(name):
    c = M.exact_case(name)
    dev = torch.device("cuda:0")
    return build(c["dims"], c["n_nets"], c["W"], c["b"], dev) + (c["x"].to(dev), None if c["draw"] is None else c["draw"].to(dev))


def run(lay, arena, pk, x, out_act, draw, with_out2):
    from pql_amd import _lib as L
    from pql_amd.models.mlp import mlp_forward_bf16_raw
    B, N = x.shape[0], lay.dims[-1]
    out = torch.full((lay.n_nets, B, lay.ld_out), 7.0, device=x.device)
    out2 = torch.full((B, L.ld(N) + 32), -3.0, device=x.device) if with_out2 else None
    mlp_forward_bf16_raw(lay, arena, pk, x, out_act, draw, M.NOISE_STD, M.NOISE_CLIP, out, None if out2 is None else out2[:, 8:])
    return out, out2


def check_rows(name, y, B):
    """The pass criteria of the exact data on the first B rows of case `name`; y: (nets, B, ld_out) from the kernel."""
    c = M.exact_case(name)
    m, N = c["model"], c["dims"][-1]
    amb = m["ambiguous"][:B]
    assert int(amb.sum()) <= 0.10 * B
    y = y.cpu()
    assert not y[:, :, N:].any(), "pad columns must be zero"
    assert torch.isfinite(y).all()
    tol = M.out_tolerance(c["dims"], m["bound"][:, :B]) + (TANH_ATOL if c["out_act"] != M.ACT_NONE else 0.0)
    err = (y[:, :, :N].double() - m["out"][:, :B]).abs()
    worst = float((err / tol)[:, ~amb].max()) if (~amb).any() else 0.0
    print(f"{name} B={B}: ambiguous {int(amb.sum())}, worst |y - o64| / bound {worst:.3f}, max err {float(err[:, ~amb].max()) if (~amb).any() else 0:.3e}")
    assert worst <= 1.0, (name, B, worst)


@pytest.mark.parametrize("B", M.BATCHES)
@pytest.mark.parametrize("name", sorted(M.EXACT_CASES))
def test_exact_data_meet_the_output_layers_fp32_bound(dev, name, B):
    lay, arena, pk, x, draw = on_device(name)
    c = M.exact_case(name)
    policy = c["n_nets"] == 1
    y, out2 = run(lay, arena, pk, x[:B].contiguous(), c["out_act"], None if draw is None else draw[:B].contiguous(), policy)
    check_rows(name, y, B)
    if policy:   # the copy: same bits in the action columns, nothing written around them
        N = c["dims"][-1]
        assert torch.equal(out2[:, 8:8 + N], y[0, :, :N])
        assert bool((out2[:, :8] == -3.0).all()) and bool((out2[:, 8 + N:] == -3.0).all())


def test_policy_writes_its_actions_into_the_tile_it_read(dev):
    """out2 = the action columns of the input tile itself (what the V-learner does): same actions as with a separate out2."""
    name = "p88_256_128_16_noise"
    lay, arena, pk, x, draw = on_device(name)
    from pql_amd.models.mlp import mlp_forward_bf16_raw
    B, O, A = 257, 88, 16
    tile = torch.zeros((B, 128), device=dev)
    tile[:, :O] = x[:, :O]
    tile[:, O:] = 1e30
    y = mlp_forward_bf16_raw(lay, arena, pk, tile, M.ACT_TANH_NOISE, draw, M.NOISE_STD, M.NOISE_CLIP, None, tile[:, O:])
    check_rows(name, y, B)
    assert torch.equal(tile[:, O:O + A], y[0, :, :A]) and torch.equal(tile[:, :O], x[:, :O])
    assert bool((tile[:, O + A:] == 1e30).all())


@pytest.mark.parametrize("name", ["c24_128_64_51", "p88_256_128_16_tanh", "c104_512_256_1"])
def test_packed_copy_is_rne_of_the_arena(dev, name):
    lay, arena, pk, _, _ = on_device(name)
    c = M.exact_case(name)
    got = M.unpack(pk.tensor.cpu(), c["dims"], c["n_nets"])
    for n in range(c["n_nets"]):
        for l in range(lay.n_layers):
            want = c["W"][n][l].to(torch.bfloat16).view(torch.int16)
            assert torch.equal(got[n][l], want), (name, n, l)


def test_packed_copy_rounds_ties_to_even_and_keeps_specials(dev):
    dims = [16, 32, 1]
    W = [[torch.zeros((32, 16)), torch.zeros((1, 32))]]
    vals = torch.tensor([1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, -(1.0 + 2.0 ** -8), 1.0 + 2.0 ** -8 + 2.0 ** -23, float("inf"), -float("inf"),
                         3.4e38, 1e-40, -0.0, float("nan")])
    W[0][0][0, :10] = vals
    b = [[torch.zeros(32), torch.zeros(1)]]
    lay, arena, pk = build(dims, 1, W, b, dev)
    got = M.unpack(pk.tensor.cpu(), dims, 1)[0][0][0, :10]
    want = vals.to(torch.bfloat16).view(torch.int16)
    assert torch.equal(got[:9], want[:9])
    assert (int(got[9]) & 0x7F80) == 0x7F80 and (int(got[9]) & 0x7F) != 0   # NaN stays NaN


def test_same_bits_every_launch_and_for_a_row_alone(dev):
    for name in ("c104_512_256_1", "p88_256_128_16_noise", "c24_128_64_51"):
        lay, arena, pk, x, draw = on_device(name)
        c = M.exact_case(name)
        y0, _ = run(lay, arena, pk, x, c["out_act"], draw, False)
        y1, _ = run(lay, arena, pk, x, c["out_act"], draw, False)
        assert torch.equal(y0.view(torch.int32), y1.view(torch.int32)), name
        for row in (0, 100, 256):
            ya, _ = run(lay, arena, pk, x[row:row + 1].contiguous(), c["out_act"], None if draw is None else draw[row:row + 1].contiguous(), False)
            assert torch.equal(ya[:, 0].view(torch.int32), y0[:, row].view(torch.int32)), (name, row)


def test_a_nan_row_stays_a_nan_row(dev):
    for name in ("c24_128_128_1", "p88_256_128_16_tanh"):
        lay, arena, pk, x, draw = on_device(name)
        c = M.exact_case(name)
        N = c["dims"][-1]
        y0, _ = run(lay, arena, pk, x, c["out_act"], draw, False)
        xn = x.clone()
        xn[70, 3] = float("nan")
        y1, _ = run(lay, arena, pk, xn, c["out_act"], draw, False)
        assert bool(torch.isnan(y1[:, 70, :N]).all()) and not y1[:, 70, N:].any()
        keep = torch.arange(257, device=dev) != 70
        assert torch.equal(y1[:, keep].view(torch.int32), y0[:, keep].view(torch.int32)), name
        xi = x.clone()
        xi[5, 0] = float("inf")
        y2, _ = run(lay, arena, pk, xi, c["out_act"], draw, False)
        assert not bool(torch.isfinite(y2[:, 5, :N]).all()) or c["out_act"] != M.ACT_NONE   # inf (or inf - inf = NaN) reaches a linear output
        assert torch.equal(y2[:, keep & (torch.arange(257, device=dev) != 5)].view(torch.int32),
                           y0[:, keep & (torch.arange(257, device=dev) != 5)].view(torch.int32))


@pytest.mark.parametrize("scale", (1, 3))
@pytest.mark.parametrize("name", sorted(M.REAL_CASES))
def test_realistic_data_meet_the_rms_criterion(dev, name, scale):
    """rms(y - o64) <= 1/8 rms(o64 - unrounded network): default-init weights x1 and x3, inputs clamp(N(0,1), +-5), B = 256."""
    c = M.real_case(name, scale)
    lay, arena, pk = build(c["dims"], c["n_nets"], c["W"], c["b"], dev)
    y, _ = run(lay, arena, pk, c["x"].to(dev), c["out_act"], None, False)
    N = c["dims"][-1]
    got, dist = M.rms(y.cpu()[:, :, :N].double() - c["o64"]), M.rms(c["o64"] - c["fp32"])
    print(f"{name} x{scale}: rms(y - o64) {got:.3e}, rms(o64 - fp32) {dist:.3e}, ratio {got / dist:.4f}")
    assert got <= dist / 8
    assert not y.cpu()[:, :, N:].any()
