"""pqlk_action_noise_colored on the GPU against the NumPy model of its law (tests/colored_noise_model.py), to the bit: the state and the
noised action over a five-step sequence with rows that start over, per-row and scalar sigma, 16-byte aligned buffers and buffers one
float past a boundary, poison in front of and behind everything written; the tie with pqlk_action_noise at rho = 0; determinism."""
import functools

import numpy as np
import pytest
import torch

import colored_noise_model as M
from guarded import Guarded
from reduction_cases import SLACK
from support import T, bits, dev  # noqa: F401

pytestmark = pytest.mark.gpu
F = np.float32
POISON = -7777.0
SCALAR = 0.3
IDS = [f"{r}x{c}-R{R}-G{G}-off{o}" for r, c, R, G, o in M.SHAPES]


@functools.lru_cache(maxsize=None)
def _case(shape, per_row):
    """Inputs, tables and the model's sequence of a shape: computed once, shared by the aligned and the unaligned run."""
    rows, cols, R, G, env_offset = shape
    acts, draws, fresh, sigma = M.inputs(rows, cols, R, seed=rows + 7 * cols + R)
    rho, coef, w = M.case_tables(R, G)
    want = M.run(acts, draws, fresh, sigma if per_row else F(SCALAR), rho, coef, w, env_offset)
    for pair in want:   # shared by the runs that follow: left unchanged
        for a in pair:
            a.setflags(write=False)
    return acts, draws, fresh, sigma, rho, coef, w, want


class _Flags:
    """The fresh bytes with 7s in `off` bytes in front and SLACK bytes behind (off = 1: an odd address)."""

    def __init__(self, dev, values, off):
        import ctypes as C
        n = len(values)
        self.full = torch.full((off + n + SLACK,), 7, dtype=torch.uint8, device=dev)
        self.t = self.full[off: off + n]
        self.t.copy_(T(values))
        self.off, self.n, self.ptr = off, n, C.c_void_p(self.t.data_ptr())

    def intact(self):
        return bool((self.full[: self.off] == 7).all()) and bool((self.full[self.off + self.n:] == 7).all())


def _launch(dev, act, draw, std, scalar, rho, coef, G, R, env_offset, fresh, state, rows, cols, w, out):
    from pql_amd import _lib as L
    L.check(L.lib.pqlk_action_noise_colored(act.ptr, draw.ptr, None if std is None else std.ptr, scalar, rho.ptr, coef.ptr, G, R, env_offset,
                                            fresh.ptr, state.ptr, rows, cols, float(w), -1.0, 1.0, out.ptr, L.stream(dev)))


@pytest.mark.parametrize("off", [SLACK, 1], ids=["aligned", "one_float_past"])
@pytest.mark.parametrize("per_row", [True, False], ids=["std_rows", "scalar"])
@pytest.mark.parametrize("shape", M.SHAPES, ids=IDS)
def test_state_and_action_are_the_models_bits(dev, shape, per_row, off):
    """Every buffer the entry reads or writes sits `off` floats (the flags: bytes) behind poison and has poison behind it; `out` and
    `state` are contiguous, so in front and behind is all there is to guard.  Poison also fills `out` before every launch and the state
    before the first, whose rows are all fresh: nothing of either may be read."""
    rows, cols, R, G, env_offset = shape
    acts, draws, fresh, sigma, rho, coef, w, want = _case(shape, per_row)
    g = lambda a, **kw: Guarded(dev, a.shape, POISON, a, off, **kw)   # noqa: E731
    rho_d, coef_d = g(rho), g(coef)
    std = g(sigma) if per_row else None
    state = Guarded(dev, (rows, R, cols), POISON, off=off)
    for t in range(M.STEPS):
        act, draw = g(acts[t]), g(draws[t])
        fr = _Flags(dev, fresh[t], off)
        out = Guarded(dev, (rows, cols), POISON, off=off)
        _launch(dev, act, draw, std, SCALAR, rho_d, coef_d, G, R, env_offset, fr, state, rows, cols, w, out)
        got_out, got_state = out.host(), state.host()
        assert np.array_equal(bits(got_state), bits(want[t][1])), t
        assert np.array_equal(bits(got_out), bits(want[t][0])), t
        assert out.intact() and state.intact() and act.intact() and draw.intact() and fr.intact(), t
        assert np.array_equal(act.host(), acts[t]) and np.array_equal(draw.host(), draws[t]), t    # the inputs are read only
    assert rho_d.intact() and coef_d.intact() and (std is None or std.intact())
    last = want[-1][0]
    if rows * cols >= 100:   # the clamp took part on both sides, and most elements are inside
        assert (last == 1).any() and (last == -1).any() and (np.abs(last) < 1).sum() > last.size // 2


@pytest.mark.parametrize("per_row", [True, False], ids=["std_rows", "scalar"])
@pytest.mark.parametrize("shape", [(37, 16, 4, 3), (M.PAST_CAP, 1, 3, 5)], ids=["37x16", "past_the_cap"])
def test_rho_zero_is_the_white_kernels_bits(dev, shape, per_row):
    """ar1 with corr_min = corr_max = 0: rho = 0, coef = 1, w = 1, so n is the draw whether a row is fresh or not, and `out` is
    pqlk_action_noise's on the same act / draw / sigma -- over three steps, the state carried along."""
    from pql_amd import _lib as L
    rows, cols, G, env_offset = shape
    rho, coef, w = M.tables("ar1", groups=G, corr_min=0.0, corr_max=0.0)
    assert not rho.any() and (coef == 1).all() and w == 1
    acts, draws, fresh, sigma = M.inputs(rows, cols, 1, seed=91)
    g = lambda a: Guarded(dev, a.shape, POISON, a, SLACK)   # noqa: E731
    rho_d, coef_d, std = g(rho), g(coef), (g(sigma) if per_row else None)
    state = Guarded(dev, (rows, 1, cols), POISON, off=SLACK)
    for t in range(3):
        act, draw = g(acts[t]), g(draws[t])
        fr = _Flags(dev, fresh[t], SLACK)
        out, white = Guarded(dev, (rows, cols), POISON, off=SLACK), Guarded(dev, (rows, cols), POISON, off=SLACK)
        _launch(dev, act, draw, std, SCALAR, rho_d, coef_d, G, 1, env_offset, fr, state, rows, cols, w, out)
        L.check(L.lib.pqlk_action_noise(act.ptr, draw.ptr, None if std is None else std.ptr, SCALAR, rows, cols, -1.0, 1.0, white.ptr,
                                        L.stream(dev)))
        assert np.array_equal(bits(out.host()), bits(white.host())), t
        assert np.array_equal(bits(state.host().reshape(rows, cols)), bits(draws[t])), t
        assert out.intact() and state.intact()


@pytest.mark.parametrize("shape", [(37, 16, 1, 8, 3), (300, 16, 8, 1, 0)], ids=["ar1", "pink"])
def test_two_launches_on_equal_inputs_give_equal_bits(dev, shape):
    rows, cols, R, G, env_offset = shape
    acts, draws, fresh, sigma, rho, coef, w, _ = _case(shape, True)
    g = lambda a: Guarded(dev, a.shape, POISON, a, SLACK)   # noqa: E731
    start = np.random.default_rng(3).standard_normal((rows, R, cols)).astype(F)
    got = []
    for _ in range(2):
        state, out = g(start), Guarded(dev, (rows, cols), POISON, off=SLACK)
        fr = _Flags(dev, fresh[1], SLACK)
        _launch(dev, g(acts[1]), g(draws[1]), g(sigma), 0.0, g(rho), g(coef), G, R, env_offset, fr, state, rows, cols, w, out)
        got.append((out.host().copy(), state.host().copy()))
    assert np.array_equal(bits(got[0][0]), bits(got[1][0])) and np.array_equal(bits(got[0][1]), bits(got[1][1]))
    assert not np.array_equal(got[0][1], start)
