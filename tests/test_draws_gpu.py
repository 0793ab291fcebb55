"""pqlk_philox_draws (pql_amd/csrc/philox.hip) over the case table of tests/draw_cases.py: every index equal to the numpy model of the
law, every normal within NORMAL_BAR of its float64 model, in guarded, sentinel-filled buffers; each chunk against a launch of its
own, the step_dev forms against the NULL form, and -- where pql_amd.utils.rng.verified says the kernel is torch's stream -- every case
bit for bit against the torch calls it replaces, with the 64-bit seed, the offsets around the counter's carry and the second trip
that tests/test_kernels_gpu.py::test_philox_draws_are_torchs_own_numbers does not reach.  tests/test_draw_cases_cpu.py shows the
checks used here rejecting eleven wrong laws.  Then DrawAhead (pql_amd/utils/rng.py) on the device, against the torch stream."""
import numpy as np
import pytest
import torch

import draw_cases as dc
from guarded import Guarded
from support import dev  # noqa: F401

pytestmark = pytest.mark.gpu

# The bar on |kernel - float64 model| of a normal.  It is not a property of this project's kernel but of Box-Muller in float32, so it
# is taken from ATen's own normal_: its largest distance from the same model at the same elements, measured on an MI355X on the
# first run of this file over all cases of draw_cases.cases(), was 2.643e-06 (case cap-s64-o4-null, 1 048 578 normals; 2.512e-06
# over the 4 194 306 of four-s64-carry+0-null, 1.1e-06 to 1.8e-06 over the 771 and 4000 of the ragged and nrmonly cases, below 4e-07
# over the 5 and 10 of the others): float32 rounding of the angle (up to 2 pi) and of log and sincos, times s up to 6.7.  The bar is
# twice the largest.  The kernel under test measured the same figures, as it must where it is torch's stream bit for bit.  A misplaced
# element is off by 0.1 to 1: the bar must stay below draw_cases.BAR_CEILING = 1e-3, and a larger measured distance is a finding, not a
# constant to raise.
TORCH_DISTANCE = 2.643e-06
NORMAL_BAR = 2 * TORCH_DISTANCE          # 5.286e-06


@pytest.fixture(scope="module")
def cap(dev):
    """torch's calc_execution_policy, from the device's properties and not from the library under test."""
    p = torch.cuda.get_device_properties(dev)
    return p.multi_processor_count * (p.max_threads_per_multi_processor // 256)


@pytest.fixture(scope="module")
def contract(dev):
    """(flag to launch with, whether the kernel claims to be torch's stream under it)."""
    from pql_amd.utils import rng as R
    flag = R.verified(dev)
    return (1, False) if flag is None else (flag, True)


class Launch:
    """One pqlk_philox_draws call of a case into fresh guarded buffers."""

    def __init__(self, dev, c, flag, chunks=None, **over):
        from pql_amd import _lib as L
        c = c._replace(**over)
        chunks = c.chunks if chunks is None else chunks
        self.idx = Guarded(dev, (chunks, c.n_idx), dc.IDX_SENTINEL, dtype=torch.int64) if c.n_idx else None
        self.nrm = Guarded(dev, (chunks, c.n_normal), dc.NRM_SENTINEL) if c.n_normal else None
        self.step = Guarded(dev, (1,), dc.STEP_GUARD, init=torch.tensor([c.step], dtype=torch.int32), off=1, dtype=torch.int32) \
            if c.step is not None else None
        L.check(L.lib.pqlk_philox_draws(c.seed, c.base_offset, c.base_step, self.step.ptr if self.step else None, c.range,
                                        self.idx.ptr if self.idx else None, c.n_idx, self.nrm.ptr if self.nrm else None, c.n_normal,
                                        chunks, flag, L.stream(dev)))
        torch.cuda.synchronize()
        self.c, self.chunks = c, chunks

    def intact(self):
        return all(g.intact() for g in (self.idx, self.nrm, self.step) if g is not None) and \
            (self.step is None or int(self.step.t.item()) == self.c.step)

    def arrays(self):
        return (self.idx.t.cpu().numpy() if self.idx else np.zeros((self.chunks, 0), np.int64),
                self.nrm.t.cpu().numpy() if self.nrm else np.zeros((self.chunks, 0), np.float32))

    def same_bits(self, other, rows=slice(None), other_rows=slice(None)):
        return all(torch.equal(a.t[rows].view(torch.int32), b.t[other_rows].view(torch.int32))
                   for a, b in ((self.idx, other.idx), (self.nrm, other.nrm)) if a is not None)


def _torch_stream(dev, c, off0):
    """The calls the launch replaces: randint then normal_ per chunk on one device generator, a part of size 0 skipped."""
    g = torch.Generator(device=dev)
    g.manual_seed(c.seed)
    g.set_offset(off0)
    idx, nrm = [], []
    for _ in range(c.chunks):
        if c.n_idx:
            idx.append(torch.randint(c.range, (c.n_idx,), generator=g, device=dev))
        if c.n_normal:
            nrm.append(torch.empty(c.n_normal, device=dev).normal_(generator=g))
    return (torch.stack(idx) if idx else None), (torch.stack(nrm) if nrm else None), g.get_offset()


def test_bar_is_below_a_misplaced_element():
    assert 0.0 < TORCH_DISTANCE and NORMAL_BAR == 2 * TORCH_DISTANCE and NORMAL_BAR <= dc.BAR_CEILING == 1e-3


@pytest.mark.parametrize("name", dc.CASE_NAMES)
def test_draws_are_the_models(dev, cap, contract, name):
    c, flag = dc.case(name, cap), contract[0]
    want = dc.model(c, cap)
    a = Launch(dev, c, flag)
    got_idx, got_nrm = a.arrays()
    dc.check_indices(want, got_idx)
    d = dc.normal_distance(want, got_nrm)
    print(f"{name}: kernel's largest distance from the float64 model {d:.3e} over {got_nrm.size} normals, bar {NORMAL_BAR:.3e}")
    dc.check_normals(want, got_nrm, NORMAL_BAR)
    assert a.intact()
    # the same launch again: the same bits
    b = Launch(dev, c, flag)
    assert a.same_bits(b) and b.intact()
    # chunk k is chunk 0 of a launch of its own, k steps further on
    for k in range(c.chunks):
        one = Launch(dev, c, flag, chunks=1, base_offset=c.base_offset + k * want.inc_step)
        assert a.same_bits(one, rows=slice(k, k + 1)) and one.intact(), k
    # every step form is the NULL form at the offset it stands for, whatever base_step the NULL form is given
    for base_step in (0, 5):
        null = Launch(dev, c, flag, step=None, base_step=base_step, base_offset=want.off0)
        assert a.same_bits(null) and null.intact(), base_step


@pytest.mark.parametrize("name", dc.CASE_NAMES)
def test_draws_are_torchs_stream(dev, cap, contract, name):
    """ATen's kernels at the same elements: their normals against the same float64 model (the figure NORMAL_BAR is taken from), their
    indices against the model exactly, and -- where rng.verified approved the kernel -- the kernel's bits against theirs."""
    c, (flag, claimed) = dc.case(name, cap), contract
    want = dc.model(c, cap)
    t_idx, t_nrm, end = _torch_stream(dev, c, want.off0)
    assert end == want.off0 + c.chunks * want.inc_step
    if t_idx is not None:
        dc.check_indices(want, t_idx.cpu().numpy())
    if t_nrm is not None:
        d = dc.normal_distance(want, t_nrm.cpu().numpy())
        print(f"{name}: torch's largest distance from the float64 model {d:.3e} over {t_nrm.numel()} normals "
              f"(TORCH_DISTANCE {TORCH_DISTANCE:.3e}, bar {NORMAL_BAR:.3e})")
        assert d < dc.BAR_CEILING
    if claimed:
        a = Launch(dev, c, flag)
        assert t_idx is None or torch.equal(a.idx.t, t_idx)
        assert t_nrm is None or torch.equal(a.nrm.t.view(torch.int32), t_nrm.view(torch.int32))
        assert a.intact()


def test_verified_still_holds(dev):
    from pql_amd.utils import rng as R
    assert R.verified(dev) is not None, "pqlk_philox_draws does not reproduce torch.randint / normal_ on this device"


# =========================================================================== DrawAhead
B, A, DEPTH, SEED = 300, 3, 4, dc.SEED


def _ahead(dev, off0, normal=True):
    """A DrawAhead whose slot buffers are guarded and sentinel-filled, and a second generator for the torch calls."""
    from pql_amd.utils import rng as R
    flag = R.verified(dev)
    assert flag is not None
    g, ref = torch.Generator(device=dev), torch.Generator(device=dev)
    for x in (g, ref):
        x.manual_seed(SEED)
        x.set_offset(off0)
    ahead = R.DrawAhead(g, dev, B, (B, A) if normal else None, DEPTH, flag)
    gi = Guarded(dev, (DEPTH, B), dc.IDX_SENTINEL, dtype=torch.int64)
    gn = Guarded(dev, (DEPTH, B, A), dc.NRM_SENTINEL) if normal else None
    ahead.idx, ahead.normal = gi.t, (gn.t if normal else None)
    return ahead, g, ref, gi, gn


def _torch_step(dev, ref, rng_range, normal=True):
    i = torch.randint(rng_range, (B,), generator=ref, device=dev)
    return i, (torch.empty((B, A), device=dev).normal_(generator=ref) if normal else None)


@pytest.mark.parametrize("normal", [True, False], ids=["v", "p"])
def test_draw_ahead_partial_refill_writes_its_steps_only(dev, normal):
    steps = 2
    ahead, g, ref, gi, gn = _ahead(dev, dc.CARRY, normal)
    ahead.refill(977, steps)
    torch.cuda.synchronize()
    assert ahead.valid == steps and g.get_offset() == dc.CARRY           # drawing ahead does not move the generator
    for k in range(steps):
        i, n = _torch_step(dev, ref, 977, normal)
        assert torch.equal(gi.t[k], i) and (not normal or torch.equal(gn.t[k].view(torch.int32), n.view(torch.int32))), k
        assert ahead.take() == k
        assert g.get_offset() == ref.get_offset(), k                     # take() leaves the generator where the torch step does
    assert ahead.valid == 0
    assert bool((gi.t[steps:] == dc.IDX_SENTINEL).all()) and gi.intact()
    assert not normal or (bool((gn.t[steps:] == dc.NRM_SENTINEL).all()) and gn.intact())


def test_draw_ahead_continues_the_stream_after_invalidate(dev):
    """randint(cap1) + normal_ twice, then the bound changes: the refill with cap2 starts where those two torch steps ended."""
    cap1, cap2 = 977, dc.RANGE_PER
    ahead, g, ref, gi, gn = _ahead(dev, 4)
    ahead.refill(cap1)
    for k in range(2):
        i, n = _torch_step(dev, ref, cap1)
        assert torch.equal(gi.t[k], i) and torch.equal(gn.t[k].view(torch.int32), n.view(torch.int32))
        ahead.take()
    ahead.invalidate()
    assert ahead.valid == 0 and g.get_offset() == ref.get_offset()
    ahead.refill(cap2)
    torch.cuda.synchronize()
    assert ahead.valid == DEPTH
    for k in range(DEPTH):
        i, n = _torch_step(dev, ref, cap2)
        assert torch.equal(gi.t[k], i) and torch.equal(gn.t[k].view(torch.int32), n.view(torch.int32)), k
        assert ahead.take() == k
    assert g.get_offset() == ref.get_offset() == 4 + (2 + DEPTH) * ahead.inc and gi.intact() and gn.intact()
