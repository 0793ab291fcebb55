"""What tests/c51_wide_cases.py guarantees, and the limits of the C51 entry points and of the Python layer, without a GPU."""
import ctypes as C

import numpy as np
import pytest
import torch

import c51_wide_cases as wc
import reduction_cases as rc

E_ALIGN, E_UNSUPPORTED = 4, 5
P = C.c_void_p(0x1000)      # stands in for a device pointer: argument validation never dereferences it


@pytest.fixture(scope="module")
def ref():
    from oracle import pql_ref_cpu
    return pql_ref_cpu


@pytest.mark.parametrize("K", wc.KS)
def test_two_level_target_logits_project_to_the_same_bits_under_any_softmax(ref, K):
    """torch's softmax and a strictly sequential fp32 one give the same pmf on the two-level logits, so two runs of the oracle's
    projection differ by exactly 0: kernel and oracle project the same numbers, and the 2e-7 bar is left to the projection."""
    lg, lt, rew, done, gn = wc.bce_inputs(wc.B_SMALL, K)
    assert bool(((lt == 0) | (lt == -200)).all()) and bool((lt == 0).any(-1).all())
    for net in range(2):
        a = torch.softmax(lt[net], 1)
        b = rc.T(wc.softmax_sequential(lt[net].numpy()))
        assert torch.equal(a, b)
        pa, pb = (ref.c51_project_ref(x, rew, done, gn, -10.0, 10.0, K) for x in (a, b))
        assert float((pa - pb).abs().max()) == 0.0


@pytest.mark.parametrize("K", wc.KS)
def test_terminal_rows_put_every_atom_into_one_bin(K):
    """10 of the 37 rows are terminal; in those one bin collects all K atoms as lower neighbour and one as upper neighbour: the
    longest range the kernels' walk can meet.  Every row meets the kernels' precondition: lo and up never decrease along a row."""
    _, _, rew, done, gn = wc.bce_inputs(wc.B_SMALL, K)
    term = done.view(-1).numpy() > 0
    assert int(term.sum()) == 10
    lo, up = wc.atom_bins(rew.numpy(), done.numpy(), gn, K)
    assert (wc.longest_run(lo)[term] == K).all() and (wc.longest_run(up)[term] == K).all()
    assert wc.longest_run(lo)[~term].max() < K
    assert (np.diff(lo, axis=1) >= 0).all() and (np.diff(up, axis=1) >= 0).all()
    assert lo.min() >= 0 and up.max() <= K - 1


@pytest.mark.parametrize("K", wc.KS)
def test_projection_rows_meet_the_precondition_and_keep_their_pattern(K):
    p, rew, done, gn, grid = wc.project_inputs(wc.PROJECT_B, K)
    assert p.shape == (wc.PROJECT_B, K)
    d = done.view(-1).numpy()
    i = np.arange(wc.PROJECT_B)
    assert np.array_equal(d > 0, i % 4 < 2) and np.array_equal(grid, i % 4 == 1)
    lo, up = wc.atom_bins(rew.numpy(), d, gn, K)
    assert (np.diff(lo, axis=1) >= 0).all() and (np.diff(up, axis=1) >= 0).all()
    r = rew.view(-1).numpy()
    assert (r[~(d > 0)] < -10).any() and (r[~(d > 0)] > 10).any()          # rewards past both ends
    # the on-atom rows: lo == up before the fix-up, i.e. the fix-ups are what separates them
    assert (up[grid] - lo[grid] == 1).all() and len(np.unique(up[grid][:, 0])) >= 8


def test_entry_points_take_up_to_256_atoms():
    """k = 65 passes the atom guard and reaches the alignment guard behind it (PQLK_E_ALIGN; it was PQLK_E_UNSUPPORTED while the
    limit was 64); k = 257 is PQLK_E_UNSUPPORTED.  Both come back before anything is launched."""
    from pql_amd import _lib as L
    lib = L.lib
    assert L.C51_MAX_ATOMS == wc.MAX_ATOMS == 256
    bce = lambda k, ld: lib.pqlk_c51_bce_loss(P, P, ld, k, P, P, P, 0.97, -10.0, 10.0, 4, P, P, None, 0, None, P, None)  # noqa: E731
    dpg = lambda k, ld: lib.pqlk_dpg_loss(P, ld, k, P, 4, P, P, None, 0, P, None)  # noqa: E731
    own = lambda k, ld: lib.pqlk_dpg_loss_owner(P, ld, k, P, 4, P, P, None, 0, P, None, None)  # noqa: E731
    prj = lambda k: lib.pqlk_c51_project(P, P, P, P, 0.97, -10.0, 10.0, k, 4, P, None)  # noqa: E731
    for f in (bce, dpg, own):
        assert f(65, 33) == E_ALIGN
        assert f(256, 255) == E_ALIGN and f(256, 224) == E_ALIGN        # ld % 32, ld < k
        assert f(257, 288) == E_UNSUPPORTED
    assert prj(257) == E_UNSUPPORTED


def test_num_atoms_is_checked_where_the_critic_is_built():
    from pql_amd.models.mlp import DistributionalDoubleQ
    for bad in (257, 1, 0, 1000):
        with pytest.raises(ValueError, match="256"):
            DistributionalDoubleQ(8, 2, num_atoms=bad, device="cpu", hidden_layers=[32, 32])
    q = DistributionalDoubleQ(8, 2, num_atoms=256, device="cpu", hidden_layers=[32, 32])
    assert q.num_atoms == 256 and q.layout.dims[-1] == 256 and q.layout.ld_out == 256 and q.z_atoms.shape == (256,)
    assert DistributionalDoubleQ(8, 2, num_atoms=2, device="cpu", hidden_layers=[32, 32]).layout.dims[-1] == 2


def test_make_critic_refuses_more_than_256_atoms_before_it_allocates():
    from pql_amd.algo.critics import make_critic
    from pql_amd.utils.cfg import load_cfg
    cfg = load_cfg(["algo.distl=True", "algo.num_atoms=257"])
    with pytest.raises(ValueError, match="256"):
        make_critic(cfg, 8, 2, torch.device("cpu"))
