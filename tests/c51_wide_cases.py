"""Inputs and shapes for the C51 kernels with 65 ... 256 atoms (tests/test_c51_wide_gpu.py; what they guarantee is proved without
a GPU in tests/test_c51_wide_cpu.py).  Plain numpy / torch, no GPU.  References: reduction_cases.c51_reference /
dpg_dist_reference and the oracle's c51_project_ref, which take K as a parameter."""
import numpy as np
import torch

import detdata as dd
import reduction_cases as rc

F32 = np.float32
T = rc.T

MAX_ATOMS = 256                                           # PQLK_C51_MAX_ATOMS (include/pqlk.h)
# (K, ld): one atom past a wave; a ragged last group; pad columns past the last group (160 > 128); every lane of every group
SHAPES = [(65, 96), (101, 128), (101, 160), (128, 128), (129, 160), (255, 256), (256, 256)]
KS = sorted({K for K, _ in SHAPES})
B_SMALL = 37
RC_PROJECT_KS = (65, 101, 128)                            # reduction_cases.project_inputs works as it is for these
PROJECT_B = 263


def two_level_logits(B, K):
    """0 on a random half of the atoms, -200 elsewhere, at least one 0 per row: exp(-200) is 0 in fp32, so the pmf is exactly
    1 / count on its support in ANY fp32 softmax (the construction reduction_cases.c51_inputs uses past its grid cap)."""
    keep = dd.bernoulli((2, B, K), 97 + K, 0.5)
    keep[:, np.arange(B), np.arange(B) % K] = 1.0
    return T(np.where(keep > 0, 0.0, -200.0).astype(F32))


def bce_inputs(B, K, saturated=False):
    """reduction_cases.c51_inputs with two-level target logits at every B.  With its U(-3, 3) target logits two fp32 softmaxes put
    1.8e-7 ... 4.8e-7 between two runs of the ORACLE's projection at these K (a terminal row sums the whole pmf into one bin), which
    is above the 2e-7 bar of the comparison; with two-level logits the difference is exactly 0 (test_c51_wide_cpu.py)."""
    lg, _, rew, done, gn = rc.c51_inputs(B, K, saturated=saturated)
    return lg, two_level_logits(B, K), rew, done, gn


def project_inputs(B, K, v_min=-10.0, v_max=10.0):
    """The rows of reduction_cases.project_inputs: i % 4 == 0 terminal with a random reward, i % 4 == 1 terminal with the reward ON
    an atom (lo == up before the fix-up), others non-terminal with rewards past both ends.  For K in RC_PROJECT_KS that function
    itself; for the others the same construction without its assertion that the LAST atom is among those an fp32 reward can hit
    exactly: at K = 256 the fp32 position (v_max - v_min) / dz is not 255 (187 atoms can be hit, 254 the highest)."""
    if K in RC_PROJECT_KS:
        return rc.project_inputs(B=B, K=K, v_min=v_min, v_max=v_max)
    p = torch.softmax(T(dd.uniform((B, K), 71, -3, 3)), 1)
    rew = (0.7 * (v_max - v_min) * dd.uniform((B,), 72, -1, 1)).astype(F32)
    done = np.zeros(B, dtype=F32)
    dz = F32((float(v_max) - float(v_min)) / (K - 1))
    on_atom = []
    for j in range(K):
        r = F32(v_min) + F32(j) * dz
        for _ in range(8):
            b = (r - F32(v_min)) / dz
            if b == F32(j):
                break
            r = np.nextafter(r, F32(np.inf) if b < j else F32(-np.inf), dtype=F32)
        if (r - F32(v_min)) / dz == F32(j):
            on_atom.append(r)
    on_atom = np.array(on_atom, dtype=F32)
    assert len(on_atom) >= K // 4 and on_atom[0] == F32(v_min)
    i = np.arange(B)
    done[i % 4 == 0] = 1.0
    grid = i % 4 == 1
    done[grid] = 1.0
    rew[grid] = on_atom[(i[grid] // 4) % len(on_atom)]
    return p, T(rew).view(-1, 1), T(done).view(-1, 1), float(F32(0.99 ** 3)), grid


def atom_bins(rew, done, gn, K, v_min=-10.0, v_max=10.0):
    """(lo, up), each (B, K) int64: the two bins every atom deposits into, by the fp32 expressions of include/pqlk.h's projection
    law (the support is torch.linspace's, as the kernels get it)."""
    z = torch.linspace(v_min, v_max, K).numpy()
    r, d = np.asarray(rew, dtype=F32).reshape(-1, 1), np.asarray(done, dtype=F32).reshape(-1, 1)
    dz = F32((float(v_max) - float(v_min)) / (K - 1))
    tz = r + ((F32(1) - d) * F32(gn)) * z[None, :]
    tz = np.minimum(np.maximum(tz, F32(v_min)), F32(v_max))
    bpos = (tz - F32(v_min)) / dz
    assert bpos.dtype == F32
    lo, up = np.floor(bpos).astype(np.int64), np.ceil(bpos).astype(np.int64)
    lo = np.where((up > 0) & (lo == up), lo - 1, lo)
    up = np.where((lo < K - 1) & (lo == up), up + 1, up)
    return lo, up


def longest_run(bins):
    """Longest run of equal neighbours in every row of a (B, K) integer array -> (B,)."""
    out = np.ones(bins.shape[0], dtype=np.int64)
    run = np.ones(bins.shape[0], dtype=np.int64)
    for k in range(1, bins.shape[1]):
        run = np.where(bins[:, k] == bins[:, k - 1], run + 1, 1)
        out = np.maximum(out, run)
    return out


def softmax_sequential(x):
    """fp32 softmax over the last axis with the sum taken strictly left to right (np.cumsum): another fp32 softmax than torch's."""
    x = np.asarray(x, dtype=F32)
    e = np.exp(x - x.max(-1, keepdims=True), dtype=F32)
    return (e / np.cumsum(e, axis=-1, dtype=F32)[..., -1:]).astype(F32)
