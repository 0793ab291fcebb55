"""Inputs, references and the shape table for tests/test_layernorm_kernels_gpu.py (plain numpy / torch, no GPU);
tests/test_layernorm_cases_cpu.py proves what they guarantee.

The law under test is written op by op in include/pqlk.h (LayerNorm + ELU section): fp32, one rounding per written operation.
Two kinds of input:

  generic  uniform rows with both ELU branches in play, checked against float64 `F.elu(F.layer_norm(...))` and its autograd at the
           bars of the BatchNorm pair's tests;
  exact    each row a permutation of a multiset of integers in [-2, 2] that sums to 0, gamma in {1/4, 1/2, 3/4, 1}, beta = 20 (so
           every y > 0).  Then every partial sum of a row is a small integer (exact in fp32 in ANY order), mean = 0 exactly,
           sum z^2 is an integer, and everything after it is a chain of single roundings: the op-by-op numpy model below gives
           the kernel's bits, whatever the summation tree.
"""
import functools
import os
import re

import numpy as np
import torch
import torch.nn.functional as F

import detdata as dd
from support import T  # noqa: F401  (re-exported)

F32 = np.float32
EPS = 1e-5
POISON, SLACK = 5.0, 64          # as tests/reduction_cases.py

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_constant(name):
    text = open(os.path.join(ROOT, "include", "pqlk.h")).read()
    return int(re.search(rf"#define\s+{name}\s+(\d+)", text).group(1))


# ---------------------------------------------------------------- dispatch seams and caps (include/pqlk.h, pql_amd/csrc/ln.hip)
ROWS_PER_BLOCK = 4                       # one wave per row, 256 threads
REG_SEAMS = [128, 256, 512, 1024]        # widest row of the 2 / 4 / 8 / 16 registers-per-lane kernels; wider: the strided path
ROW_BLOCKS = 4096                        # PQLK_LN_ROW_BLOCKS: forward, backward without parameter gradients
CHUNKS = 512                             # PQLK_LN_CHUNKS: backward with parameter gradients
FOLD_GROUPS = 16                         # the fold launch's groups of consecutive chunks

COLS = [1, 2, 33, 64, 65, 128, 129, 130, 256, 257, 512, 513, 1024, 1025]
M_SMALL = [1, 3, 5, 257]
M_PAST_CHUNKS = ROWS_PER_BLOCK * CHUNKS + 1          # a wave of the column-sum backward takes a second row
M_PAST_ROW_BLOCKS = ROWS_PER_BLOCK * ROW_BLOCKS + 1  # a wave of the forward takes a second row
# (m, cols): every width at every small m; past each cap at a scalar-tail width, a ragged vector width and (the chunked column
# sums of the strided path, whose chunk count is min(m, CHUNKS)) the wide path
SHAPES = [(m, c) for c in COLS for m in M_SMALL] + [(M_PAST_CHUNKS, 33), (M_PAST_CHUNKS, 130), (M_PAST_CHUNKS, 1025),
                                                   (M_PAST_ROW_BLOCKS, 33), (M_PAST_ROW_BLOCKS, 130)]
ALIGN = ["scalar", "vector"]             # ld = cols + 3, one float past a 16-byte boundary | ld = pqlk_ld(cols), 16-byte aligned
EXACT_COLS = [64, 130, 1026]
EXACT_COLS_TORCH = [2, 64, 130, 1000, 1026]

Y_BAR = dict(rtol=1e-5, atol=5e-6)       # test_bn_elu_forward_shapes
STAT_RTOL, MEAN_ATOL = 1e-5, 1e-6
BWD_RTOL, BWD_ATOL_REL = 2e-5, 2e-5      # _bn_backward: atol = 2e-5 * max|ref|


def shape_id(s):
    return f"m{s[0]}-c{s[1]}"


# ---------------------------------------------------------------- generic inputs and the float64 reference
def generic_inputs(m, cols, seed=0):
    """z with a per-row offset and scale (so mean and rstd differ from row to row), gamma around 1, beta around 0: xhat * gamma +
    beta takes both signs, both ELU branches run.
    cols == 2 is scaled down to |z0 - z1| ~ sqrt(eps): with two columns xhat = +-1 whatever z is, and dz is eps / (var + eps) of the
    terms it is the difference of.  At |z0 - z1| ~ 1 that is 1e-5 of what fp32 resolves, for any implementation (torch's own fp32
    CPU autograd then misses the backward bar 3870-fold); at sqrt(eps) the gradient is O(1) of its terms and eps takes part."""
    s = 1000 * seed + 7 * m + 13 * cols
    z = dd.uniform((m, cols), s + 1, -2, 2) * dd.uniform((m, 1), s + 2, 0.5, 3.0) + dd.uniform((m, 1), s + 3, -1, 1)
    if cols == 2:
        z = z * F32(0.004)
    gamma, beta = dd.uniform((cols,), s + 4, 0.5, 1.5), dd.uniform((cols,), s + 5, -0.5, 0.5)
    dy = dd.uniform((m, cols), s + 6, -1, 1)
    return z.astype(F32), gamma, beta, dy


def torch_reference(z, gamma, beta, dy, dtype=torch.float64):
    """y, mean, rstd, dz, dgamma, dbeta of `F.elu(F.layer_norm(z, (cols,), gamma, beta, EPS))` and its autograd in `dtype`."""
    zt = torch.tensor(z, dtype=dtype, requires_grad=True)
    g, b = torch.tensor(gamma, dtype=dtype, requires_grad=True), torch.tensor(beta, dtype=dtype, requires_grad=True)
    y = F.elu(F.layer_norm(zt, (z.shape[1],), g, b, EPS))
    dz, dg, db = torch.autograd.grad(y, [zt, g, b], torch.tensor(dy, dtype=dtype))
    with torch.no_grad():
        mean = zt.mean(1)
        rstd = 1.0 / torch.sqrt(zt.var(1, unbiased=False) + EPS)
    return dict(y=y.detach().numpy(), mean=mean.numpy(), rstd=rstd.numpy(), dz=dz.numpy(), dgamma=dg.numpy(), dbeta=db.numpy())


@functools.lru_cache(maxsize=None)
def generic_case(m, cols):
    """(inputs, float64 reference) of one shape: computed once, shared by the tests, never written to."""
    inp = generic_inputs(m, cols)
    ref = torch_reference(*inp)
    for a in (*inp, *ref.values()):
        a.setflags(write=False)
    return inp, ref


def bwd_atol(ref):
    return BWD_ATOL_REL * float(np.abs(ref).max())


# ---------------------------------------------------------------- the exact design and the op-by-op model of the law
def zero_sum_multiset(cols):
    """cols integers in [-2, 2] with sum 0: pairs (k, -k), k = 1, 2, 1, 2, ..., and one 0 when cols is odd."""
    v = []
    for i in range(cols // 2):
        k = 1 + (i % 2)
        v += [k, -k]
    return np.array(v + [0] * (cols % 2), dtype=F32)


def exact_inputs(m, cols, seed=1):
    """seed picks the rows' permutations.  The kernel and the model do not care; torch's CPU moments do: they come from a cascaded
    Welford update, which on some permutations (seeds 0, 2, 3 at cols 130) leaves the variance one ulp off the integer ratio.  The
    default is a set of permutations on which torch, too, computes the law exactly at every width the CPU test compares."""
    base = zero_sum_multiset(cols)
    z = np.stack([base[np.random.RandomState(1000 * seed + r).permutation(cols)] for r in range(m)])
    gamma = (F32(0.25) * (1 + dd.integers((cols,), 77 + seed, 4))).astype(F32)
    beta = np.full((cols,), 20.0, F32)
    return z.astype(F32), gamma, beta


def _sum32(v, order):
    """fp32 running sum of v in `order` (None: index order; "exact": the float64 sum rounded once -- on the exact design, where every
    order gives the same bits (tests/test_layernorm_cases_cpu.py), that is the running sum too, and it is fast at many rows)."""
    if isinstance(order, str):
        return F32(np.asarray(v, np.float64).sum())
    s = F32(0.0)
    for x in (v if order is None else v[order]):
        s = F32(s + x)
    return s


def model_forward(z, gamma, beta, eps=EPS, order=None):
    """The law, op by op in fp32 (one rounding per written operation), the two row sums taken as running sums in `order`.
    Returns y, mean, rstd."""
    z = np.asarray(z, F32)
    m, n = z.shape
    y, mean, rstd = np.empty_like(z), np.empty(m, F32), np.empty(m, F32)
    nf, e = F32(n), F32(eps)
    for r in range(m):
        mu = F32(_sum32(z[r], order) / nf)
        d = (z[r] - mu).astype(F32)
        var = F32(_sum32((d * d).astype(F32), order) / nf)
        rs = F32(F32(1.0) / np.sqrt(F32(var + e)))
        pre = ((d * rs).astype(F32) * gamma).astype(F32) + beta
        pre = pre.astype(F32)
        y[r] = np.where(pre > 0, pre, np.expm1(pre)).astype(F32)
        mean[r], rstd[r] = mu, rs
    return y, mean, rstd


def near_constant_rows():
    """4 x 512 rows of 1000 + 0.01 U(-1, 1): the variance is 1e-10 of the squared mean."""
    z = (1000.0 + 0.01 * dd.uniform((4, 512), 4242, -1, 1).astype(np.float64)).astype(F32)
    return z, np.ones(512, F32), np.zeros(512, F32)
