"""Inputs, references and the torch twin for the residual LayerNorm critic's tests (tests/test_bronet_kernels_gpu.py,
tests/test_bronet_agents_gpu.py, tests/test_bronet_cpu.py); plain numpy / torch, no GPU.  tests/test_bronet_cases_cpu.py proves what
they guarantee.

The laws under test are written op by op in include/pqlk.h (pqlk_ln_res_forward / pqlk_ln_sum_backward).  Everything that is not
new comes from tests/layernorm_cases.py: the shape table, the bars, the generic inputs (z, gamma, beta, dy) and the exact design.
Added here:

  res, dy2   the skip of the forward and the second addend of the backward, per shape, from detdata;
  float64    `res + F.layer_norm(z)` with mean / rstd, and the backward of LayerNorm (with ELU and without) whose incoming gradient is
             dy + dy2: dsum, dz, dgamma, dbeta by autograd;
  model      the op-by-op fp32 model of the forward without the activation, extended by the ONE new addition y = res + t.  On the
             exact design (layernorm_cases) its t is layernorm_cases.model_forward's y bit for bit (beta = 20: every pre-activation
             is > 0 and ELU is the identity there), and a dyadic res (multiples of 1/4 in [-2, 2]) leaves one rounding, whatever the
             summation tree;
  Twin       the `nn.Module` whose state_dict keys are DoubleQBroNet's: the float64 reference of the critic.
"""
import functools

import numpy as np
import torch
import torch.nn.functional as F
from torch import nn

import detdata as dd
import layernorm_cases as lc

F32 = np.float32
T = lc.T
EPS = lc.EPS
SHAPES, ALIGN, EXACT_COLS = lc.SHAPES, lc.ALIGN, lc.EXACT_COLS
M_PAST_CHUNKS, M_PAST_ROW_BLOCKS = lc.M_PAST_CHUNKS, lc.M_PAST_ROW_BLOCKS
Y_BAR, STAT_RTOL, MEAN_ATOL, BWD_RTOL, bwd_atol = lc.Y_BAR, lc.STAT_RTOL, lc.MEAN_ATOL, lc.BWD_RTOL, lc.bwd_atol
shape_id = lc.shape_id


# ---------------------------------------------------------------- generic inputs and the float64 references
def extra_inputs(m, cols, seed=0):
    """res (the skip: the size of an activation) and dy2 (the second addend: the size of dy) of one shape."""
    s = 1000 * seed + 7 * m + 13 * cols
    return dd.uniform((m, cols), s + 8, -2, 2), dd.uniform((m, cols), s + 9, -1, 1)


def res_reference(z, gamma, beta, res, dtype=torch.float64):
    """y, mean, rstd of `res + F.layer_norm(z, (cols,), gamma, beta, EPS)` in `dtype`."""
    zt = torch.tensor(z, dtype=dtype)
    y = torch.tensor(res, dtype=dtype) + F.layer_norm(zt, (z.shape[1],), torch.tensor(gamma, dtype=dtype), torch.tensor(beta, dtype=dtype), EPS)
    rstd = 1.0 / torch.sqrt(zt.var(1, unbiased=False) + EPS)
    return dict(y=y.numpy(), mean=zt.mean(1).numpy(), rstd=rstd.numpy())


def sum_reference(z, gamma, beta, dy, dy2, elu, dtype=torch.float64):
    """dsum, dz, dgamma, dbeta: autograd of LayerNorm (followed by ELU if `elu`) in `dtype` with the incoming gradient dy + dy2."""
    zt = torch.tensor(z, dtype=dtype, requires_grad=True)
    g, b = torch.tensor(gamma, dtype=dtype, requires_grad=True), torch.tensor(beta, dtype=dtype, requires_grad=True)
    y = F.layer_norm(zt, (z.shape[1],), g, b, EPS)
    if elu:
        y = F.elu(y)
    dsum = torch.tensor(dy, dtype=dtype) + torch.tensor(dy2, dtype=dtype)
    dz, dg, db = torch.autograd.grad(y, [zt, g, b], dsum)
    return dict(dsum=dsum.numpy(), dz=dz.numpy(), dgamma=dg.numpy(), dbeta=db.numpy())


@functools.lru_cache(maxsize=None)
def generic_case(m, cols):
    """((z, gamma, beta, dy, res, dy2), forward float64 reference, no-activation backward float64 reference (None at cols == 1, where
    dz is a difference of equal terms)) of one shape: computed once, shared by the tests, never written to."""
    (z, gamma, beta, dy), _ = lc.generic_case(m, cols)
    res, dy2 = extra_inputs(m, cols)
    fwd = res_reference(z, gamma, beta, res)
    bwd = sum_reference(z, gamma, beta, dy, dy2, elu=False) if cols >= 2 else None
    for a in (res, dy2, *fwd.values(), *(bwd or {}).values()):
        a.setflags(write=False)
    return (z, gamma, beta, dy, res, dy2), fwd, bwd


# ---------------------------------------------------------------- the op-by-op model and the exact design
def model_res_forward(z, gamma, beta, res, eps=EPS, order=None):
    """pqlk_ln_res_forward's law, op by op in fp32 (one rounding per written operation), the two row sums as running sums in `order`
    (layernorm_cases._sum32).  Returns y, mean, rstd."""
    z = np.asarray(z, F32)
    m, n = z.shape
    y, mean, rstd = np.empty_like(z), np.empty(m, F32), np.empty(m, F32)
    nf, e = F32(n), F32(eps)
    for r in range(m):
        mu = F32(lc._sum32(z[r], order) / nf)
        d = (z[r] - mu).astype(F32)
        var = F32(lc._sum32((d * d).astype(F32), order) / nf)
        rs = F32(F32(1.0) / np.sqrt(F32(var + e)))
        t = ((d * rs).astype(F32) * gamma).astype(F32)
        t = (t + beta).astype(F32)
        y[r] = (np.asarray(res[r], F32) + t).astype(F32)     # the one new addition
        mean[r], rstd[r] = mu, rs
    return y, mean, rstd


def exact_res(m, cols, seed=3):
    """Dyadic skip values: multiples of 1/4 in [-2, 2]."""
    return ((dd.integers((m, cols), 500 + seed, 17) - 8).astype(F32) * F32(0.25)).astype(F32)


def exact_grads(m, cols, seed=4):
    """Integer dy and dy2 in [-3, 3]: dy + dy2 is exact, and so are its column sums."""
    return (dd.integers((m, cols), 600 + seed, 7) - 3).astype(F32), (dd.integers((m, cols), 700 + seed, 7) - 3).astype(F32)


# ---------------------------------------------------------------- the torch twin of DoubleQBroNet
class TwinNet(nn.Module):
    def __init__(self, in_dim, width, blocks):
        super().__init__()
        self.stem = nn.Sequential(nn.Linear(in_dim, width), nn.LayerNorm(width, eps=EPS), nn.ELU())
        self.blocks = nn.ModuleList(nn.Sequential(nn.Linear(width, width), nn.LayerNorm(width, eps=EPS), nn.ELU(), nn.Linear(width, width),
                                                  nn.LayerNorm(width, eps=EPS)) for _ in range(blocks))
        self.out = nn.Linear(width, 1)

    def forward(self, x):
        h = self.stem(x)
        for blk in self.blocks:
            h = h + blk(h)
        return self.out(h)


class Twin(nn.Module):
    """Keys: net_q{1,2}.stem.{0,1}.*, net_q{1,2}.blocks.{k}.{0,1,3,4}.*, net_q{1,2}.out.*"""

    def __init__(self, in_dim, width, blocks):
        super().__init__()
        self.net_q1, self.net_q2 = TwinNet(in_dim, width, blocks), TwinNet(in_dim, width, blocks)

    def forward(self, x):
        return self.net_q1(x), self.net_q2(x)


def num_params(in_dim, width, blocks):
    """Trainable scalars of the twin critic: per net the stem Linear + norm, two Linear + norm per block, the output Linear."""
    per_net = (in_dim * width + width) + 2 * width + blocks * 2 * (width * width + width + 2 * width) + (width + 1)
    return 2 * per_net


def twin_state(in_dim, width, blocks, seed):
    """A deterministic state for the twin (and, by its keys, for DoubleQBroNet): Linears at the nn.Linear scale, non-trivial norms."""
    twin = Twin(in_dim, width, blocks)
    st = {}
    for i, (k, v) in enumerate(twin.state_dict().items()):
        shape = tuple(v.shape)
        is_norm = isinstance(dict(twin.named_modules())[k.rsplit(".", 1)[0]], nn.LayerNorm)
        if is_norm:
            a = dd.uniform(shape, seed + 31 * i, 0.5, 1.5) if k.endswith("weight") else dd.uniform(shape, seed + 31 * i, -0.5, 0.5)
        else:
            fan_in = shape[1] if len(shape) == 2 else dict(twin.named_modules())[k.rsplit(".", 1)[0]].in_features
            bound = 1.0 / np.sqrt(fan_in)
            a = dd.uniform(shape, seed + 31 * i, -bound, bound)
        st[k] = T(a.astype(F32))
    return st
