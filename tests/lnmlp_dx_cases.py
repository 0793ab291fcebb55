"""Support of the `pqlk_lnmlp_dx` tests (no test in it): the case list and the float64 reference, torch autograd through a model built
from the critic's arena views like `_reference` of tests/test_lnmlp_kernels_gpu.py."""
import torch
import torch.nn.functional as F

# hidden layers, obs + act, m: one tile and one row past it; two layers on more than one block; ragged tiles per wave; the R = 2 edge
# (64-row image of 512 columns); R = 1 with VPL = 16
CASES = [([32], 3, 1), ([32], 3, 33), ([64, 32], 40, 65), ([160, 96], 104, 129), ([512, 512, 256], 104, 65), ([1024], 104, 33)]
# (col0, cols) of the tanh form per input width: inside one 32-column tile, and straddling two (an input of 3 has one tile)
WINDOWS = {3: [(1, 2)], 40: [(4, 16), (24, 16)], 104: [(40, 16), (88, 16)]}
FORMS = [(*c, w) for c in CASES for w in (None, *WINDOWS[c[1]])]


def q64(q, x, arena=None):
    """Twin Q (2, m) in float64 of critic `q` (parameters: its arena, or `arena`, a float64 tensor laid out like it) on x (m, in)."""
    from pql_amd.models.layernorm import LN_EPS
    p = (lambda t: t.double()) if arena is None else (lambda t: t)
    out, H = [], q.n_layers - 1
    for n in range(2):
        a = x
        for l in range(H):
            z = F.linear(a, p(q.weight(n, l, arena)), p(q.bias(n, l, arena)))
            a = F.elu(F.layer_norm(z, z.shape[1:], p(q.norm_param(n, l, "gamma", arena)), p(q.norm_param(n, l, "beta", arena)), LN_EPS))
        out.append(F.linear(a, p(q.weight(n, H, arena)), p(q.bias(n, H, arena)))[:, 0])
    return torch.stack(out)


def dx64(q, x, dq, arena=None):
    """d sum_n(dq_n . Q_n) / d x, (m, in) float64.  x (m, >= in) fp32, dq (2, m, 32) with the gradient in column 0."""
    x64 = x[:, :q.dims[0]].double().requires_grad_()
    with torch.enable_grad():
        (dq[:, :, 0].double() * q64(q, x64, arena)).sum().backward()
    return x64.grad
