"""Support of the `pqlk_lnmlp_grad_chain` tests (no test in it): the case list, the float64 parameter gradient (torch autograd through
`q64` of lnmlp_dx_cases.py) and the per-group error against it."""
import torch

from lnmlp_dx_cases import CASES, q64

# lnmlp_dx_cases.py's shapes, and 549 rows = 18 tiles, which spread unevenly over the fold's 16 groups (2 tiles each in 9 groups, 7 empty)
GRAD_CASES = [*CASES, ([32], 3, 549)]
GROUPS = ("W", "b", "gamma", "beta")


def grads64(q, x, dq, arena=None):
    """d sum_n(dq_n . Q_n) / d parameters, float64, laid out like the arena of critic `q` (parameters: `arena` fp32, or its own)."""
    a64 = (q.arena.data if arena is None else arena).double().requires_grad_()
    with torch.enable_grad():
        (dq[:, :, 0].double() * q64(q, x[:, :q.dims[0]].double(), a64)).sum().backward()
    return a64.grad


def group_errors(q, got, ref):
    """{W / b / gamma / beta: max abs error of the fp32 gradient `got` against `ref`} over every net and layer."""
    e = dict.fromkeys(GROUPS, 0.0)
    for (key, g), (_, r) in zip(q.named_views(got), q.named_views(ref)):
        layer, kind = key.split(".")[-2:]
        group = ("W" if kind == "weight" else "b") if int(layer) % 3 == 0 else ("gamma" if kind == "weight" else "beta")
        e[group] = max(e[group], float((g.double() - r).abs().max()))
    return e
