"""The guarded buffers and the one-case job shared by the exact backward tests, tests/test_backward_paths_gpu.py and
tests/test_td_paths_gpu.py: every written buffer has SLACK floats of poison behind it, which must come back intact, and can start
as NaN; every read buffer has 1.0 in front of (tests/guarded.py's off=SLACK) and behind it, which would move a sum by a whole unit.
A HIP error ends the session: nothing more may be started on a device that has faulted."""
import ctypes as C

import pytest
import torch

import backward_cases as bc
from guarded import Guarded, T  # noqa: F401

POISON, SLACK, IN_ONE = bc.POISON, bc.SLACK, bc.IN_ONE
NAN = float("nan")


def _sync_or_stop(what):
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:      # a HIP error: nothing more may be started on this device
        pytest.exit(f"{what}: {e}", returncode=3)


def _returned(rcode, what):
    if rcode < 0:
        pytest.exit(f"{what}: HIP error {rcode}", returncode=3)
    return rcode


class _Job:
    """One case on the device: arena, stash, x, dy, tanh matrix; grads, dx, ws."""

    def __init__(self, dev, case, stash=None, dy=None):
        from pql_amd import _lib as L
        self.dev, self.case = dev, case
        self.desc = L.mlp_desc(case.dims, case.nets)
        self.want_grads, self.want_dx = case.form in ("gdx", "g"), case.form != "g"
        self.arena = Guarded(dev, (bc.net_stride(case.dims) * case.nets,), IN_ONE, bc.arena(case), off=SLACK)
        self.acts = Guarded(dev, (bc.acts_floats(case.dims, case.nets, case.B),), IN_ONE, bc.stash(case) if stash is None else stash, off=SLACK)
        self.x = Guarded(dev, (case.B, case.ldx), IN_ONE, bc.x_input(case), off=SLACK)
        self.dy = Guarded(dev, (case.nets, case.B, bc.ld(case.dims[-1])), IN_ONE, bc.dy_input(case) if dy is None else dy, off=SLACK)
        self.ld_dx, self.ld_tanh = bc.dx_geometry(case)
        self.tanh = None
        if case.form == "slice":
            self.tanh = Guarded(dev, (case.B, self.ld_tanh), IN_ONE, off=SLACK)
            self.tanh.t[:, : case.cols] = T(bc.tanh_input(case)).to(dev)
        self.inputs = [g for g in (self.arena, self.acts, self.x, self.dy, self.tanh) if g is not None]
        self.before = [g.full.clone() for g in self.inputs]
        self.ws_floats = int(L.lib.pqlk_mlp_bwd_ws_floats(C.byref(self.desc), case.B, case.splits))
        assert self.ws_floats == bc.bwd_ws_floats(case.dims, case.nets, case.B, case.splits)
        self.ws = Guarded(dev, (self.ws_floats,), POISON, body=NAN)
        self.fresh_outputs()

    def fresh_outputs(self):
        self.grads = Guarded(self.dev, (self.arena.n,), POISON, body=NAN) if self.want_grads else None
        self.dx = Guarded(self.dev, (self.case.B, self.ld_dx), POISON) if self.want_dx else None
        self.dx_before = self.dx.host() if self.want_dx else None

    def call(self, ws_floats=None, what=""):
        from pql_amd import _lib as L
        c = self.case
        rcode = L.lib.pqlk_mlp_backward(C.byref(self.desc), L.ptr(self.arena.t), L.ptr(self.x.t), c.ldx, c.B, L.ptr(self.acts.t), L.ptr(self.dy.t),
                                        L.ptr(self.grads.t) if self.want_grads else None, c.splits,
                                        L.ptr(self.dx.t) if self.want_dx else None, self.ld_dx if self.want_dx else 0, c.col0, c.cols,
                                        L.ptr(self.tanh.t) if self.tanh is not None else None, self.ld_tanh,
                                        L.ptr(self.ws.t), self.ws_floats if ws_floats is None else ws_floats, L.stream(self.dev))
        _returned(rcode, f"pqlk_mlp_backward on {c.name} {what}")
        _sync_or_stop(f"pqlk_mlp_backward on {c.name} {what}")
        return rcode

    def assert_guards(self, what):
        for g in (self.ws, self.grads, self.dx):
            assert g is None or g.intact(), f"{what}: slack behind a written buffer was written"
        for g, b in zip(self.inputs, self.before):
            same = (g.full == b) | (torch.isnan(g.full) & torch.isnan(b))
            assert bool(same.all()), f"{what}: an input buffer or its slack was written"

    def check(self, what):
        c = self.case
        grads = self.grads.host() if self.want_grads else None
        dx = self.dx.host() if self.want_dx else None
        if self.want_grads:
            bc.check_grads(grads, c, what=what)
        if c.form in ("gdx", "dx"):
            bc.check_dx_full(dx, self.dx_before, c, what=what)
        if c.form == "slice":
            bc.check_dx_slice(dx, self.dx_before, c, what=what)
        self.assert_guards(what)
        return grads, dx
