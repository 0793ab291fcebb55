"""The one guarded device buffer of the GPU kernel tests: a tensor with poison in front of it and behind it, so that a write or a read
past its ends shows.  (tests/test_support_cpu.py holds its behaviour on CPU tensors.)"""
import ctypes as C

import numpy as np
import torch

from reduction_cases import SLACK
from support import T, bits  # noqa: F401


class Guarded:
    """A device tensor of `shape` with `fill` in SLACK elements behind it and in `off` elements in front (off = 1 also puts the
    tensor one float past a 16-byte boundary; off = SLACK keeps it 256-byte aligned).  The tensor starts as `init`, else filled with
    `body`, else as `fill`."""

    def __init__(self, dev, shape, fill, init=None, off=0, dtype=torch.float32, body=None):
        n = int(np.prod(shape))
        self.full = torch.full((off + n + SLACK,), fill, dtype=dtype, device=dev)
        self.t = self.full[off: off + n].view(*shape)
        self.n, self.off, self.fill = n, off, fill
        if init is not None:
            self.t.copy_(init if torch.is_tensor(init) else T(np.asarray(init)))
        elif body is not None:
            self.t.fill_(body)
        assert self.t.data_ptr() % 16 == (4 * off) % 16

    @property
    def ptr(self):
        return C.c_void_p(self.t.data_ptr())

    def intact(self):
        return bool((self.full[: self.off] == self.fill).all()) and bool((self.full[self.off + self.n:] == self.fill).all())

    def host(self):
        return self.t.cpu().numpy()
