"""The device sum tree of pql_amd/csrc/per.hip as the prioritized-replay tests drive it (tests/test_per_gpu.py,
tests/test_per_pql_gpu.py) and its NumPy model: the documented fp32 butterfly for the tree's sums.  Not collected as tests."""
import numpy as np
import torch

from support import T


def level_sizes(capacity):
    n = [capacity]
    while n[-1] > 64:
        n.append(-(-n[-1] // 64))
    return n


def butterfly64(x):
    """fp32 sums of rows of 64 in the order of per.hip's header: lane j pairs with j ^ 32, then ^ 16, ... ^ 1 (lane 0's value)."""
    v = np.asarray(x, dtype=np.float32).reshape(-1, 64)
    for o in (32, 16, 8, 4, 2, 1):
        v = v[:, :o] + v[:, o:2 * o]
    return v[:, 0]


def model_tree(leaves):
    """The whole flat buffer (every level padded to 64) that belongs to these leaves, by butterfly64."""
    out, cur = [], np.asarray(leaves, dtype=np.float32)
    for n in level_sizes(len(leaves)):
        pad = np.zeros(-(-n // 64) * 64, dtype=np.float32)
        pad[:n] = cur[:n]
        out.append(pad)
        cur = butterfly64(pad)
    return np.concatenate(out), np.float32(butterfly64(out[-1])[0])   # (buffer, total)


class Tree:
    def __init__(self, capacity, dev):
        from pql_amd import _lib as L
        self.L, self.dev, self.cap = L, dev, int(capacity)
        assert L.lib.pqlk_per_levels(self.cap) == len(level_sizes(self.cap))
        self.tree = torch.zeros(int(L.lib.pqlk_per_tree_floats(self.cap)), device=dev)
        self.pmax = torch.ones(1, device=dev)

    def update(self, idx, td, alpha=1.0, eps=0.0):
        L = self.L
        i, t = T(np.asarray(idx, dtype=np.int64)).to(self.dev), T(np.asarray(td, dtype=np.float32)).to(self.dev)
        L.check(L.lib.pqlk_per_update(L.ptr(self.tree), self.cap, L.ptr(self.pmax), L.ptr(i), L.ptr(t), i.shape[0], eps, alpha, L.stream(self.dev)))

    def insert(self, dst, m, alpha=1.0):
        L = self.L
        L.check(L.lib.pqlk_per_insert(L.ptr(self.tree), self.cap, L.ptr(self.pmax), dst, m, alpha, L.stream(self.dev)))

    def rebuild(self):
        L = self.L
        L.check(L.lib.pqlk_per_rebuild(L.ptr(self.tree), self.cap, L.stream(self.dev)))

    def sample(self, u):
        L = self.L
        ud = T(np.asarray(u, dtype=np.float32)).to(self.dev)
        idx = torch.full((ud.shape[0],), -7, dtype=torch.int64, device=self.dev)
        L.check(L.lib.pqlk_per_sample(L.ptr(self.tree), self.cap, L.ptr(ud), ud.shape[0], L.ptr(idx), L.stream(self.dev)))
        return idx.cpu().numpy()

    def weights(self, idx, n_valid, beta):
        L = self.L
        i = T(np.asarray(idx, dtype=np.int64)).to(self.dev)
        w, wmax = torch.full((i.shape[0],), -1.0, device=self.dev), torch.full((1,), 123.0, device=self.dev)
        L.check(L.lib.pqlk_per_weights(L.ptr(self.tree), self.cap, L.ptr(i), i.shape[0], n_valid, beta, L.ptr(w), L.ptr(wmax), L.stream(self.dev)))
        return w.cpu().numpy(), float(wmax.item())

    def leaves(self):
        return self.tree[: self.cap].cpu().numpy()

    def buffer(self):
        return self.tree.cpu().numpy()
