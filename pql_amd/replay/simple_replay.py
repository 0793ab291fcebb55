"""Replay ring buffer on HBM.

Drop-in for the reference's `pql/replay/simple_replay.py` (`create_buffer` :4-18, `ReplayBuffer` :21-104):
same constructor, `add_to_buffer(trajectory)`, `sample_batch(batch_size, device)`, public pointer
attributes `next_p / if_full / cur_capacity / capacity` and `buf_*` tensors.

MI355X design: the five SoA tensors of the reference become one array of fixed-stride, 128-byte
aligned records (layout in include/pqlk.h) so that a uniform random sample touches the minimum number
of HBM lines; `buf_obs`, `buf_action`, `buf_next_obs`, `buf_reward` are strided views into it and
`buf_done` a bool view computed on access.  Insert and gather are single HIP launches.

`reserve_space=True` (the reference's switch, simple_replay.py:9,15,91,94) or `obs_dtype=torch.float16` stores the two
observation fields as float16 -- 512 B per record instead of 896 B at obs 88 / act 16.  The reference parks those tensors on
the host because its GPU is small; here they stay in HBM.  Observations are rounded to nearest even once, at insert, and
widened exactly by every gather: the ring behaves bit for bit like an fp32 ring fed `x.to(float16).to(float32)`.  fp16 and
not bf16: it is the reference's dtype, and 8 significand bits are too coarse for raw, not yet normalised observations.
"""
from __future__ import annotations

import ctypes as C

import torch

from pql_amd import _lib as L


def _obs_width(obs_dim) -> int:
    if isinstance(obs_dim, int):
        return obs_dim
    if len(obs_dim) != 1:
        raise NotImplementedError("only flat observations are supported (the reference flattens them too)")
    return int(obs_dim[0])


_OBS_DTYPES = {"float32": torch.float32, "float16": torch.float16}


def parse_obs_dtype(value, key="obs_dtype") -> torch.dtype:
    """torch.float32 / torch.float16, or their names as the config writes them (`algo.replay_obs_dtype`)."""
    if isinstance(value, torch.dtype):
        dt = value if value in _OBS_DTYPES.values() else None
    else:
        dt = _OBS_DTYPES.get(str(value))
    if dt is None:
        raise ValueError(f"{key} must be float32 or float16, got {value!r}")
    return dt


def cfg_obs_dtype(algo) -> torch.dtype:
    """`algo.replay_obs_dtype` of a config node (absent: float32)."""
    value = algo.get("replay_obs_dtype") if hasattr(algo, "get") else getattr(algo, "replay_obs_dtype", None)
    return parse_obs_dtype("float32" if value is None else value, key="algo.replay_obs_dtype")


def ring_plan(next_p: int, if_full: bool, capacity: int, m: int):
    """Integer pointer law of simple_replay.py:52-83 -> ordered (dst_start, src_start, length) segments."""
    p = next_p + m
    segs = []
    if p > capacity:
        if_full = True
        head = capacity - next_p
        if head > 0:
            segs.append((next_p, 0, head))
        p -= capacity
        if p > capacity:
            raise RuntimeError(f"cannot insert {m} rows into a ring of capacity {capacity} at pointer {next_p}")
        segs.append((0, m - p, p))  # the LAST p rows wrap to the front (simple_replay.py:66)
    else:
        segs.append((next_p, 0, m))
    return segs, p, if_full, (capacity if if_full else p)


class RecordRing:
    """Device record array + descriptor shared by ReplayBuffer (A >= 0) and the P-learner obs ring (A = -1)."""

    def __init__(self, capacity: int, obs_dim: int, act_dim: int, device, obs_dtype=torch.float32):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise L.PqlkError(f"replay ring must live on a GPU (got {device}); pql_amd has no CPU path")
        self.capacity, self.O, self.A = int(capacity), int(obs_dim), int(act_dim)
        self.obs_dtype = parse_obs_dtype(obs_dtype)
        self.half = self.obs_dtype == torch.float16
        code = L.OBS_F16 if self.half else L.OBS_F32
        self.rec_ld = int(L.lib.pqlk_replay_rec_ld_ex(self.O, self.A, code))
        # raw 4-byte words whatever the observation format (an fp16 field packs two columns per word): checkpoints stream them as is
        self.records = torch.zeros((self.capacity, self.rec_ld), dtype=torch.float32, device=self.device)
        self.desc = L.PqlReplayDesc(self.records.data_ptr(), self.capacity, self.O, self.A, self.rec_ld, code)
        ow = ((self.O + 7) & ~7) // 2 if self.half else (self.O + 3) & ~3   # words of one observation field
        self.off_nobs, self.off_act = ow, 2 * ow   # (word offsets; meaningful for a transition ring)
        self.off_rd = 2 * ow + ((max(self.A, 0) + 3) & ~3)
        self.version = 0   # bumped by every insert: the learners' draws-ahead tiles are stamped with it (stale tiles are re-gathered)

    def obs_view(self, next_obs=False):
        """(capacity, O) strided view of the obs (or next_obs) field in its storage dtype."""
        off = self.off_nobs if next_obs else 0
        if self.half:
            return self.records.view(torch.float16)[:, 2 * off: 2 * off + self.O]
        return self.records[:, off: off + self.O]

    def rows(self, n):
        """Records [0, n) raw, pads included (a contiguous prefix of the record array): what a checkpoint streams."""
        return self.records[: int(n)]

    def training_state(self):
        return {"capacity": self.capacity, "O": self.O, "A": self.A, "rec_ld": self.rec_ld, "version": int(self.version),
                "obs_dtype": "float16" if self.half else "float32"}

    def load_training_state(self, st):
        """Header check + version.  The caller then writes `rows(cur_capacity)` straight into the record array, which no
        `Tensor._version` sees: the version moves past the saved one so that tiles gathered ahead are re-gathered."""
        have, saved = ("float16" if self.half else "float32"), str(st.get("obs_dtype", "float32"))   # (no key: written before fp16 rings)
        if have != saved:
            raise ValueError(f"replay ring: obs_dtype={have} but the checkpoint holds obs_dtype={saved}")
        for key in ("capacity", "O", "A", "rec_ld"):
            if int(st[key]) != getattr(self, key):
                raise ValueError(f"replay ring: {key}={getattr(self, key)} but the checkpoint holds {key}={int(st[key])}")
        self.version = int(st["version"]) + 1

    def insert_segments(self, segs, obs, act=None, rew=None, nobs=None, done=None):
        self.version += 1
        with torch.cuda.device(self.device):
            st = L.stream(self.device)
            for dst, src, n in segs:
                if n == 0:
                    continue
                L.check(L.lib.pqlk_replay_insert(
                    C.byref(self.desc), dst, n,
                    L.ptr(obs[src:]), obs.stride(0),
                    L.ptr(act[src:]) if act is not None else None, act.stride(0) if act is not None else 0,
                    L.ptr(rew[src:]) if rew is not None else None, rew.stride(0) if rew is not None else 0,
                    L.ptr(nobs[src:]) if nobs is not None else None, nobs.stride(0) if nobs is not None else 0,
                    L.ptr(done[src:]) if done is not None else None, done.stride(0) if done is not None else 0,
                    st))


def create_buffer(capacity, obs_dim, action_dim, device="cuda", reserve_space=False):
    """Reference-shaped allocator (simple_replay.py:4-18): returns (obs, action, next_obs, reward, done).
    Kept for callers that want plain SoA tensors; ReplayBuffer itself uses the record layout.
    reserve_space=True gives float16 obs / next_obs, as in the reference -- but on `device`: the reference puts the two tensors
    on the host to spare a small GPU's memory, a 288-GB card keeps them in HBM where the gather reads them."""
    cap = (capacity,) if isinstance(capacity, int) else tuple(capacity)
    O = _obs_width(obs_dim)
    f = dict(dtype=torch.float32, device=device)
    fo = dict(dtype=torch.float16 if reserve_space else torch.float32, device=device)
    return (torch.empty((*cap, O), **fo), torch.empty((*cap, int(action_dim)), **f), torch.empty((*cap, O), **fo),
            torch.empty((*cap, 1), **f), torch.empty((*cap, 1), dtype=torch.bool, device=device))


class ReplayBuffer:
    def __init__(self, capacity: int, obs_dim, action_dim: int, device="cuda", left_agent: bool = False,
                 reserve_space: bool = False, obs_dtype=None):
        if left_agent:
            raise NotImplementedError("left_agent belongs to the bimanual fork variants, out of scope")
        # reserve_space=True is the reference's name for float16 observation storage; obs_dtype= says the same thing directly
        obs_dtype = parse_obs_dtype(obs_dtype if obs_dtype is not None else (torch.float16 if reserve_space else torch.float32))
        if reserve_space and obs_dtype != torch.float16:
            raise ValueError(f"reserve_space=True means float16 observations, but obs_dtype={obs_dtype} was given")
        self.obs_dim = (obs_dim,) if isinstance(obs_dim, int) else tuple(obs_dim)
        self.action_dim = int(action_dim)
        self.device = torch.device(device)
        self.next_p = 0
        self.if_full = False
        self.cur_capacity = 0
        self.capacity = int(capacity)
        self.ring = RecordRing(self.capacity, _obs_width(obs_dim), self.action_dim, self.device, obs_dtype=obs_dtype)

    # ---- reference-named views -------------------------------------------------------------
    @property
    def records(self):
        return self.ring.records

    @property
    def buf_obs(self):
        return self.ring.obs_view()

    @property
    def buf_next_obs(self):
        return self.ring.obs_view(next_obs=True)

    @property
    def buf_action(self):
        return self.ring.records[:, self.ring.off_act: self.ring.off_act + self.ring.A]

    @property
    def buf_reward(self):
        return self.ring.records[:, self.ring.off_rd: self.ring.off_rd + 1]

    @property
    def buf_done(self):
        return self.ring.records[:, self.ring.off_rd + 1: self.ring.off_rd + 2] != 0

    def training_state(self):
        return {"ring": self.ring.training_state(), "next_p": int(self.next_p), "if_full": bool(self.if_full),
                "cur_capacity": int(self.cur_capacity)}

    def load_training_state(self, st):
        self.ring.load_training_state(st["ring"])
        self.next_p, self.if_full, self.cur_capacity = int(st["next_p"]), bool(st["if_full"]), int(st["cur_capacity"])

    def rows(self):
        return self.ring.rows(self.cur_capacity)

    # ---- a3 ---------------------------------------------------------------------------------
    @torch.no_grad()
    def add_to_buffer(self, trajectory):
        obs, actions, rewards, next_obs, dones = trajectory
        O, A = self.ring.O, self.ring.A
        f = dict(dtype=torch.float32, device=self.device)
        obs = obs.reshape(-1, O).to(**f).contiguous()
        actions = actions.reshape(-1, A).to(**f).contiguous()
        rewards = rewards.reshape(-1, 1).to(**f).contiguous()
        next_obs = next_obs.reshape(-1, O).to(**f).contiguous()
        dones = dones.reshape(-1, 1).to(**f).contiguous()
        segs, self.next_p, self.if_full, self.cur_capacity = ring_plan(self.next_p, self.if_full, self.capacity,
                                                                       rewards.shape[0])
        self.ring.insert_segments(segs, obs, actions, rewards, next_obs, dones)

    # ---- a4 ---------------------------------------------------------------------------------
    def draw_indices(self, batch_size, device=None):
        """The one RNG draw of sample_batch (simple_replay.py:87): same call, same shape/dtype/device."""
        return torch.randint(self.cur_capacity, size=(batch_size,), device=device or self.device)

    @torch.no_grad()
    def sample_batch(self, batch_size, device="cuda", indices=None):
        dev = self.device
        idx = self.draw_indices(batch_size) if indices is None else indices.to(device=dev, dtype=torch.int64).contiguous()
        B, O, A = idx.shape[0], self.ring.O, self.ring.A
        f = dict(dtype=torch.float32, device=dev)
        out = (torch.empty((B, O), **f), torch.empty((B, A), **f), torch.empty((B, 1), **f), torch.empty((B, O), **f),
               torch.empty((B, 1), **f))
        with torch.cuda.device(dev):
            L.check(L.lib.pqlk_replay_gather(C.byref(self.ring.desc), L.ptr(idx), B, *[L.ptr(t) for t in out],
                                             L.stream(dev)))
        tgt = torch.device(device)
        if tgt.type == "cuda" and tgt.index is None:
            tgt = dev
        return tuple(t.to(tgt) for t in out)
