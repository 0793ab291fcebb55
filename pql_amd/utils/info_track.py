"""`info_track_keys` / `info_track_step` on the device: moving windows over values the env reports in its info dict.

Reference: pql/algo/pql_actor.py:28-33,138-151, pql/algo/ac_base.py:54-59,88-101,116-119, pql/utils/evaluator.py:56-61,89-111.  There
every key costs a `torch.where(done)[0]`, a `.cpu()` and a `deque.extend` per env step.  Here `InfoTrackers` (one instance in
`PQLActor` -- and so in DDPG, SAC, CrossQ --, one in `AgentPPO`, one per evaluation) keeps per key a `DeviceTracker` window and,
for `all-episode`, an (N,) fp32 accumulator, and `update(done, info)` is stream work only:

    last          append info[key][done] in env order
    all-episode   acc += info[key]; append acc[done]; acc[done] = 0         (`all` is the reference `PQLActor`'s spelling of it)
    all-step      append all N values

"append" is `DeviceTracker.update`: when one step brings more values than the window holds, only the last `window_len` stay.  A key
absent from this step's info is skipped for this step (ac_base.py:91-92, evaluator.py:92-93); bool / uint8 values count as 0.0 /
1.0.  `info_track_step[i]` belongs to `info_track_keys[i]`; a key may be listed more than once (with different modes), each entry
has its own window, and `means()` then reports the last entry of that name.

The torch form below (`_update_torch`) is the definition and the CPU path.  On a GPU, entries whose values are contiguous float32 or
bool / uint8 -- with a bool `done` -- go through `pqlk_rollout_info` (pql_amd/csrc/rollout.hip): ONE launch for up to 8 entries, one
block per entry, bit-equal to the torch form.

Unlike the reference, an unknown mode, a length mismatch or (where the env declares `info_keys`) a key the env never reports is a
`ValueError` at construction: the reference ignores an unknown mode silently and logs zeros.
"""
from __future__ import annotations

import torch

from pql_amd import _lib as L

LAST, ALL_EPISODE, ALL_STEP = L.INFO_LAST, L.INFO_ALL_EPISODE, L.INFO_ALL_STEP   # PqlInfoKey.mode (include/pqlk.h)
MODES = {"last": LAST, "all-episode": ALL_EPISODE, "all": ALL_EPISODE, "all-step": ALL_STEP}
ALWAYS_OFFERED = ("TimeLimit.truncated",)   # every env of this project reports it


def _as_list(x):
    if x is None:
        return []
    return [x] if isinstance(x, str) else list(x)


class InfoTrackers:
    def __init__(self, keys, steps, num_envs, window_len, device, offered=None):
        """keys / steps: `cfg.info_track_keys` / `cfg.info_track_step` (None, a string or a list).  offered: the env's `info_keys`
        when it declares them (None: any key is accepted and one the env never reports just stays at zero)."""
        from pql_amd.algo.pql_actor import DeviceTracker
        self.keys, modes = _as_list(keys), _as_list(steps)
        if not self.keys and modes:
            raise ValueError(f"info_track_step={steps!r} is set but info_track_keys is not: there is nothing to track")
        if len(self.keys) != len(modes):
            raise ValueError(f"info_track_keys={self.keys!r} has {len(self.keys)} entries but info_track_step={modes!r} has {len(modes)}: "
                             f"info_track_step[i] belongs to info_track_keys[i]")
        for key, mode in zip(self.keys, modes):
            if mode not in MODES:
                raise ValueError(f"info_track_step={mode!r} for info_track_keys entry {key!r}: no such mode; known modes: {', '.join(MODES)}")
        if offered is not None:
            known = (*offered, *ALWAYS_OFFERED)
            for key in self.keys:
                if key not in known:
                    raise ValueError(f"info_track_keys entry {key!r}: the env reports no such value; it offers: {', '.join(known)}")
        self.spellings = modes
        self.modes = [MODES[m] for m in modes]
        self.num_envs, self.window_len, self.device = int(num_envs), int(window_len), torch.device(device)
        self.trackers = [DeviceTracker(self.window_len, self.device) for _ in self.keys]
        self.accs = [torch.zeros(self.num_envs, dtype=torch.float32, device=self.device) if m == ALL_EPISODE else None for m in self.modes]
        self._all = None   # the all-True mask of `all-step` on the torch path

    @classmethod
    def from_cfg(cls, cfg, env, num_envs, window_len, device):
        return cls(getattr(cfg, "info_track_keys", None), getattr(cfg, "info_track_step", None), num_envs, window_len, device,
                   offered=getattr(env, "info_keys", None))

    def __len__(self):
        return len(self.keys)

    # ---- one env step ------------------------------------------------------------------------------
    @torch.no_grad()
    def update(self, done, info):
        """Exactly one window update per entry whose key this step's info holds."""
        if not self.keys or not isinstance(info, dict):
            return
        hip, hip_ok = [], self.device.type == "cuda" and done.dtype == torch.bool and done.is_contiguous() and done.numel() == self.num_envs
        for i, key in enumerate(self.keys):
            if key not in info:
                continue
            v = info[key]
            if v.numel() != self.num_envs:
                raise ValueError(f"info_track_keys entry {key!r}: info[{key!r}] has shape {tuple(v.shape)}, expected one value per env "
                                 f"({self.num_envs})")
            if (hip_ok and v.is_cuda and v.device == self.device and v.is_contiguous()
                    and v.dtype in (torch.float32, torch.bool, torch.uint8)):
                hip.append((i, v))
            else:
                self._update_torch(i, done, v)
        if hip:
            self._update_hip(done, hip)

    def _update_torch(self, i, done, v):
        """The definition (and the CPU path): masked device ops, no host sync."""
        v = v.reshape(-1)
        v = v.ne(0).to(torch.float32) if v.dtype in (torch.bool, torch.uint8) else v.to(torch.float32)
        v, finished = v.to(self.device), done.reshape(-1).bool()
        tracker, mode = self.trackers[i], self.modes[i]
        if mode == LAST:
            tracker.update(v, finished)
        elif mode == ALL_EPISODE:
            acc = self.accs[i]
            acc += v
            tracker.update(acc, finished)
            acc.masked_fill_(finished, 0)
        else:
            if self._all is None:
                self._all = torch.ones(self.num_envs, dtype=torch.bool, device=self.device)
            tracker.update(v, self._all)

    def _update_hip(self, done, entries):
        """`pqlk_rollout_info`: one launch per 8 entries, one block each."""
        with torch.cuda.device(self.device):
            for s in range(0, len(entries), L.INFO_MAX_KEYS):
                part = entries[s:s + L.INFO_MAX_KEYS]
                arr = (L.PqlInfoKey * len(part))()
                for slot, (i, v) in zip(arr, part):
                    acc, tr = self.accs[i], self.trackers[i]
                    slot.values, slot.acc = v.data_ptr(), None if acc is None else acc.data_ptr()
                    slot.ring, slot.ring_ptr = tr.ring.data_ptr(), tr.ptr.data_ptr()
                    slot.dtype, slot.mode = L.INFO_F32 if v.dtype == torch.float32 else L.INFO_U8, self.modes[i]
                L.check(L.lib.pqlk_rollout_info(self.num_envs, L.ptr(done), self.window_len, len(part), arr, L.stream(self.device)))

    # ---- what the log reads --------------------------------------------------------------------------
    def windows(self):
        """(n_keys, window_len): the windows stacked, for ONE read-back."""
        return torch.stack([t.ring[: self.window_len] for t in self.trackers])

    def means(self):
        """{key: mean over all window slots, zero-filled like common.Tracker} (each a host read, like `DeviceTracker.mean`)."""
        return {key: t.mean() for key, t in zip(self.keys, self.trackers)}

    def add_to_log(self, log_info):
        """`add_info_tracker_log` (pql_actor.py:148-151, ac_base.py:116-119): the means under the bare key names."""
        log_info.update(self.means())
        return log_info

    # ---- training state ------------------------------------------------------------------------------
    def training_state(self):
        return {"keys": list(self.keys), "steps": list(self.spellings), "trackers": [t.training_state() for t in self.trackers],
                "accs": [None if a is None else a.detach().cpu() for a in self.accs]}

    @torch.no_grad()
    def load_training_state(self, st):
        """st None (a checkpoint from before the keys were tracked): the trackers start from zero."""
        if st is None:
            for t, a in zip(self.trackers, self.accs):
                t.ring.zero_()
                t.ptr.zero_()
                if a is not None:
                    a.zero_()
            return
        saved = list(zip(st["keys"], (MODES.get(m) for m in st["steps"])))
        if saved != list(zip(self.keys, self.modes)):
            raise ValueError(f"InfoTrackers.load_training_state: the checkpoint tracks info_track_keys={list(st['keys'])!r} with "
                             f"info_track_step={list(st['steps'])!r}, but the configured ones are info_track_keys={self.keys!r} with "
                             f"info_track_step={self.spellings!r}")
        for t, a, ts, sa in zip(self.trackers, self.accs, st["trackers"], st["accs"]):
            if tuple(ts["ring"].shape) != tuple(t.ring.shape) or (a is not None and tuple(sa.shape) != tuple(a.shape)):
                raise ValueError(f"InfoTrackers.load_training_state: the checkpoint's windows hold {ts['ring'].numel() - 1} values for "
                                 f"{None if sa is None else sa.numel()} envs, the configured ones {self.window_len} for {self.num_envs}")
            t.load_training_state(ts)
            if a is not None:
                a.copy_(sa)
