"""Training-state checkpoints: the on-disk form and the process-level state.

A checkpoint is a DIRECTORY `<dir>/step-<global_steps>/`:
    state.pt        one `torch.save` of a nested dict of tensors / numbers / strings / lists / tuples / dicts
                    (`torch.load(..., weights_only=True)` reads it back), replay rings excluded
    ring_<x>.bin    one raw little-endian fp32 file per replay ring: records [0, cur_capacity), pads included
`state.pt` records every ring file's byte length and SHA-256 (`state["rings"]`); load checks the length always and the hash
with `verify=True`.  Rings are streamed through ONE reusable staging buffer of `STAGING_BYTES` (pinned when a GPU is
present): host memory used by save or load does not grow with the ring.

Publishing is atomic: everything is written into `<dir>/.tmp-<pid>-<n>/`, fsynced, renamed to `step-<N>`, and then the
one-line file `<dir>/latest` is replaced.  A `.tmp-*` left by a killed run is never read and is removed by the next save;
the `keep` newest checkpoints stay.

This module needs neither libpqlk.so nor a GPU (it must not import pql_amd._lib): the component state itself comes from the
`training_state()` / `load_training_state()` methods of the learners, the rollout actor, the replay rings and the env.
"""
from __future__ import annotations

import hashlib
import os
import random
import shutil
import sys

import numpy as np
import torch

STAGING_BYTES = 64 << 20   # one staging buffer for every ring of a save / load (<= 256 MiB by contract)
FORMAT = 1
_TMP = ".tmp-"
_STEP = "step-"
_serial = 0


# ------------------------------------------------------------------------------------------------ staging + ring streams
class Staging:
    """The one host buffer ring chunks travel through.  `allocations` / `nbytes` let a test see that nothing else is allocated."""

    allocations = 0   # buffers created by this process (class-wide)

    def __init__(self, nbytes=STAGING_BYTES):
        if nbytes < 4 or nbytes > (256 << 20):
            raise ValueError(f"staging buffer of {nbytes} bytes: must be 4 B .. 256 MiB")
        self.nbytes = int(nbytes) // 4 * 4
        self._buf = None

    @property
    def buf(self):
        if self._buf is None:
            self._buf = torch.empty(self.nbytes // 4, dtype=torch.float32, pin_memory=torch.cuda.is_available())
            Staging.allocations += 1
        return self._buf


def _flat_f32(t):
    if t.dtype != torch.float32 or not t.is_contiguous():
        raise ValueError("ring data must be a contiguous fp32 tensor")
    return t.view(-1)


def write_ring(path, tensor, staging):
    """Stream `tensor` (contiguous fp32, any device) to `path` chunk by chunk; returns {"bytes", "sha256"}."""
    if sys.byteorder != "little":
        raise RuntimeError("ring files are little-endian; this host is not")
    src = _flat_f32(tensor)
    n, chunk = src.numel(), staging.nbytes // 4
    sha = hashlib.sha256()
    host = staging.buf.numpy()
    with open(path, "wb") as f:
        for off in range(0, n, chunk):
            m = min(chunk, n - off)
            staging.buf[:m].copy_(src[off: off + m])   # (blocking: the buffer is reused for the next chunk)
            view = memoryview(host[:m]).cast("B")
            sha.update(view)
            f.write(view)
        f.flush()
        os.fsync(f.fileno())
    return {"bytes": 4 * n, "sha256": sha.hexdigest()}


def read_ring(path, tensor, staging, meta, verify=False):
    """Stream `path` into `tensor` (contiguous fp32, any device).  The file's length must equal `meta["bytes"]` and the
    tensor's; with `verify` the SHA-256 of what was read must equal `meta["sha256"]`."""
    dst = _flat_f32(tensor)
    n, chunk = dst.numel(), staging.nbytes // 4
    size = os.path.getsize(path)
    if size != int(meta["bytes"]) or size != 4 * n:
        raise ValueError(f"{path}: {size} bytes on disk, checkpoint recorded {int(meta['bytes'])}, ring expects {4 * n}")
    sha = hashlib.sha256() if verify else None
    host = staging.buf.numpy()
    with open(path, "rb") as f:
        for off in range(0, n, chunk):
            m = min(chunk, n - off)
            view = memoryview(host[:m]).cast("B")
            got = f.readinto(view)
            if got != 4 * m:
                raise ValueError(f"{path}: short read at byte {4 * off}")
            if sha is not None:
                sha.update(view)
            dst[off: off + m].copy_(staging.buf[:m])
    if sha is not None and sha.hexdigest() != meta["sha256"]:
        raise ValueError(f"{path}: SHA-256 mismatch (file {sha.hexdigest()[:16]}.., checkpoint recorded {str(meta['sha256'])[:16]}..)")


# ------------------------------------------------------------------------------------------------ directory protocol
def _fsync_dir(path):
    fd = os.open(path, os.O_RDONLY)
    try:
        os.fsync(fd)
    finally:
        os.close(fd)


def _steps(root):
    """[(global_steps, name)] of the published checkpoints under `root`, oldest first."""
    out = []
    for name in os.listdir(root):
        if name.startswith(_STEP) and name[len(_STEP):].isdigit() and os.path.isfile(os.path.join(root, name, "state.pt")):
            out.append((int(name[len(_STEP):]), name))
    return sorted(out)


def save(root, global_steps, state, rings=None, keep=2, staging=None):
    """Publish one checkpoint under `root`; returns its path.  state: nested dict (see module docstring); rings: {file stem:
    contiguous fp32 tensor}, streamed through `staging` (a `Staging`; default: one of STAGING_BYTES)."""
    global _serial
    os.makedirs(root, exist_ok=True)
    for name in os.listdir(root):   # what a killed run left behind
        if name.startswith(_TMP):
            stale = os.path.join(root, name)
            shutil.rmtree(stale, ignore_errors=True) if os.path.isdir(stale) else os.remove(stale)
    _serial += 1
    tmp = os.path.join(root, f"{_TMP}{os.getpid()}-{_serial}")
    os.makedirs(tmp)
    meta = {}
    if rings:
        staging = staging or Staging()
        for stem, tensor in rings.items():
            meta[stem] = write_ring(os.path.join(tmp, f"{stem}.bin"), tensor, staging)
    state = dict(state, format=FORMAT, global_steps=int(global_steps), rings=meta)
    with open(os.path.join(tmp, "state.pt"), "wb") as f:
        torch.save(state, f)
        f.flush()
        os.fsync(f.fileno())
    _fsync_dir(tmp)
    name = f"{_STEP}{int(global_steps)}"
    final = os.path.join(root, name)
    if os.path.exists(final):   # the same step saved twice (a resumed run that stops where it started)
        old = os.path.join(root, f"{_TMP}{os.getpid()}-{_serial}-old")
        os.replace(final, old)
        shutil.rmtree(old, ignore_errors=True)
    os.replace(tmp, final)
    latest_tmp = os.path.join(root, f"{_TMP}latest-{os.getpid()}")
    with open(latest_tmp, "w") as f:
        f.write(name + "\n")
        f.flush()
        os.fsync(f.fileno())
    os.replace(latest_tmp, os.path.join(root, "latest"))
    _fsync_dir(root)
    published = [n for _, n in _steps(root) if n != name]   # `keep` newest stay; the one just written is the newest by definition
    for old_name in published[: max(0, len(published) - (max(1, int(keep)) - 1))]:
        shutil.rmtree(os.path.join(root, old_name), ignore_errors=True)
    return final


def resolve(path):
    """`path` is a `step-*` directory, or its parent (then `latest` decides).  Returns the checkpoint directory."""
    path = os.path.abspath(str(path))
    if os.path.isfile(os.path.join(path, "state.pt")):
        return path
    latest = os.path.join(path, "latest")
    if os.path.isfile(latest):
        with open(latest) as f:
            name = f.read().strip()
        cand = os.path.join(path, name)
        if name.startswith(_STEP) and os.path.isfile(os.path.join(cand, "state.pt")):
            return cand
    raise FileNotFoundError(f"resume={path}: neither a checkpoint directory (state.pt) nor a directory whose `latest` names one")


def load(path):
    """(checkpoint directory, state dict).  Ring files are read afterwards, into their rings, with `load_ring`."""
    ckpt = resolve(path)
    state = torch.load(os.path.join(ckpt, "state.pt"), map_location="cpu", weights_only=True)
    if state.get("format") != FORMAT:
        raise ValueError(f"{ckpt}: checkpoint format {state.get('format')}, this build reads {FORMAT}")
    for stem, meta in state["rings"].items():   # lengths are checked before anything is restored
        f = os.path.join(ckpt, f"{stem}.bin")
        if not os.path.isfile(f) or os.path.getsize(f) != int(meta["bytes"]):
            raise ValueError(f"{f}: missing or truncated ({os.path.getsize(f) if os.path.isfile(f) else 0} bytes, "
                             f"checkpoint recorded {int(meta['bytes'])})")
    return ckpt, state


def load_ring(ckpt, state, stem, tensor, staging=None, verify=False):
    read_ring(os.path.join(ckpt, f"{stem}.bin"), tensor, staging or Staging(), state["rings"][stem], verify)


# ------------------------------------------------------------------------------------------------ config
def options(cfg):
    """(resume, dir, freq, keep, replay, verify) of a composed config."""
    ck = cfg.get("checkpoint") or {}
    freq = ck.get("freq")
    return dict(resume=cfg.get("resume"), dir=ck.get("dir"), freq=None if freq is None else max(1, int(freq)),
                keep=int(ck.get("keep") if ck.get("keep") is not None else 2),
                replay=bool(ck.get("replay") if ck.get("replay") is not None else True), verify=bool(ck.get("verify") or False))


def refuse(cfg, world=1):
    """What resume / checkpointing does not cover yet is an error at start-up, not a silent no-op."""
    opt = options(cfg)
    if opt["resume"] is None and opt["dir"] is None:
        return
    what = "resume" if opt["resume"] is not None else "checkpoint.dir"
    if world > 1:
        raise ValueError(f"{what} is single-process only: data-parallel ranks (WORLD_SIZE={world}) would have to agree on the "
                         f"save iteration and write per-rank shards")
    if cfg.algo.name == "PPO":
        raise ValueError(f"{what} does not cover algo=ppo_algo (permutation stream, value_rms and trajectory slabs are not saved)")


def structure(cfg, obs_dim, act_dim):
    """The part of the config a checkpoint's tensors depend on.  Learning rates, batch_size, max_step / max_time and logging keys
    are free to differ between the run that saved and the run that resumes."""
    from pql_amd.algo import critics   # (loads libpqlk.so through the model files: put off to this call, which every caller makes with it loaded)
    algo = cfg.algo
    hidden = algo.get("hidden_layers")
    distl = bool(algo.get("distl") or False)
    per = algo.get("per") or {}
    per_on = bool(per.get("enabled") or False)
    return {"task.obs_dim": int(obs_dim), "task.act_dim": int(act_dim), "num_envs": int(cfg.num_envs),
            "algo.hidden_layers": None if hidden is None else [int(h) for h in hidden],
            "algo.act_class": str(algo.get("act_class")), "algo.distl": distl,
            "algo.cri_class": critics.critic_rules(algo).name,   # (without the Distributional the V-learner puts in front when algo.distl is set)
            "algo.num_atoms": int(algo.get("num_atoms") or 0) if distl else 0,
            # (the class's own keys -- the quantile heads' width, the residual critic's width and depth; 0 for every other class)
            **critics.structure_keys(algo), "algo.nstep": int(algo.get("nstep") or 1),
            "algo.memory_size": int(algo.get("memory_size") or 0),
            "algo.replay_obs_dtype": str(algo.get("replay_obs_dtype") or "float32"),
            # (the V-learner's target forwards: bf16 targets change every later step, so a run resumes in the dtype it was saved in)
            "algo.target_dtype": str(algo.get("target_dtype") or "float32"),
            # (prioritized replay: the ring carries a sum tree of priority^alpha; alpha, and when the priorities are refreshed --
            #  every step, or once per run of prefetched steps -- count only when it is on)
            "algo.per.enabled": per_on, "algo.per.alpha": float(per.get("alpha")) if per_on else None,
            "algo.per.refresh": str(per.get("refresh") or "step") if per_on else None}


def check_structure(saved, current, has_rings=True):
    # (a checkpoint from before a key existed was written with float32 targets, uniform replay, none of the critic classes that have
    #  structure keys of their own; prioritized, with per-step refresh)
    from pql_amd.algo.critics import STRUCTURE_DEFAULTS
    saved = {"algo.target_dtype": "float32", "algo.per.enabled": False, "algo.per.alpha": None, **STRUCTURE_DEFAULTS, **saved}
    saved.setdefault("algo.per.refresh", "step" if saved["algo.per.enabled"] else None)
    for key, want in saved.items():
        if key in ("algo.memory_size", "algo.replay_obs_dtype") and not has_rings:
            continue
        have = current.get(key)
        if isinstance(want, (list, tuple)):
            want, have = list(want), (None if have is None else list(have))
        if have != want:
            raise ValueError(f"resume: {key}={have!r} but the checkpoint was written with {key}={want!r}")


# ------------------------------------------------------------------------------------------------ process state
def process_state(devices=()):
    """torch CPU generator, the default CUDA generator of every device in `devices`, NumPy and Python `random`."""
    kind, keys, pos, has_gauss, gauss = np.random.get_state()
    py = random.getstate()
    return {"torch_cpu": torch.get_rng_state(),
            "torch_cuda": {int(torch.device(d).index or 0): torch.cuda.get_rng_state(d) for d in devices},
            "numpy": (str(kind), torch.from_numpy(keys.astype(np.int64)), int(pos), int(has_gauss), float(gauss)),
            "python": (int(py[0]), [int(x) for x in py[1]], py[2])}


def load_process_state(st):
    torch.set_rng_state(st["torch_cpu"])
    for idx, s in st["torch_cuda"].items():
        torch.cuda.set_rng_state(s, int(idx))
    kind, keys, pos, has_gauss, gauss = st["numpy"]
    np.random.set_state((kind, keys.numpy().astype(np.uint32), int(pos), int(has_gauss), float(gauss)))
    py = st["python"]
    random.setstate((int(py[0]), tuple(int(x) for x in py[1]), py[2]))


def sha(t, rows=None):
    """16-hex-digit SHA-256 of a tensor's bytes (first `rows` rows): the fingerprints the entry points return."""
    t = t.detach()
    if rows is not None:
        t = t[:rows]
    return hashlib.sha256(t.contiguous().cpu().numpy().tobytes()).hexdigest()[:16]


def sha_stream(tensor, staging=None):
    """The same fingerprint for a replay ring, hashed chunk by chunk through the staging buffer (no host copy of the ring)."""
    src, staging = _flat_f32(tensor), staging or Staging()
    h, chunk, host = hashlib.sha256(), staging.nbytes // 4, staging.buf.numpy()
    for off in range(0, src.numel(), chunk):
        m = min(chunk, src.numel() - off)
        staging.buf[:m].copy_(src[off: off + m])
        h.update(memoryview(host[:m]).cast("B"))
    return h.hexdigest()[:16]
