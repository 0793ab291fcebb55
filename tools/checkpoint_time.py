#!/usr/bin/env python3
"""What a training-state save and load cost: builds the two learners at a given shape, fills both rings, and times
`checkpoint.save` / `checkpoint.load` + ring reads with the host clock around a device synchronisation (median of `--repeat`).
The yardstick is a plain sequential write (and read back) of the same number of bytes into the same directory with the same
chunk size -- what the disk under `--dir` gives, not what this code does.

    python tools/checkpoint_time.py --dir /scratch/ck --out profiles/checkpoint_time.json                  # cfg #2: 1 M rows
    python tools/checkpoint_time.py --dir /scratch/ck --rows 5000000 --num-envs 16384 --label cfg4_5M      # cfg #4 at 5 M rows
"""
import argparse
import json
import os
import shutil
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from pql_amd.algo.pql_p_learner import PQLPLearner  # noqa: E402
from pql_amd.algo.pql_v_learner import PQLVLearner  # noqa: E402
from pql_amd.utils import checkpoint as CK  # noqa: E402
from pql_amd.utils.cfg import load_cfg  # noqa: E402


def plain_write_read(path, nbytes, chunk):
    """dd-style: sequential write of `nbytes` in `chunk`-byte pieces + fsync, then a sequential read back."""
    buf = bytearray(os.urandom(1 << 20) * (chunk >> 20)) if chunk >= (1 << 20) else bytearray(os.urandom(chunk))
    t0 = time.perf_counter()
    with open(path, "wb") as f:
        left = nbytes
        while left > 0:
            n = min(left, len(buf))
            f.write(memoryview(buf)[:n])
            left -= n
        f.flush()
        os.fsync(f.fileno())
    t1 = time.perf_counter()
    with open(path, "rb") as f:
        while f.readinto(buf):
            pass
    t2 = time.perf_counter()
    os.remove(path)
    return t1 - t0, t2 - t1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dir", required=True, help="directory the checkpoints (and the plain file) are written into")
    ap.add_argument("--task", default="AllegroHand")
    ap.add_argument("--rows", type=int, default=1_000_000, help="rows in each ring (= algo.memory_size, rings full)")
    ap.add_argument("--num-envs", type=int, default=4096)
    ap.add_argument("--batch", type=int, default=8192)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--label", default="cfg2_1M")
    ap.add_argument("--out", default=None, help="JSON file to write (entries of other labels in it are kept)")
    a = ap.parse_args()

    cfg = load_cfg([f"task={a.task}", f"num_envs={a.num_envs}", f"algo.batch_size={a.batch}", f"algo.memory_size={a.rows}", "algo.num_gpus=1",
                    "algo.v_learner_gpu=0", "algo.p_learner_gpu=0", "device=cuda:0"])
    from pql_amd.envs.synthetic import TASK_SHAPES
    O, A = TASK_SHAPES[a.task]
    dev = torch.device("cuda:0")
    v, p = PQLVLearner((O,), A, cfg), PQLPLearner((O,), A, cfg)
    gen = torch.Generator(device=dev).manual_seed(1)
    block = 65536
    for start in range(0, a.rows, block):   # fill both rings through their own insert paths
        n = min(block, a.rows - start)
        rnd = lambda *s: torch.randn(s, device=dev, generator=gen)   # noqa: E731
        traj = (rnd(n, O), rnd(n, A), rnd(n, 1), rnd(n, O), (rnd(n, 1) > 2).float())
        v.update(p.actor, traj, None, 0)
        p.update(v.critic, traj[0], None, 0)
    torch.cuda.synchronize()
    assert v.memory.cur_capacity == a.rows == p.cur_capacity

    def state():
        return {"v_learner": v.training_state(), "p_learner": p.training_state(), "process": CK.process_state([dev])}

    def rings():
        return {"ring_v": v.memory.rows(), "ring_p": p.ring.rows(p.cur_capacity)}

    root = os.path.join(a.dir, f"checkpoint_time_{os.getpid()}")
    staging = CK.Staging()
    staging.buf   # (allocated outside the timed region, as a training run allocates it once)
    nbytes = sum(t.numel() * 4 for t in rings().values())
    save_s, load_s, load_verify_s = [], [], []
    for k in range(a.repeat):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        CK.save(root, k, state(), rings(), keep=1, staging=staging)
        save_s.append(time.perf_counter() - t0)
        for verify, acc in ((False, load_s), (True, load_verify_s)):
            t0 = time.perf_counter()
            ckpt, st = CK.load(root)
            v.load_training_state(st["v_learner"])
            p.load_training_state(st["p_learner"])
            CK.load_ring(ckpt, st, "ring_v", v.memory.rows(), staging, verify)
            CK.load_ring(ckpt, st, "ring_p", p.ring.rows(p.cur_capacity), staging, verify)
            torch.cuda.synchronize()
            acc.append(time.perf_counter() - t0)
    state_bytes = os.path.getsize(os.path.join(root, f"step-{a.repeat - 1}", "state.pt"))
    plain = [plain_write_read(os.path.join(root, "plain.bin"), nbytes, staging.nbytes) for _ in range(a.repeat)]
    # where a save's time goes: the device -> pinned host copies alone, and the SHA-256 alone, over the same bytes
    t0 = time.perf_counter()
    for t in rings().values():
        flat, chunk = t.view(-1), staging.nbytes // 4
        for off in range(0, flat.numel(), chunk):
            m = min(chunk, flat.numel() - off)
            staging.buf[:m].copy_(flat[off: off + m])
    d2h_s = time.perf_counter() - t0
    import hashlib
    t0 = time.perf_counter()
    h, view = hashlib.sha256(), memoryview(staging.buf.numpy()).cast("B")
    for _ in range(0, nbytes, staging.nbytes):
        h.update(view)
    sha_s = time.perf_counter() - t0
    shutil.rmtree(root, ignore_errors=True)
    med = statistics.median
    pw, pr = med(x[0] for x in plain), med(x[1] for x in plain)
    gbs = lambda s: round(nbytes / s / 1e9, 3)   # noqa: E731
    entry = dict(label=a.label, task=a.task, rows=a.rows, ring_v_bytes=v.memory.rows().numel() * 4, ring_p_bytes=p.ring.rows(a.rows).numel() * 4,
                 ring_bytes=nbytes, state_pt_bytes=state_bytes, staging_bytes=staging.nbytes, repeat=a.repeat,
                 save_s=round(med(save_s), 4), save_GBps=gbs(med(save_s)), load_s=round(med(load_s), 4), load_GBps=gbs(med(load_s)),
                 load_verify_s=round(med(load_verify_s), 4), load_verify_GBps=gbs(med(load_verify_s)),
                 plain_write_s=round(pw, 4), plain_write_GBps=gbs(pw), plain_read_s=round(pr, 4), plain_read_GBps=gbs(pr),
                 save_vs_plain_write=round(pw / med(save_s), 3), d2h_only_s=round(d2h_s, 4), sha256_only_s=round(sha_s, 4),
                 device=torch.cuda.get_device_name(0))
    print(json.dumps(entry))
    if a.out:
        doc = json.load(open(a.out)) if os.path.isfile(a.out) else {}
        doc[a.label] = entry
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
