"""The on-disk form of a training-state checkpoint (pql_amd/utils/checkpoint.py) and the config / env ends of resume: everything
that needs neither a GPU nor libpqlk.so."""
import os
import subprocess
import sys

import pytest
import torch

from pql_amd.utils import checkpoint as CK
from pql_amd.utils.cfg import load_cfg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _state(tag):
    return {"iter_t": tag, "weights": torch.full((5,), float(tag)), "nested": {"names": ["a", "b"], "pair": (1, 2.5), "none": None},
            "process": CK.process_state()}


def _ring(rows=300, ld=7, seed=0):
    return torch.randn((rows, ld), generator=torch.Generator().manual_seed(seed))


def test_module_needs_no_native_library():
    """`import pql_amd.utils.checkpoint` must not pull in pql_amd._lib (it would load libpqlk.so)."""
    code = "import sys; import pql_amd.utils.checkpoint; assert 'pql_amd._lib' not in sys.modules, 'pql_amd._lib was imported'"
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]


def test_directory_protocol(tmp_path):
    root, staging = str(tmp_path / "ck"), CK.Staging(4096)
    ring_a, ring_b = _ring(seed=1), _ring(rows=123, seed=2)
    first = CK.save(root, 1000, _state(1), {"ring_v": ring_a, "ring_p": ring_b}, keep=1, staging=staging)
    assert os.path.basename(first) == "step-1000" and sorted(os.listdir(first)) == ["ring_p.bin", "ring_v.bin", "state.pt"]
    assert open(os.path.join(root, "latest")).read() == "step-1000\n"
    assert CK.resolve(root) == first == CK.resolve(first)
    ckpt, st = CK.load(root)
    assert st["iter_t"] == 1 and st["global_steps"] == 1000 and st["nested"] == {"names": ["a", "b"], "pair": (1, 2.5), "none": None}
    assert st["rings"]["ring_v"]["bytes"] == ring_a.numel() * 4 and len(st["rings"]["ring_v"]["sha256"]) == 64
    # a stray temporary directory (a killed run) is ignored by load and gone after the next save; keep=1 removes the first
    stray = os.path.join(root, ".tmp-99999-1")
    os.makedirs(stray)
    open(os.path.join(stray, "state.pt"), "wb").write(b"torn")
    assert CK.load(root)[0] == first
    second = CK.save(root, 2000, _state(2), {"ring_v": ring_b, "ring_p": ring_a}, keep=1, staging=staging)
    assert sorted(os.listdir(root)) == ["latest", "step-2000"]
    ckpt, st = CK.load(root)
    assert ckpt == second and st["iter_t"] == 2 and torch.equal(st["weights"], torch.full((5,), 2.0))
    # keep=2 keeps the two newest; the same step saved twice replaces itself
    CK.save(root, 3000, _state(3), None, keep=2)
    CK.save(root, 4000, _state(4), None, keep=2)
    CK.save(root, 4000, _state(5), None, keep=2)
    assert sorted(os.listdir(root)) == ["latest", "step-3000", "step-4000"] and CK.load(root)[1]["iter_t"] == 5
    assert CK.load(os.path.join(root, "step-3000"))[1]["rings"] == {}
    with pytest.raises(FileNotFoundError):
        CK.resolve(str(tmp_path / "nothing"))


def test_damaged_ring_files_are_refused(tmp_path):
    root, staging = str(tmp_path / "ck"), CK.Staging(4096)
    ring = _ring()
    path = CK.save(root, 10, _state(1), {"ring": ring}, staging=staging)
    ckpt, st = CK.load(root)
    dst = torch.zeros_like(ring)
    CK.load_ring(ckpt, st, "ring", dst, staging, verify=True)
    assert torch.equal(dst, ring)
    f = os.path.join(path, "ring.bin")
    raw = bytearray(open(f, "rb").read())
    raw[len(raw) // 2] ^= 0x01
    open(f, "wb").write(bytes(raw))             # a flipped byte: same length
    CK.load_ring(ckpt, st, "ring", dst, staging, verify=False)
    with pytest.raises(ValueError, match="SHA-256"):
        CK.load_ring(ckpt, st, "ring", dst, staging, verify=True)
    open(f, "wb").write(bytes(raw[:-8]))        # truncated: refused before anything is restored, verify or not
    with pytest.raises(ValueError, match="truncated"):
        CK.load(root)
    with pytest.raises(ValueError, match="bytes"):
        CK.load_ring(ckpt, st, "ring", dst, staging, verify=False)
    with pytest.raises(ValueError, match="bytes"):   # a ring of another size than the file
        CK.read_ring(f, torch.zeros(10, 7), staging, st["rings"]["ring"])


def test_chunked_ring_stream_round_trips_through_one_small_buffer(tmp_path):
    staging = CK.Staging(4096)
    ring = _ring(rows=1237, ld=7, seed=3)                      # 34 636 B: 8 full chunks and a partial one
    assert (ring.numel() * 4) % staging.nbytes != 0 and ring.numel() * 4 > 8 * staging.nbytes
    before = CK.Staging.allocations
    f = str(tmp_path / "ring.bin")
    meta = CK.write_ring(f, ring, staging)
    assert open(f, "rb").read() == ring.numpy().tobytes() and meta["bytes"] == ring.numel() * 4
    dst = torch.full_like(ring, float("nan"))
    CK.read_ring(f, dst, staging, meta, verify=True)
    assert dst.numpy().tobytes() == ring.numpy().tobytes()
    assert CK.sha_stream(ring, staging) == CK.sha(ring) == meta["sha256"][:16]
    # one buffer of the configured size for everything above, and the default is the named constant
    assert CK.Staging.allocations == before + 1 and staging.buf.numel() * 4 == staging.nbytes == 4096
    assert CK.Staging().nbytes == CK.STAGING_BYTES <= 256 << 20
    with pytest.raises(ValueError):
        CK.Staging(512 << 20)
    with pytest.raises(ValueError, match="contiguous"):
        CK.write_ring(f, ring[:, :3], staging)


BASE = ["task=Toy", "num_envs=64", "algo.batch_size=256", "algo.memory_size=20000"]


@pytest.mark.parametrize("override,key", [("algo.nstep=5", "algo.nstep"), ("num_envs=128", "num_envs"), ("algo.hidden_layers=[64,64]", "algo.hidden_layers"),
                                          ("algo.distl=True", "algo.distl"), ("algo.memory_size=30000", "algo.memory_size")])
def test_structural_config_mismatch_names_the_key(override, key):
    saved = CK.structure(load_cfg(BASE), 8, 2)
    with pytest.raises(ValueError, match=key.replace(".", r"\.") + "="):
        CK.check_structure(saved, CK.structure(load_cfg(BASE + [override]), 8, 2))


def test_non_structural_config_may_differ():
    saved = CK.structure(load_cfg(BASE), 8, 2)
    for override in ("algo.critic_lr=0.001", "max_step=123", "algo.batch_size=512", "max_time=5", "logging.jsonl=/tmp/x.jsonl"):
        CK.check_structure(saved, CK.structure(load_cfg(BASE + [override]), 8, 2))
    CK.check_structure(saved, CK.structure(load_cfg(BASE + ["algo.memory_size=30000"]), 8, 2), has_rings=False)   # no rings: free
    with pytest.raises(ValueError, match=r"task\.obs_dim"):
        CK.check_structure(saved, CK.structure(load_cfg(BASE), 9, 2))
    # the V-learner's rewrite of cri_class under algo.distl is not a difference
    a, b = load_cfg(BASE + ["algo.distl=True"]), load_cfg(BASE + ["algo.distl=True"])
    b.algo.cri_class = "Distributional" + b.algo.cri_class
    CK.check_structure(CK.structure(a, 8, 2), CK.structure(b, 8, 2))


def test_config_keys_and_defaults():
    cfg = load_cfg([])
    assert cfg.resume is None and dict(cfg.checkpoint) == {"dir": None, "freq": None, "keep": 2, "replay": True, "verify": False}
    assert CK.options(cfg) == dict(resume=None, dir=None, freq=None, keep=2, replay=True, verify=False)
    cfg = load_cfg(["resume=/x", "checkpoint.dir=/y", "checkpoint.freq=5", "checkpoint.replay=False"])
    assert cfg.resume == "/x" and CK.options(cfg) == dict(resume="/x", dir="/y", freq=5, keep=2, replay=False, verify=False)
    with pytest.raises(KeyError):
        load_cfg(["checkpoint.directory=/y"])


def test_refusals_need_no_gpu():
    CK.refuse(load_cfg(["algo=ppo_algo"]))                                   # nothing asked for: nothing refused
    CK.refuse(load_cfg([]), world=8)
    for key in ("resume=/x", "checkpoint.dir=/x"):
        with pytest.raises(ValueError, match="ppo_algo"):
            CK.refuse(load_cfg(["algo=ppo_algo", key]))
        with pytest.raises(ValueError, match="WORLD_SIZE=2"):
            CK.refuse(load_cfg([key]), world=2)
        CK.refuse(load_cfg([key]))
        CK.refuse(load_cfg(["algo=ddpg_algo", key]))


def test_process_state_round_trip():
    import random

    import numpy as np
    torch.manual_seed(7), np.random.seed(7), random.seed(7)
    torch.rand(3), np.random.rand(3), random.random()
    st = CK.process_state()
    want = (torch.rand(4), np.random.rand(4), np.random.randn(), [random.random() for _ in range(4)])
    torch.rand(10), np.random.rand(10), random.random()
    CK.load_process_state(st)
    got = (torch.rand(4), np.random.rand(4), np.random.randn(), [random.random() for _ in range(4)])
    assert torch.equal(want[0], got[0]) and (want[1] == got[1]).all() and want[2] == got[2] and want[3] == got[3]


def test_synthetic_env_state_round_trip(tmp_path):
    from pql_amd.envs.synthetic import SyntheticVecEnv
    mk = lambda: SyntheticVecEnv(16, 8, 2, device="cpu", seed=5, episode_length=20, env_offset=3)   # noqa: E731
    act = lambda k: torch.full((16, 2), 0.1 * k)   # noqa: E731
    env = mk()
    env.reset()
    for k in range(5):
        env.step(act(k))
    obs_then = env._obs.clone()
    torch.save({"env": env.state_dict()}, tmp_path / "s.pt")
    want = [env.step(act(k)) for k in range(5, 8)]
    fresh = mk()
    fresh.load_state_dict(torch.load(tmp_path / "s.pt", weights_only=True)["env"])
    assert fresh.t == 5 and torch.equal(fresh._obs, obs_then)
    got = [fresh.step(act(k)) for k in range(5, 8)]
    for (o1, r1, d1, _), (o2, r2, d2, _) in zip(want, got):
        assert torch.equal(o1, o2) and torch.equal(r1, r2) and torch.equal(d1, d2)
    with pytest.raises(ValueError, match="seed"):
        SyntheticVecEnv(16, 8, 2, device="cpu", seed=6, episode_length=20, env_offset=3).load_state_dict(env.state_dict())
