"""Half-precision observation storage of the replay rings (PQLK_OBS_F16, `algo.replay_obs_dtype`), the parts that need no GPU:
record widths, the config key, the public header and the drain counts of the built fp16 gather kernels."""
import os
import re

import pytest

from task_cases import load_script

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, F16 = 0, 1


def _ld_h(O, A):
    """Word count of the fp16 record as the header states it."""
    oh = (O + 7) // 8 * 8 // 2
    used = oh if A < 0 else 2 * oh + (A + 3) // 4 * 4 + 4
    return (used + 31) // 32 * 32


def test_record_widths():
    from pql_amd import _lib as L
    ex = L.lib.pqlk_replay_rec_ld_ex
    assert L.OBS_F32 == F32 and L.OBS_F16 == F16
    for (O, A), want in {(88, 16): 128, (211, 20): 256, (108, 21): 160, (88, -1): 64, (3, 1): 32}.items():
        assert ex(O, A, F16) == want == _ld_h(O, A), (O, A)
    shapes = [(8, 2), (88, 16), (211, 20), (108, 21), (3, 1), (13, 5), (600, 7), (1, 1), (88, -1), (3, -1), (211, -1), (600, -1), (255, 4)]
    for O, A in shapes:
        assert ex(O, A, F32) == L.lib.pqlk_replay_rec_ld(O, A) > 0, (O, A)
        assert ex(O, A, F16) == _ld_h(O, A) and ex(O, A, F16) % 32 == 0, (O, A)
        assert ex(O, A, F16) <= ex(O, A, F32)
    # records per GB at the benchmarked shapes: 896 -> 512 B, 384 -> 256 B, 1792 -> 1024 B, 1024 -> 640 B
    assert [4 * ex(*s, F32) for s in ((88, 16), (88, -1), (211, 20), (108, 21))] == [896, 384, 1792, 1024]
    assert [4 * ex(*s, F16) for s in ((88, 16), (88, -1), (211, 20), (108, 21))] == [512, 256, 1024, 640]
    assert ex(0, 2, F16) == 0 and ex(8, 2, 2) == 0 and ex(8, 2, -1) == 0   # bad width / unknown dtype


def test_descriptor_keeps_its_size_and_positional_constructor():
    import ctypes as C
    from pql_amd import _lib as L
    assert C.sizeof(L.PqlReplayDesc) == 32
    d = L.PqlReplayDesc(None, 10, 8, 2, 32, 0)
    assert d.obs_dtype == 0
    assert L.PqlReplayDesc(None, 10, 8, 2, 32, 1).obs_dtype == 1
    assert [f[0] for f in L.PqlReplayDesc._fields_] == ["records", "capacity", "obs_dim", "act_dim", "rec_ld", "obs_dtype"]


def test_config_key_composes_and_bad_values_are_refused():
    import torch
    from pql_amd.replay.simple_replay import cfg_obs_dtype, parse_obs_dtype
    from pql_amd.utils.cfg import load_cfg
    assert load_cfg([]).algo.replay_obs_dtype == "float32"                       # the default: nothing changes
    for algo in ("pql_algo", "ddpg_algo", "sac_algo", "crossq_algo"):
        assert cfg_obs_dtype(load_cfg([f"algo={algo}"]).algo) == torch.float32
        assert cfg_obs_dtype(load_cfg([f"algo={algo}", "algo.replay_obs_dtype=float16"]).algo) == torch.float16
    for bad in ("bfloat16", "half", "fp16", "16"):
        with pytest.raises(ValueError, match="algo.replay_obs_dtype"):
            cfg_obs_dtype(load_cfg([f"algo.replay_obs_dtype={bad}"]).algo)
    assert parse_obs_dtype(torch.float16) == torch.float16 and parse_obs_dtype("float32") == torch.float32
    with pytest.raises(ValueError):
        parse_obs_dtype(torch.bfloat16)


def test_structure_of_a_checkpoint_names_the_dtype():
    from pql_amd.utils import checkpoint as CK
    from pql_amd.utils.cfg import load_cfg
    a = CK.structure(load_cfg([]), 8, 2)
    b = CK.structure(load_cfg(["algo.replay_obs_dtype=float16"]), 8, 2)
    assert a["algo.replay_obs_dtype"] == "float32" and b["algo.replay_obs_dtype"] == "float16"
    with pytest.raises(ValueError, match="obs_dtype"):
        CK.check_structure(a, b)
    with pytest.raises(ValueError, match="obs_dtype"):
        CK.check_structure(b, a)
    CK.check_structure(a, b, has_rings=False)                                     # a checkpoint without rings: free to differ
    old = {k: v for k, v in a.items() if k != "algo.replay_obs_dtype"}            # written before the key existed
    CK.check_structure(old, a)


def test_header_and_library_export_the_new_symbol():
    import ctypes as C
    from pql_amd import _lib as L
    hdr = open(os.path.join(ROOT, "include", "pqlk.h")).read()
    assert re.search(r"int64_t\s+pqlk_replay_rec_ld_ex\(int32_t obs_dim, int32_t act_dim, int32_t obs_dtype\);", hdr)
    assert re.search(r"PQLK_OBS_F32\s*=\s*0", hdr) and re.search(r"PQLK_OBS_F16\s*=\s*1", hdr)
    assert re.search(r"int32_t\s+obs_dtype;", hdr) and not re.search(r"int32_t\s+reserved;", hdr)
    assert "pqlk_replay_rec_ld_ex" in L.PROTOTYPES
    assert hasattr(C.CDLL(os.fspath(L.LIB_FILE)), "pqlk_replay_rec_ld_ex")


def test_fp16_gather_kernels_keep_their_counted_waits():
    """The fp16 counterparts of k_replay_gather_fast / k_replay_gather_obs are held to the limits
    test_gather_kernels_keep_their_counted_waits holds the fp32 kernels to: at most 3 full drains of the vector-memory queue
    (`s_waitcnt vmcnt(0)`) in the fast kernel, 5 in the obs kernel.  7 instantiations each, as there (4 + 3 with normalisation), of
    the 16-B-chunk kernels (`_f16`) and of the 8-B-chunk kernels that serve records of at most 512 B (`_h8`)."""
    kr = load_script("tools/kernel_resources.py", "kernel_resources")
    if not os.path.exists(f"{kr.LLVM}/llvm-objdump"):
        pytest.skip("no llvm-objdump")
    drains = kr.full_drains(want=("k_replay_gather_fast_f16<true", "k_replay_gather_obs_f16<true", "k_replay_gather_fast_h8<true",
                                  "k_replay_gather_obs_h8<true"))
    assert len(drains) == 14, sorted(drains)
    for name, n in drains.items():
        limit = 3 if "gather_fast" in name else 5
        assert n <= limit, f"{name}: {n} full drains of the vector-memory queue"
