"""`algo.critic_target_dtype` with `algo.cri_class=DoubleQBroNet`, without a GPU: what is refused is a ValueError naming a key before
anything is allocated, the default builds no packed state, and the entries of pql_amd/csrc/fwd_bro_bf16.hip are bound from
include/pqlk.h."""
import ctypes as C

import pytest

from support import cfg_of

KEY = "algo.critic_target_dtype"
BRO, FUSED = "algo.cri_class=DoubleQBroNet", "algo.bronet_fused_forward=True"


@pytest.mark.parametrize("extra, names", [((BRO, FUSED, f"{KEY}=float16"), KEY), ((BRO, "algo.bronet_fused_forward=False", f"{KEY}=bfloat16"), KEY),
                                          ((BRO, FUSED, "algo.critic_width=48", f"{KEY}=bfloat16"), "algo.")],
                         ids=["bad_value", "not_fused", "width_48"])
def test_refusals_name_the_key(extra, names):
    from pql_amd.algo.critics import check_critic_class
    with pytest.raises(ValueError, match=names.replace(".", r"\.")):
        check_critic_class(cfg_of("ddpg_algo", *extra), agent=True)


def test_the_key_is_accepted_and_the_default_builds_no_packed_state():
    from pql_amd.algo.critics import check_critic_class, structure_keys
    from pql_amd.models.bronet import DoubleQBroNet
    cfg = cfg_of("ddpg_algo", BRO, FUSED, f"{KEY}=bfloat16")
    check_critic_class(cfg, agent=True)
    assert KEY not in structure_keys(cfg.algo)
    plain = DoubleQBroNet((8,), 2, 64, 1, fused_forward=True)
    on = DoubleQBroNet((8,), 2, 64, 1, fused_forward=True, target_dtype="bfloat16")
    assert plain.packed is None and not list(plain.buffers()) and on.packed.dtype.itemsize == 2
    assert on.packed.numel() == 2 * (64 * 16 + 2 * 64 * 64 + 64)   # per net: the stem (64, 10 -> 16), two (64, 64), the 64 output weights
    assert plain.init_kwargs == on.init_kwargs == dict(state_dim=8, act_dim=2, width=64, blocks=1)
    assert on.state_dict().keys() == plain.state_dict().keys()   # the packed copy is never saved
    with pytest.raises(ValueError, match=KEY.replace(".", r"\.")):
        plain.refresh()
    for bad in (dict(target_dtype="bfloat16"), dict(fused_forward=True, target_dtype="float16")):   # before anything is allocated
        with pytest.raises(ValueError, match=KEY.replace(".", r"\.")):
            DoubleQBroNet((8,), 2, 64, 1, **bad)
    with pytest.raises(ValueError):
        DoubleQBroNet((8,), 2, 48, 1, fused_forward=True, target_dtype="bfloat16")


def test_prototypes_come_out_of_the_header():
    from pql_amd import _lib as L
    P, I, I64 = C.c_void_p, C.c_int32, C.c_int64
    assert L.PROTOTYPES["pqlk_bro_bf16_ok"] == (C.c_int, [I, I, I, I]) and L.PROTOTYPES["pqlk_bro_packed_bf16_elems"] == (I64, [I, I, I, I])
    assert L.PROTOTYPES["pqlk_bro_pack_bf16"] == (C.c_int, [I, I, I, I, P, P, P])
    assert L.PROTOTYPES["pqlk_bro_forward_bf16"] == (C.c_int, [I, I, I, I, P, P, P, I64, I64, C.c_float, P, P])
