"""`algo.critic_target_dtype` without a GPU: what is refused names the key, the default builds no packed state, and the entries of
pql_amd/csrc/fwd_ln_bf16.hip are bound from include/pqlk.h."""
import ctypes as C

import pytest

from support import cfg_of

KEY = "algo.critic_target_dtype"
LN, FUSED = "algo.cri_class=DoubleQLayerNorm", "algo.critic_fused_forward=True"


@pytest.mark.parametrize("extra", [(LN, FUSED, f"{KEY}=float16"), (LN, "algo.critic_fused_forward=False", f"{KEY}=bfloat16"),
                                   ("algo.cri_class=DoubleQBroNet", f"{KEY}=bfloat16"),
                                   ("algo.cri_class=DoubleQDropoutLayerNorm", f"{KEY}=bfloat16"), (f"{KEY}=bfloat16",)],
                         ids=["bad_value", "not_fused", "BroNet", "DroQ", "DoubleQ"])
def test_refusals_name_the_key(extra):
    from pql_amd.algo.critics import check_critic_class
    with pytest.raises(ValueError, match=KEY.replace(".", r"\.")):
        check_critic_class(cfg_of("ddpg_algo", *extra), agent=True)


def test_default_builds_no_packed_state():
    from pql_amd.algo.critics import check_critic_class, structure_keys
    from pql_amd.models.layernorm import DoubleQLayerNorm
    cfg, plain = cfg_of("ddpg_algo", LN, FUSED), DoubleQLayerNorm((8,), 2, [64, 32], fused_forward=True)
    check_critic_class(cfg, agent=True)
    assert cfg.algo.critic_target_dtype == "float32" and KEY not in structure_keys(cfg.algo)
    on = DoubleQLayerNorm((8,), 2, [64, 32], fused_forward=True, target_dtype="bfloat16")
    assert plain.packed is None and not list(plain.buffers()) and on.packed.dtype.itemsize == 2
    assert on.packed.numel() == 2 * (64 * 16 + 32 * 64 + 32)   # per net: (64, 10 -> 16), (32, 64), the 32 output weights
    assert plain.init_kwargs == on.init_kwargs == dict(state_dim=8, act_dim=2, hidden_layers=[64, 32])
    assert on.state_dict().keys() == plain.state_dict().keys()   # the packed copy is never saved
    with pytest.raises(ValueError, match=KEY.replace(".", r"\.")):
        plain.refresh()
    with pytest.raises(ValueError, match=KEY.replace(".", r"\.")):
        DoubleQLayerNorm((8,), 2, [64, 32], target_dtype="bfloat16")   # not fused: refused before anything is allocated


def test_prototypes_come_out_of_the_header():
    from pql_amd import _lib as L
    PD, P, I64 = C.POINTER(L.PqlMlpDesc), C.c_void_p, C.c_int64
    assert L.PROTOTYPES["pqlk_lnmlp_bf16_ok"] == (C.c_int, [PD]) and L.PROTOTYPES["pqlk_lnmlp_packed_bf16_elems"] == (I64, [PD])
    assert L.PROTOTYPES["pqlk_lnmlp_pack_bf16"] == (C.c_int, [PD, P, P, P])
    assert L.PROTOTYPES["pqlk_lnmlp_forward_bf16"] == (C.c_int, [PD, P, P, P, I64, I64, C.c_float, P, P])
