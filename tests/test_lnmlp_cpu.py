"""`algo.critic_fused_forward` without a GPU: what is refused names the key, the default builds no fused state, and the entries of
pql_amd/csrc/fwd_ln.hip are bound from include/pqlk.h."""
import ctypes as C

import pytest

from support import cfg_of

KEY = "algo.critic_fused_forward"
LN = "algo.cri_class=DoubleQLayerNorm"


@pytest.mark.parametrize("extra", [(f"{KEY}=True",), ("algo.cri_class=DoubleQDropoutLayerNorm", f"{KEY}=True"),
                                   ("algo.cri_class=DoubleQBroNet", f"{KEY}=True"), (LN, f"{KEY}=True", "algo.hidden_layers=[64,48]"),
                                   (LN, f"{KEY}=True", "algo.hidden_layers=[1056]"), (LN, f"{KEY}=True", "algo.hidden_layers=[]"),
                                   (LN, f"{KEY}=2")],
                         ids=["DoubleQ", "DroQ", "BroNet", "width48", "width1056", "no_hidden", "not_bool"])
def test_refusals_name_the_key(extra):
    from pql_amd.algo.critics import check_critic_class
    with pytest.raises(ValueError, match=KEY.replace(".", r"\.")):
        check_critic_class(cfg_of("ddpg_algo", *extra), agent=True)


def test_constructor_refuses_before_it_allocates():
    from pql_amd.models.layernorm import DoubleQLayerNorm
    with pytest.raises(ValueError, match=KEY.replace(".", r"\.")):
        DoubleQLayerNorm((1300,), 2, [64], fused_forward=True)   # an input wider than the LDS image


def test_default_builds_no_fused_state():
    from pql_amd.algo.critics import check_critic_class, critic_rules, structure_keys
    from pql_amd.models.layernorm import DoubleQLayerNorm
    cfg = cfg_of("ddpg_algo", LN)
    check_critic_class(cfg, agent=True)
    assert cfg.algo.critic_fused_forward is False and "algo.critic_fused_forward" not in structure_keys(cfg.algo)
    assert ("critic_fused_forward", False) == critic_rules(cfg.algo).keys[1][:2]
    q = DoubleQLayerNorm((8,), 2, [64, 32])
    assert q.fused is None and "fused_forward" not in q.init_kwargs
    with pytest.raises(ValueError, match=KEY.replace(".", r"\.")):
        q.forward_raw(None, stash=False)
    on = DoubleQLayerNorm((8,), 2, [64, 32], fused_forward=True)
    assert on.fused is not None and on.state_dict().keys() == q.state_dict().keys()


def test_prototypes_come_out_of_the_header():
    from pql_amd import _lib as L
    PD, P, I32, I64 = C.POINTER(L.PqlMlpDesc), C.c_void_p, C.c_int32, C.c_int64
    assert L.PROTOTYPES["pqlk_lnmlp_ok"] == (C.c_int, [PD]) and L.PROTOTYPES["pqlk_lnmlp_stash_floats"] == (I64, [PD, I64])
    assert L.PROTOTYPES["pqlk_lnmlp_param_floats"] == (I64, [PD]) and L.PROTOTYPES["pqlk_lnmlp_offsets"] == (C.c_int, [PD, I32, P, P, P])
    assert L.PROTOTYPES["pqlk_lnmlp_stash_offset"] == (C.c_int, [PD, I64, I32, I32, I32, P, P])
    assert L.PROTOTYPES["pqlk_lnmlp_forward"] == (C.c_int, [PD, P, P, I64, I64, C.c_float, P, P, P])
    assert (L.LNMLP_Z, L.LNMLP_Y, L.LNMLP_MEAN, L.LNMLP_RSTD) == (0, 1, 2, 3)
