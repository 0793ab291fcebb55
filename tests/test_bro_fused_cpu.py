"""`algo.bronet_fused_forward` without a GPU: what is refused names the key, the default builds no fused state, and the entries of
pql_amd/csrc/fwd_bro.hip are bound from include/pqlk.h."""
import ctypes as C

import pytest

from support import cfg_of

KEY = "algo.bronet_fused_forward"
BRO = "algo.cri_class=DoubleQBroNet"


@pytest.mark.parametrize("extra", [(f"{KEY}=True",), ("algo.cri_class=DoubleQLayerNorm", f"{KEY}=True"),
                                   (BRO, f"{KEY}=True", "algo.critic_width=48"), (BRO, f"{KEY}=2")],
                         ids=["DoubleQ", "LayerNorm", "width48", "not_bool"])
def test_refusals_name_the_key(extra):
    from pql_amd.algo.critics import check_critic_class
    with pytest.raises(ValueError, match=KEY.replace(".", r"\.")):
        check_critic_class(cfg_of("ddpg_algo", *extra), agent=True)


def test_constructor_refuses_before_it_allocates():
    from pql_amd.models.bronet import DoubleQBroNet
    with pytest.raises(ValueError, match=KEY.replace(".", r"\.")):
        DoubleQBroNet((1300,), 2, 64, 1, fused_forward=True)   # an input wider than the LDS image


def test_default_builds_no_fused_state():
    from pql_amd.algo.critics import check_critic_class, structure_keys
    from pql_amd.models.bronet import DoubleQBroNet
    cfg = cfg_of("ddpg_algo", BRO)
    check_critic_class(cfg, agent=True)
    assert cfg.algo.bronet_fused_forward is False and KEY not in structure_keys(cfg.algo)
    q = DoubleQBroNet((8,), 2, 64, 1)
    assert q.fused is None and q.init_kwargs == dict(state_dim=8, act_dim=2, width=64, blocks=1)
    with pytest.raises(ValueError, match=KEY.replace(".", r"\.")):
        q.forward_raw(None, stash=False)
    on = DoubleQBroNet((8,), 2, 64, 1, fused_forward=True)   # (asserts the library's arena law against the module's own)
    assert on.fused == (10, 64, 1, 2) and on.init_kwargs == q.init_kwargs and on.state_dict().keys() == q.state_dict().keys()
    check_critic_class(cfg_of("ddpg_algo", BRO, f"{KEY}=True", "algo.critic_width=1024", "algo.critic_blocks=16"), agent=True)


def test_eligibility_and_prototypes_come_out_of_the_header():
    from pql_amd import _lib as L
    P, I32, I64 = C.c_void_p, C.c_int32, C.c_int64
    assert L.lib.pqlk_bro_ok(40, 64, 16, 2) == 1 and L.lib.pqlk_bro_ok(40, 64, 17, 2) == 0
    assert L.lib.pqlk_bro_param_floats(40, 64, 17, 2) == 0 and L.lib.pqlk_bro_stash_floats(64, 17, 2, 4) == 0
    assert L.PROTOTYPES["pqlk_bro_ok"] == (C.c_int, [I32] * 4) and L.PROTOTYPES["pqlk_bro_param_floats"] == (I64, [I32] * 4)
    assert L.PROTOTYPES["pqlk_bro_offsets"] == (C.c_int, [I32] * 4 + [P] * 3)
    assert L.PROTOTYPES["pqlk_bro_stash_floats"] == (I64, [I32] * 3 + [I64])
    assert L.PROTOTYPES["pqlk_bro_stash_offset"] == (C.c_int, [I32] * 3 + [I64] + [I32] * 3 + [P] * 2)
    assert L.PROTOTYPES["pqlk_bro_forward"] == (C.c_int, [I32] * 4 + [P, P, I64, I64, C.c_float, P, P, P])
