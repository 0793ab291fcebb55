"""`algo.droq_fused_forward` without a GPU: refusals name their key, the default builds nothing new, the two entries reach the binding."""
import ctypes as C

import pytest

from support import cfg_of

KEY, TDT = "algo.droq_fused_forward", "algo.critic_target_dtype"
DROQ = "algo.cri_class=DoubleQDropoutLayerNorm"


@pytest.mark.parametrize("extra, key", [
    ((f"{KEY}=True",), KEY), (("algo.cri_class=DoubleQLayerNorm", f"{KEY}=True"), KEY), (("algo.cri_class=DoubleQBroNet", f"{KEY}=True"), KEY),
    ((DROQ, f"{KEY}=2"), KEY), ((f"{KEY}=2",), KEY), ((DROQ, f"{KEY}=True", "algo.hidden_layers=[64,48]"), KEY),
    ((DROQ, f"{KEY}=True", "algo.hidden_layers=[1056]"), KEY), ((DROQ, f"{TDT}=bfloat16"), TDT), ((DROQ, f"{KEY}=True", f"{TDT}=float16"), TDT)],
    ids=["DoubleQ", "LayerNorm", "BroNet", "not_bool", "not_bool_other_class", "width48", "width1056", "bf16_not_fused", "bad_dtype"])
def test_refusals_name_the_key(extra, key):
    from pql_amd.algo.critics import check_critic_class
    with pytest.raises(ValueError, match=key.replace(".", r"\.")):
        check_critic_class(cfg_of("ddpg_algo", *extra), agent=True)


def test_accepted_settings_and_the_default():
    from pql_amd.algo.critics import check_critic_class, critic_rules
    from pql_amd.models.droq import DoubleQDropoutLayerNorm
    built = []
    for extra in ((), (f"{KEY}=True",), (f"{KEY}=True", f"{TDT}=bfloat16")):
        cfg = cfg_of("droq_algo", "algo.hidden_layers=[64,32]", *extra)
        check_critic_class(cfg, agent=True)
        kwargs = {arg: cfg.algo.get(key, default) for key, default, _, arg in critic_rules(cfg.algo).keys if arg}   # what make_critic passes
        built.append(DoubleQDropoutLayerNorm((8,), 2, **kwargs))
    q, f, b = built
    assert cfg_of("droq_algo").algo.droq_fused_forward is False and q.fused is None and q.packed is None   # no fused or packed state
    assert f.fused is not None and f.packed is None and b.fused is not None and b.packed is not None
    assert q.init_kwargs == b.init_kwargs == dict(state_dim=8, act_dim=2, hidden_layers=[64, 32]) and list(q.state_dict()) == list(b.state_dict())


def test_the_prototypes_come_out_of_the_header():
    from pql_amd import _lib as L
    fp32, bf16 = L.lib.pqlk_lnmlp_drop_forward, L.lib.pqlk_lnmlp_drop_forward_bf16
    assert fp32.restype is C.c_int and bf16.restype is C.c_int
    assert [fp32.argtypes[i] for i in (6, 7, 8)] == [bf16.argtypes[i] for i in (7, 8, 9)] == [C.c_float, C.c_uint64, C.c_uint64]
    assert len(fp32.argtypes) == len(bf16.argtypes) == 12
