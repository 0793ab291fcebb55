"""`algo.critic_fused_backward` without a GPU: what is refused names the key, and the default builds a critic with the switch off."""
import pytest

from support import cfg_of

KEY = "algo.critic_fused_backward"
LN = "algo.cri_class=DoubleQLayerNorm"
FWD = "algo.critic_fused_forward=True"


@pytest.mark.parametrize("extra", [(LN, f"{KEY}=True"), ("algo.cri_class=DoubleQDropoutLayerNorm", "algo.droq_fused_forward=True", f"{KEY}=True"),
                                   ("algo.cri_class=DoubleQBroNet", f"{KEY}=True"), (f"{KEY}=True",), (LN, FWD, f"{KEY}=2")],
                         ids=["no_fused_forward", "DroQ", "BroNet", "DoubleQ", "not_bool"])
def test_refusals_name_the_key(extra):
    from pql_amd.algo.critics import check_critic_class
    with pytest.raises(ValueError, match=KEY.replace(".", r"\.")):
        check_critic_class(cfg_of("ddpg_algo", *extra), agent=True)


def test_the_constructors_refuse_and_name_the_key():
    from pql_amd.models.droq import DoubleQDropoutLayerNorm
    from pql_amd.models.layernorm import DoubleQLayerNorm
    with pytest.raises(ValueError, match=r"algo\.critic_fused_backward=True needs algo\.critic_fused_forward=True"):
        DoubleQLayerNorm((8,), 2, [64, 32], fused_backward=True)
    with pytest.raises(ValueError, match=r"algo\.critic_fused_backward"):
        DoubleQDropoutLayerNorm((8,), 2, [64, 32], fused_forward=True, fused_backward=True)


def test_default_builds_the_switch_off():
    from pql_amd.algo.critics import check_critic_class, critic_rules, structure_keys
    from pql_amd.models.layernorm import DoubleQLayerNorm
    cfg = cfg_of("ddpg_algo", LN)
    check_critic_class(cfg, agent=True)
    assert cfg.algo.critic_fused_backward is False and KEY not in structure_keys(cfg.algo)
    kwargs = {arg: cfg.algo.get(key, default) for key, default, _, arg in critic_rules(cfg.algo).keys if arg}   # what make_critic passes
    q = DoubleQLayerNorm((8,), 2, **kwargs)
    assert kwargs["fused_backward"] is False and q.fused_backward_on is False and "fused_backward" not in q.init_kwargs
    assert DoubleQLayerNorm((8,), 2, [64, 32], fused_forward=True, fused_backward=True).fused_backward_on is True
