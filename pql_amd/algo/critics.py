"""`TABLE`: THE place where a critic class's configuration rules are stated -- one `Rules` row per `algo.cri_class`; the functions below
are the engine over it, and the learners, the agents and pql_amd/utils/checkpoint.py ask them.  A new critic class is its model file and
one row here (and a head in pql_amd/algo/heads.py, the loss side's counterpart of this file, if its head is new)."""
from typing import NamedTuple

import torch

from pql_amd.models import model_name_to_path
from pql_amd.models.bronet import check_blocks, check_width
from pql_amd.models.droq import check_dropout
from pql_amd.models.mlp import check_num_atoms, check_num_quantiles
from pql_amd.replay.prioritized_replay import per_cfg, per_refresh
from pql_amd.utils.common import load_class_from_path

# A config key of a critic class: (algo.<key>, the default of a config without it, checker(value) or None, constructor argument or None).
# A null in the config goes to the checker like any other value.
HIDDEN = ("hidden_layers", None, None, "hidden_layers")


class Rules(NamedTuple):
    """What `algo.cri_class=<name>` may be combined with; the defaults are those of a class nothing is known about (PPO's value net)."""
    name: str
    no_distl: str = None        # why algo.distl=True is refused (None: accepted -- Distributional<name>, the C51 form, exists)
    fused: bool = True          # may run in a fused learner (PQLVLearner, PQLPLearner, scripts/train_pql.py)
    algos: str = None           # "the class is for ..."
    refuses: dict = {}          # {algo.name: why}; {algos} in it is the field above
    needed_by: dict = {}        # {algo.name: what its agent tells any other class}
    no_target_dtype: dict = {}  # {algo.target_dtype: why not}
    keys: tuple = (HIDDEN,)     # the class's keys, in the order they are checked
    structure: tuple = ()       # those that are part of a checkpoint's structure (0 for every other class and in an older checkpoint)


def check_huber_kappa(v):
    if v is None or not float(v) > 0.0:
        raise ValueError(f"algo.huber_kappa must be > 0, got {v!r}")


NO_CROSSQ = "CrossQ is the BatchNorm critic on joint batches, without a target critic; the class is for {algos}"
TABLE = {r.name: r for r in (
    Rules("DoubleQ"),   # (and DistributionalDoubleQ, its C51 form)
    Rules("QuantileDoubleQ", algos="algo=pql_algo and algo=ddpg_algo",
          no_distl="algo.distl selects the C51 head and the class the quantile head -- drop algo.distl=True to train the quantile critic",
          refuses={"SAC": "the entropy shift of the SAC target has no N-wide head; the class is for {algos} (the maximum-entropy agent on "
                          "this class is algo=tqc_algo)", "CrossQ": "the BatchNorm critic has no N-wide head; the class is for {algos}"},
          no_target_dtype={"bfloat16": "the bf16 target forward has not been taken to the quantile head (use algo.target_dtype=float32)"},
          keys=(("num_quantiles", 32, check_num_quantiles, "num_quantiles"), ("huber_kappa", 1.0, check_huber_kappa, None), HIDDEN),
          structure=("num_quantiles",)),   # (algo.qr_drop, whose range depends on num_quantiles, is checked behind the keys)
    Rules("DoubleQBatchNorm", "the BatchNorm critic has no C51 head", needed_by={"CrossQ": "CrossQ needs the BatchNorm critic"}),
    Rules("DoubleQLayerNorm", "the LayerNorm critic has no C51 head", fused=False, algos="algo=ddpg_algo / algo=sac_algo"),
    Rules("DoubleQDropoutLayerNorm", "the dropout LayerNorm critic has no C51 head", fused=False, refuses={"CrossQ": NO_CROSSQ},
          algos="algo=droq_algo / algo=sac_algo / algo=ddpg_algo", keys=(("critic_dropout", 0.01, check_dropout, "dropout"), HIDDEN)),
    Rules("DoubleQBroNet", "the residual LayerNorm critic has no C51 head", fused=False, refuses={"CrossQ": NO_CROSSQ},
          algos="algo=ddpg_algo / algo=sac_algo", structure=("critic_width", "critic_blocks"),   # (algo.hidden_layers stays the actor's)
          keys=(("critic_width", 512, check_width, "width"), ("critic_blocks", 2, check_blocks, "blocks"))),
)}
STRUCTURE_DEFAULTS = {f"algo.{key}": 0 for row in TABLE.values() for key in row.structure}


def critic_rules(algo):
    """The row of `algo.cri_class`; Distributional<name> (what `make_critic` leaves in the config when algo.distl is set) is <name>'s."""
    name = str(algo.get("cri_class")).removeprefix("Distributional")
    return TABLE.get(name) or Rules(name)


def check_target_dtype(algo, value):
    r = critic_rules(algo)
    if str(value) in r.no_target_dtype:
        raise ValueError(f"algo.target_dtype={value} is not supported with algo.cri_class={r.name}: {r.no_target_dtype[str(value)]}")


def check_critic_class(cfg, fused_learner=None, agent=False):
    """Refusals that follow from `algo.cri_class` (and, for the fused learners, `algo.per.enabled` with `algo.per.refresh`) alone, raised
    before anything is allocated.  fused_learner: the name of a component whose launch sequences are built on the fused MLP kernels
    (scripts/train_pql.py, PQLVLearner, PQLPLearner).  agent: the caller is the agent that runs `algo.name`'s update law."""
    algo = cfg.algo
    r, cri, name = critic_rules(algo), str(algo.get("cri_class")), str(algo.get("name") or "")
    if agent:
        for row in TABLE.values():
            if name in row.needed_by and cri != row.name:
                raise ValueError(f"{row.needed_by[name]}: algo.cri_class={row.name}, not {cri}")
    # ---- the rules in front of any class
    per = per_cfg(algo)
    if fused_learner is not None and per is not None and per_refresh(per) != "run":
        raise ValueError(f"algo.per.enabled=True cannot run in {fused_learner}: the PQL learners gather batches ahead and replay steps as one "
                         f"hipGraph, which assumes a sampling distribution that does not change between hand-offs; prioritized replay works "
                         f"in scripts/train_baselines.py (algo=ddpg_algo / sac_algo / crossq_algo), and in the PQL V-learner with "
                         f"algo.per.refresh=run (the distribution frozen for each run of prefetched steps)")
    drop, quantile = algo.get("qr_drop"), r.name == "QuantileDoubleQ"
    if name == "TQC":   # algo=tqc_algo is the quantile critic on the truncated soft target, nothing else
        if not quantile:
            raise ValueError(f"algo=tqc_algo needs algo.cri_class=QuantileDoubleQ (got algo.cri_class={cri}): its soft truncated target and "
                             f"its mean-of-critics actor loss are laws of the quantile heads; algo=sac_algo runs the scalar critics")
        if drop is None:
            raise ValueError("algo.qr_drop=null cannot run with algo=tqc_algo: the non-truncated soft quantile law (one whole target net "
                             "per row, shifted by the entropy term) is not built; set algo.qr_drop to an integer from 0 to "
                             "algo.num_quantiles - 1 (0 keeps every pooled atom)")
    if drop is not None and not quantile:
        raise ValueError(f"algo.qr_drop={drop!r} needs algo.cri_class=QuantileDoubleQ (got algo.cri_class={cri}): it truncates the pooled "
                         f"target atoms of the quantile critic; leave algo.qr_drop null with any other critic")
    # (algo.distl_loss, algo.hl_sigma: which law trains the C51 head's logits -- the loss launch alone, so neither a row's key nor a
    # constructor argument nor a checkpoint's structure)
    loss, sigma = algo.get("distl_loss", "c51"), algo.get("hl_sigma", 0.75)
    if loss not in ("c51", "hl_gauss"):
        raise ValueError(f"algo.distl_loss must be c51 or hl_gauss, got {loss!r}")
    if loss == "hl_gauss":
        if not algo.get("distl"):
            raise ValueError(f"algo.distl_loss=hl_gauss needs algo.distl=True (got algo.distl={algo.get('distl')!r}): HL-Gauss is a loss of "
                             f"the categorical head; leave algo.distl_loss=c51 with a scalar or quantile critic")
        if name not in ("PQL", "DDPG"):
            raise ValueError(f"algo.distl_loss=hl_gauss cannot run with algo.name={name}: the HL-Gauss loss is built for algo=pql_algo and "
                             f"algo=ddpg_algo (its target carries no entropy term and no joint-batch statistics)")
    if isinstance(sigma, bool) or not isinstance(sigma, (int, float)) or not float(sigma) > 0.0:
        raise ValueError(f"algo.hl_sigma must be > 0 (sigma of the HL-Gauss target in bin widths), got {sigma!r}")
    # ---- the class's row
    where = f"algo.cri_class={r.name}"
    if algo.get("distl") and r.no_distl:
        raise ValueError(f"algo.distl=True is not supported with {where}: {r.no_distl}")
    if fused_learner is not None and not r.fused:
        raise ValueError(f"{where} cannot run in {fused_learner}, whose launch sequences are built on the fused MLP kernels: the class is "
                         f"for {r.algos} (scripts/train_baselines.py)")
    if name in r.refuses:
        raise ValueError(f"{where} cannot run with algo={name.lower()}_algo: {r.refuses[name].format(algos=r.algos)}")
    check_target_dtype(algo, algo.get("target_dtype") or "float32")
    for key, default, check, _ in r.keys:
        if check is not None:
            check(algo.get(key, default))
    n = int(algo.get("num_quantiles") or 0)
    if drop is not None and not (isinstance(drop, (int, float)) and not isinstance(drop, bool) and int(drop) == drop and 0 <= int(drop) <= n - 1):
        raise ValueError(f"algo.qr_drop must be null or an integer from 0 to algo.num_quantiles - 1 = {n - 1} (the atoms dropped "
                         f"per target net; at least one per net is kept), got {drop!r}")


def make_critic(cfg, obs_dim, action_dim, device):
    """The critic `cfg.algo` names, freshly initialised on `device` (consumes the CPU generator like any module constructor)."""
    algo = cfg.algo
    check_critic_class(cfg)
    kwargs = {arg: algo.get(key, default) for key, default, _, arg in critic_rules(algo).keys if arg}   # (the constructors check them again)
    distl = algo.get("distl")   # (the baselines' configs need not carry the key)
    if distl and "Distributional" not in algo.cri_class:
        algo.cri_class = "Distributional" + algo.cri_class  # same rewrite as the reference (:30-31)
    cri_class = load_class_from_path(algo.cri_class, model_name_to_path[algo.cri_class])
    if distl:
        check_num_atoms(algo.num_atoms)   # before anything is allocated: a wrong value fails here, not after the warm-up rollout
        kwargs.update(v_min=algo.v_min, v_max=algo.v_max, num_atoms=algo.num_atoms, device=device)
    with torch.cuda.device(device):
        return cri_class(obs_dim, action_dim, **kwargs).to(device)


def structure_keys(algo):
    """A checkpoint's per-class structure keys: the class's own from the config, the others at what a checkpoint from before them is read with."""
    return {**STRUCTURE_DEFAULTS, **{f"algo.{key}": int(algo.get(key) or 0) for key in critic_rules(algo).structure}}
