"""The whole rule set of `algo.cri_class`, as a case table and its recorded outcomes (tests/golden/critic_rules.json).

A case is (algo config, cri_class, fused_learner, one override set).  `record()` runs every case through `check_critic_class`, and for
fused_learner=None through `make_critic` on the CPU, and through `checkpoint.structure`; `dump()` is the file's text.  The file was
recorded on the commit before pql_amd/algo/critics.py existed, with `record(check_critic_class, make_critic)` of that commit's
pql_amd.algo.learner: it pins what the scattered rules did, full messages included.  tests/test_critic_rules_cpu.py holds the tree to it.
"""
import contextlib
import json
import os

import torch

ALGOS = ("pql_algo", "ddpg_algo", "sac_algo", "crossq_algo", "tqc_algo", "droq_algo")
CLASSES = ("DoubleQ", "QuantileDoubleQ", "DoubleQBatchNorm", "DoubleQLayerNorm", "DoubleQDropoutLayerNorm", "DoubleQBroNet")
FUSED = (None, "PQLVLearner", "PQLPLearner", "scripts/train_pql.py")
OVERRIDES = (
    (),
    ("algo.distl=True",),
    ("algo.qr_drop=2",),
    ("algo.qr_drop=-1",),
    ("algo.qr_drop=32",),            # = algo.num_quantiles (every config's default)
    ("algo.qr_drop=null",),
    ("algo.num_quantiles=1",),
    ("algo.num_quantiles=65",),
    ("algo.huber_kappa=0",),
    ("algo.target_dtype=bfloat16",),
    ("algo.per.enabled=True",),
    ("algo.per.enabled=True", "algo.per.refresh=run"),
    ("algo.critic_dropout=1.0",),
    ("algo.critic_width=0",),
    ("algo.critic_blocks=17",),
    ("algo.distl=True", "algo.num_atoms=1"),
    ("algo.distl=True", "algo.num_atoms=257"),
)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "critic_rules.json")


def key(algo, cls, overrides):
    return "|".join((algo, cls, " ".join(overrides)))


def _cfg(algo, cls, overrides):
    from pql_amd.utils.cfg import load_cfg
    return load_cfg([f"algo={algo}", "task.name=Toy", "num_envs=4", f"algo.cri_class={cls}", *overrides])


def _outcome(fn):
    try:
        return json.loads(json.dumps(fn()))   # (as it reads out of the file: tuples are lists there)
    except Exception as e:   # noqa: BLE001  (the type and the whole message ARE the record)
        return {"error": type(e).__name__, "message": str(e)}


@contextlib.contextmanager
def _no_device_switch():
    """`make_critic` selects the device it builds on; there is none here."""
    real = torch.cuda.device
    torch.cuda.device = lambda d: contextlib.nullcontext()
    try:
        yield
    finally:
        torch.cuda.device = real


def run_group(check_critic_class, make_critic, algo, cls):
    """{case key: {"check": [outcome per FUSED], "make": outcome, "structure": outcome}} of one (algo config, cri_class)."""
    from pql_amd.utils import checkpoint as CK
    out = {}
    for ov in OVERRIDES:
        try:
            cfg = _cfg(algo, cls, ov)
        except Exception as e:   # noqa: BLE001  (a config that lacks the key: the same for every part of the case)
            bad = {"error": type(e).__name__, "message": str(e), "where": "load_cfg"}
            out[key(algo, cls, ov)] = {"check": [bad] * len(FUSED), "make": bad, "structure": bad}
            continue

        def make():
            critic = make_critic(cfg, (8,), 2, torch.device("cpu"))
            return {"class": type(critic).__name__, "init_kwargs": critic.init_kwargs, "num_params": int(critic.num_params()),
                    "cri_class": str(cfg.algo.cri_class)}   # (as it reads afterwards: the Distributional rewrite is behaviour)

        case = {"check": [_outcome(lambda: check_critic_class(cfg, f) or "ok") for f in FUSED],
                "structure": _outcome(lambda: CK.structure(cfg, 8, 2))}
        with _no_device_switch():
            case["make"] = _outcome(make)   # last: it rewrites cfg.algo.cri_class
        out[key(algo, cls, ov)] = case
    return out


def record(check_critic_class=None, make_critic=None):
    """Every case's outcomes, each distinct outcome stored once: {"outcomes": [...], "cases": {key: [structure, make, check x 4]}}."""
    if check_critic_class is None:
        from pql_amd.algo.critics import check_critic_class, make_critic
    outcomes, ids, cases = [], {}, {}

    def oid(o):
        text = json.dumps(o, sort_keys=True)
        if text not in ids:
            ids[text] = len(outcomes)
            outcomes.append(o)
        return ids[text]

    for algo in ALGOS:
        for cls in CLASSES:
            for k, case in run_group(check_critic_class, make_critic, algo, cls).items():
                cases[k] = [oid(case["structure"]), oid(case["make"]), *(oid(c) for c in case["check"])]
    return {"outcomes": outcomes, "cases": cases}


def dump(rec, changed=None):
    """The file's text: one outcome and one case per line.  changed: {case key: its row after the change}, the cases whose outcome
    was changed on purpose (the recorded row stays under "cases")."""
    one = lambda v: json.dumps(v, sort_keys=True)  # noqa: E731
    lines = ["{", '"fused": ' + one(list(FUSED)) + ",", '"row": ["structure", "make", "check per fused"],', '"outcomes": [']
    lines += [one(o) + ("," if i + 1 < len(rec["outcomes"]) else "") for i, o in enumerate(rec["outcomes"])]
    for name, table in (("cases", rec["cases"]), ("changed_on_purpose", changed or {})):
        lines += ["]," if name == "cases" else "},", f'"{name}": {{']
        lines += [f"{one(k)}: {one(v)}" + ("," if i + 1 < len(table) else "") for i, (k, v) in enumerate(table.items())]
    lines += ["}", "}"]
    return "\n".join(lines) + "\n"


def load():
    with open(GOLDEN) as f:
        return json.load(f)
