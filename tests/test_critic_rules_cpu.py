"""The rules of `algo.cri_class` (pql_amd/algo/critics.py) against tests/golden/critic_rules.json, the outcomes of every case of
tests/critic_rule_cases.py as recorded before the rules were one table: accepted or refused, the exception type and the WHOLE message,
what `make_critic` builds and what `checkpoint.structure` returns.  The cases under "changed_on_purpose" (a bare KeyError out of the
plugin lookup then, a ValueError naming the keys now) are held to their new rows; every other case to the recorded one."""
import pytest

import critic_rule_cases as crc


@pytest.fixture(scope="module")
def golden_rules():
    return crc.load()


@pytest.fixture(scope="module")
def fresh():
    return crc.record()   # (the whole table once, on the working tree)


def _outcomes(rec, row):
    return [rec["outcomes"][i] for i in row]


def test_the_file_covers_the_case_table(golden_rules):
    keys = [crc.key(a, c, ov) for a in crc.ALGOS for c in crc.CLASSES for ov in crc.OVERRIDES]
    assert list(golden_rules["cases"]) == keys and golden_rules["fused"] == list(crc.FUSED)
    lookup = {"error": "KeyError", "message": "'DistributionalDoubleQBatchNorm'"}
    for k, row in golden_rules["changed_on_purpose"].items():   # only the bare plugin-lookup KeyError may change, and into a ValueError
        old, new = _outcomes(golden_rules, golden_rules["cases"][k]), _outcomes(golden_rules, row)
        assert old[1] == lookup and new[0] == old[0], k   # (the structure is as recorded)
        assert all(o["error"] == "ValueError" and "algo.distl=True is not supported with algo.cri_class=" in o["message"] for o in new[1:]), k


@pytest.mark.parametrize("cls", crc.CLASSES)
@pytest.mark.parametrize("algo", crc.ALGOS)
def test_every_case_is_as_recorded(algo, cls, golden_rules, fresh):
    wrong = []
    for ov in crc.OVERRIDES:
        k = crc.key(algo, cls, ov)
        got = _outcomes(fresh, fresh["cases"][k])
        want = _outcomes(golden_rules, golden_rules["changed_on_purpose"].get(k, golden_rules["cases"][k]))
        wrong += [(k, part, g, w) for part, g, w in zip(("structure", "make", *map(str, crc.FUSED)), got, want) if g != w]
    assert not wrong, "\n".join(f"{k} [{part}]\n  got  {g}\n  want {w}" for k, part, g, w in wrong)


def test_a_fresh_recording_is_the_file_but_for_the_marked_cases(golden_rules, fresh):
    """Byte for byte: the text of `dump(record())` against the text of the file's recorded part, line by line."""
    with open(crc.GOLDEN) as f:
        assert f.read() == crc.dump(golden_rules, golden_rules["changed_on_purpose"])
    then = dict(golden_rules, outcomes=golden_rules["outcomes"][:-1])   # (the file's last outcome is the one the marked cases reached)
    a, b = crc.dump(then).split("\n"), crc.dump(fresh).split("\n")
    differ = [(x, y) for x, y in zip(a, b) if x != y]
    marked = tuple(crc.json.dumps(k) + ":" for k in golden_rules["changed_on_purpose"])
    assert len(a) == len(b) and len(marked) == 15
    assert [x for x, _ in differ if x.startswith('"')] == [x for x in a if x.startswith(marked)]   # case lines: the marked ones, no other
    assert [(x, y) for x, y in differ if not x.startswith('"')] == [   # outcome lines: the one the marked cases left -> the one they reached
        ('{"error": "KeyError", "message": "\'DistributionalDoubleQBatchNorm\'"},', crc.json.dumps(golden_rules["outcomes"][-1], sort_keys=True) + ",")]


def test_the_agent_path_holds_the_need_of_crossq():
    """What moved out of AgentCrossQ: under algo=crossq_algo the agent (`agent=True`, ActorCriticBase) refuses every class but the
    BatchNorm critic, first and with the message it had; a call that is not the agent's keeps the recorded outcomes above."""
    from pql_amd.algo.crossq import AgentCrossQ
    from pql_amd.algo.critics import check_critic_class
    for cls in crc.CLASSES:
        cfg = crc._cfg("crossq_algo", cls, ())
        if cls == "DoubleQBatchNorm":
            check_critic_class(cfg, agent=True)
            continue
        for make in (lambda: check_critic_class(cfg, agent=True), lambda: AgentCrossQ(None, cfg)):
            with pytest.raises(ValueError) as e:
                make()
            assert str(e.value) == f"CrossQ needs the BatchNorm critic: algo.cri_class=DoubleQBatchNorm, not {cls}"
    for algo in ("ddpg_algo", "sac_algo"):   # (no other algo's agent has such a need)
        check_critic_class(crc._cfg(algo, "DoubleQLayerNorm", ()), agent=True)
