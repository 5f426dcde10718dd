"""The host planner answers what it answered when tests/golden/host_plan.json was recorded (tools/host_plan_record.py): validate's and
make_geometry's codes and messages, every scalar of Geo, the parameter block's bytes and the five device tables, over the corpus of
tests/host_plan_cases.py — accepted workloads through every layout, lane count, register budget and batch size, and single-field mutations of
small workloads for the refusals.  CPU only.

A change that is meant to alter an answer re-records the file and shows the difference in review; one that is not leaves the file alone."""
import json

import pytest

from tests import host_plan_cases as HP


@pytest.fixture(scope="module")
def replay():
    return HP.record()[0]


@pytest.fixture(scope="module")
def golden():
    with open(HP.GOLDEN) as f:
        return json.load(f)


def by_message(rec, tally):
    """{codes and messages in full: how many answers}"""
    return {rec["messages"][int(k)]: n for k, n in tally.items()}


def test_bench_cases_plan_as_recorded_field_by_field(replay, golden):
    assert list(replay["bench"]) == list(golden["bench"]) and len(golden["bench"]) == 5
    for name, want in golden["bench"].items():
        assert want["validate"][0] == 0 and want["geometry"][0] == 0 and set(want["geo"]) == set(HP.emu.GEO_SCALARS), name
        for field in want:
            assert replay["bench"][name][field] == want[field], (name, field)


def test_accepted_workloads_plan_as_recorded(replay, golden):
    got, want = replay["accepted"], golden["accepted"]
    assert list(got) == list(want), "the corpus itself changed: its entries or their order"
    for sec in golden["accepted_answers"]:
        assert by_message(replay, replay["accepted_answers"][sec]) == by_message(golden, golden["accepted_answers"][sec]), (sec, "other answers, or other numbers of them")
    for name, (members, stands, cross) in want.items():
        assert got[name][0] == members, (name, "members")
        assert got[name][1] == stands, (name, "as it stands: codes, messages, Geo, the parameter block or a device table")
        assert got[name][2] == cross, (name, "somewhere in the cross of layouts, lane counts, trace, register budgets and batch sizes")


def test_mutated_workloads_are_answered_as_recorded(replay, golden):
    assert list(replay["refused"]) == list(golden["refused"]), "the mutation bases changed"
    assert by_message(replay, replay["refused_answers"]) == by_message(golden, golden["refused_answers"]), "other answers, or other numbers of them"
    for base, (mutants, answers, plans) in golden["refused"].items():
        assert replay["refused"][base][0] == mutants, (base, "mutants")
        assert replay["refused"][base][1] == answers, (base, "a mutant is answered with another code or message")
        assert replay["refused"][base][2] == plans, (base, "an accepted mutant plans differently")
    assert replay["messages"] == golden["messages"]


def test_every_reachable_rule_is_in_the_record(golden):
    """Every message literal passed to fail( inside validate() and make_geometry() occurs in the record, but for the ones HP.UNREACHABLE
    lists with their reasons — so the record cannot leave a rule out silently."""
    lits = HP.fail_literals()
    assert len(lits["validate"]) >= 45 and len(lits["make_geometry"]) >= 12, "the header is no longer parsed"
    assert HP.uncovered(set(golden["messages"])) == []      # (code|message keys: a literal is a substring)
