"""The campaign entry points' answers to calls that need no device, held against tests/golden/campaign_entry_errors.json: the return code
and madsim_hip_last_error() of every row of tools/campaign_entry_errors.py — one argument fault, two faults at once (which check runs
first), a NULL context, no contexts, an empty list without a context — for madsim_hip_X, madsim_hip_ctx_X and madsim_hip_X_multi of the ten
campaign operations.  The golden file was recorded from the library as it stood before the entry points were folded onto one body per
operation; no row's outcome depends on a device being present."""
import importlib.util
import json
import os

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


def _tool():
    spec = importlib.util.spec_from_file_location("campaign_entry_errors", os.path.join(HERE, "..", "tools", "campaign_entry_errors.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


TOOL = _tool()
GOLDEN = json.load(open(os.path.join(HERE, "golden", "campaign_entry_errors.json")))
ENTRY_POINTS = sorted(s for op in TOOL.OPS for s in ("madsim_hip_" + op, "madsim_hip_ctx_" + op, f"madsim_hip_{op}_multi"))


@pytest.fixture(scope="module")
def observed():
    return TOOL.observe()


def test_the_table_is_the_golden_files():
    assert sorted(row for row, *_ in TOOL.rows()) == sorted(GOLDEN)
    assert len(ENTRY_POINTS) == 30


@pytest.mark.parametrize("symbol", ENTRY_POINTS)
def test_entry_point_answers_as_recorded(observed, symbol):
    mine = {row: got for row, got in observed.items() if row.split(":")[0] == symbol}
    assert mine, symbol
    assert any("+" in row for row in mine), f"{symbol}: no row that combines two faults"
    for row, got in mine.items():
        assert got == GOLDEN[row], row


def test_default_context_rows_never_reach_a_context(observed):
    """The rows of a default-context spelling are told before any context is looked at, whatever this process has initialised."""
    for row, got in observed.items():
        if not row.startswith("madsim_hip_ctx_") and not row.split(":")[0].endswith("_multi"):
            assert got["rc"] == -1, row


def test_an_empty_list_needs_no_device_on_one_context_only(observed):
    """The single-context forms' rule: an empty list without a context is 0 with the reports of an empty range; a _multi call still asks for a context."""
    empty = {row: got for row, got in observed.items() if "empty_list+" in row or "nothing_to_run+" in row}
    assert len(empty) == 10
    for row, got in empty.items():
        if row.startswith("madsim_hip_ctx_"):
            assert got["rc"] == 0 and all(r == [0, 0, 0, (1 << 64) - 1, 0, 0, 0] for r in got["reports"]), row
        else:
            assert got["rc"] == -1 and got["error"].endswith("_multi needs at least one context"), row
