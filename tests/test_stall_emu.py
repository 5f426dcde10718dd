"""The trace builds' task log on a box without a GPU: the device code compiled for the host (tests/stall_emu) runs the directed workloads
of tests/stall_workloads.py — every seed must end with the hand-written table — and a slice of the traced lossy ping-pong against the
truth the oracle implies (tests/test_stall.py).  This checks the kernel's LOGIC: which word is written for which task, the panic record,
the pc of every awaiting op of all five trace builds, the cap guard and the empty row of a runner verdict.  tests/test_stall_gpu.py runs
the same cases through the product library on the device."""
import numpy as np
import pytest

import oracle
from madsim_amd import _abi as A
from tests import stall_emu
from tests import stall_ref as R
from tests import stall_workloads as SW
from tests import test_stall as T

SEEDS = list(range(1, 9)) + [70]                 # (nine seeds on a geometry of two emulated compute units: more than one lane, a second pass)


def run_case(case, seeds, task_cap=32):
    w, lim, verdict, want = case
    res, rows, lens = stall_emu.task_states(w, seeds, task_cap, limits=lim)
    ref = np.concatenate([oracle.run_batch(w, s, 1, limits=lim)[0] for s in seeds])
    assert res.tobytes() == ref.tobytes()
    for i, s in enumerate(seeds):
        got = [int(x) for x in rows[i]]
        assert int(res["verdict"][i]) == verdict and int(lens[i]) == len(want), (s, res[i], int(lens[i]))
        assert got == (want + [0] * task_cap)[:task_cap], (s, [(R.state(x), R.prog(x), R.pc(x), R.cnt0(x), R.cnt1(x)) for x in got])


@pytest.mark.parametrize("name", ["leak", "panic", "abort", "fused_assert", "assert_alone"])
def test_directed_small(name):
    case = {"leak": SW.leak, "panic": SW.panic, "abort": SW.abort, "fused_assert": SW.fused_assert, "assert_alone": lambda: SW.fused_assert(True)}[name]()
    run_case(case, SEEDS)
    run_case(case, SEEDS[:2], task_cap=1)                                          # the cap guard: the first record, the true count


@pytest.mark.parametrize("tier", SW.TIERS)
def test_one_task_parked_in_every_awaiting_op_under_a_time_limit(tier):
    case = SW.time_limit(tier)
    run_case(case, SW.time_limit_seeds(case[0], case[1], 6))


def test_a_crowd_around_a_cap_of_64():
    case = SW.crowd(64)
    run_case(case, [1, 2], task_cap=64)
    run_case(case, [1], task_cap=254)


def test_a_runner_verdict_leaves_an_empty_row():
    w, lim, _, want = SW.crowd(10)
    lim.max_tasks = 5                                                              # the sixth spawn finds no slot
    res, rows, lens = stall_emu.task_states(w, [1, 2], 16, limits=lim)
    assert (res["verdict"] == A.OVERFLOW).all() and not rows.any() and not lens.any()


def test_pingpong_slice_against_the_oracle_derived_truth():
    w, cfg, seeds, tables, verdicts, results, _ = T.pingpong_truth()
    dead = [i for i, v in enumerate(verdicts) if v == A.DEADLOCK]
    pick = dead[:24] + [0, 1, 2] + [i for i in dead if len(tables[i]) == 5][:2] + [i for i in dead if len(tables[i]) == 2][:2]
    res, rows, lens = stall_emu.task_states(w, [seeds[i] for i in pick], 8, config=cfg)
    for j, i in enumerate(pick):
        assert tuple(int(x) for x in res[j]) == results[i].astuple(), seeds[i]
        want = [R.word(*r) for r in tables[i]]
        assert int(lens[j]) == len(want) and [int(x) for x in rows[j]] == (want + [0] * 8)[:8], (seeds[i], tables[i])
