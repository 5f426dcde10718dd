"""The timer heap at every LDS / spill boundary under tied deadlines, on the host-compiled kernels (tests/emu): the matrix of
tests/heap_cases.py — every layout, workload and quota, 130 seeds each on all 48 result bytes — where MADSIM_INTERNAL also flags a mirror
the kernel keeps beside the heap (the root's deadline, the de-duplication table's occupancy word) that went out of step.  Beside it the
premises the matrix rests on: which build each layout's limits select, that the workloads' deadlines do tie and their heaps reach the
depth they are named for (the oracle's heap counters), and that the oracle they are compared with agrees with the generator restatement
of tests/golden/make_golden_async.py.

What these cases see and the fuzz suites do not: tools/heap_mutants.py, profiles/heap_boundaries.md."""
import importlib.util
import os

import numpy as np
import pytest

import oracle
from madsim_amd import _abi as A
from tests import emu
from tests import heap_cases as H

FIELDS = ("verdict", "steps", "clock_ns", "msg_count", "rng_calls", "trace_hash", "obs_hash")


@pytest.mark.parametrize("layout", list(H.LAYOUTS))
def test_layout_selects_its_build(layout):
    """Every case of a layout — each workload at each quota — runs on the build the layout names, in the library and in the emulation."""
    n = 0
    for _, w, _, lim in H.cases(layout):
        H.check_variant(layout, w, lim, emu)
        n += 1
    assert n >= 2


def test_layouts_cover_the_builds_with_a_heap_path_of_their_own():
    names = {lay.variant for lay in H.LAYOUTS.values()}
    assert len(names) == 17, sorted(names)
    # the two run-time switches of one build each are layouts of their own
    assert sum(lay.dedup for lay in H.LAYOUTS.values()) == 4 and sum(lay.narrow for lay in H.LAYOUTS.values()) == 5


@pytest.mark.parametrize("layout", list(H.LAYOUTS))
def test_heap_boundaries_emu(layout):
    H.run_layout(layout, emu.run_batch, lambda w, lim: emu.geometry(w, lim).heap_lds_slots)


def test_trace_build_emu():
    """The trace build's raw determinism log, byte for byte against the oracle's."""
    w = H.workload(H.TRACE_KEY)
    for q in H.TRACE_QUOTAS:
        lim = H.quota_limits(H.TRACE_KEY[1], q)
        for i, (log, res) in enumerate(H.trace_truth(q)):
            got_log, got = emu.trace_seed(w, H.SEED0 + i, None, lim)
            assert res[0] == A.PASS and tuple(int(x) for x in got) == res, (q, i, got, res)
            assert got_log == log, (q, i, len(got_log), len(log))


@pytest.mark.parametrize("key", [k for k in H.all_keys() if k[0] == "lockstep"], ids=str)
def test_lockstep_premises(key):
    """The deadlines tie in at least a third of the seeds, the heap reaches n entries in every seed, every heap length is popped every round,
    and every seed passes."""
    _, n, rounds, _ = key
    st = H.stats_by_seed(key)
    ties = int((st[:, 0] > 0).sum())
    print(f"[heap boundaries] {key}: heap_tie_pops {int(st[:, 0].sum())} in total, {ties} of {H.SEEDS} seeds with a tie")
    assert 3 * ties >= H.SEEDS, (key, ties)
    assert (st[:, 2] == n).all(), (key, np.unique(st[:, 2]))
    assert (st[:, 1] == n * rounds).all(), (key, np.unique(st[:, 1]))
    assert (H.truth(key)["verdict"] == A.PASS).all()


@pytest.mark.parametrize("key", [k for k in H.all_keys() if k[0] == "steady"], ids=str)
def test_steady_premises(key):
    st = H.stats_by_seed(key)
    assert (st[:, 2] == key[1]).all() and (st[:, 1] == key[1] * key[2]).all(), key
    assert (H.truth(key)["verdict"] == A.PASS).all()


def test_counters_sum_over_a_batch():
    """heap_pops / heap_tie_pops are sums over the seeds of a call, like the tier counters; max_heap stays a maximum."""
    key = ("lockstep", 5, 128, "base")
    st = H.stats_by_seed(key)
    whole = oracle.run_batch(H.workload(key), H.SEED0, H.SEEDS, want_stats=True)[2]
    assert (whole.heap_tie_pops, whole.heap_pops, whole.max_heap) == (int(st[:, 0].sum()), int(st[:, 1].sum()), 5)


_ASYNC_MOD = None


def _async_mod():
    global _ASYNC_MOD
    if _ASYNC_MOD is None:
        p = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "make_golden_async.py")
        spec = importlib.util.spec_from_file_location("make_golden_async", p)
        _ASYNC_MOD = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(_ASYNC_MOD)
    return _ASYNC_MOD


@pytest.mark.parametrize("key", H.all_keys(), ids=str)
def test_truth_agrees_with_the_generator_restatement(key):
    """The oracle's heap against a second statement of BinaryHeap (Python's list algorithm of make_golden_async.py), every result field."""
    mod = _async_mod()
    w, want = H.workload(key), H.truth(key)
    cfg = A.Config.default()
    for i in range(H.GOLDEN_SEEDS):
        ref = mod.Sim(w, cfg, H.SEED0 + i).run(0)
        assert {f: int(want[i][f]) for f in FIELDS} == {f: ref[f] for f in FIELDS}, (key, H.SEED0 + i)
