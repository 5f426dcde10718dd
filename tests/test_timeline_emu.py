"""The trace builds' time log on a box without a GPU: the device code compiled for the host (tests/span_emu) runs every workload of
tests/spans_workloads.py, and the time row of each seed must be the odd entries of the ORACLE's observation list of the stamped twin — the
oracle knows nothing of a time log, the twin's trace_instant()s are its only clock (tests/test_spans.py proves the stamp changes nothing).
This checks the kernel's LOGIC: that the clock at the observation is stored and not the value (the ticker's late ticks, the system time),
at the observation's own index, under the observation log's cap guard, by all five trace builds.  tests/test_spans_gpu.py runs the same
cases through the product library on the device.

(The trace builds compile one layout, the extended one with every class: there is no compact or base-op trace build to run beside it.)"""
import numpy as np
import pytest

from madsim_amd import _abi as A
from tests import span_emu
from tests import spans_workloads as SW
from tests import test_spans as T

SEEDS = list(range(0, 70)) + [599, 1 << 40, (1 << 64) - 1]        # more lanes than one wave on two emulated compute units, a second pass, wide seeds


def twin_truth(name, seeds=tuple(SEEDS)):
    return T.twin_truth(name, tuple(seeds))


def check_rows(res, obs, tim, lens, truth, cap, twice=False):
    for i, (vals, times, r) in enumerate(truth):
        if twice:                                     # the stamped run on the device: every value followed by its own stamp
            vals = tuple(x for v, t in zip(vals, times) for x in (v, t))
            times = tuple(x for t in times for x in (t, t))
        k = min(len(vals), cap)
        assert int(lens[i]) == len(vals), (i, int(lens[i]), len(vals))
        assert [int(x) for x in obs[i]] == list(vals[:k]) + [0] * (cap - k), i
        assert [int(x) for x in tim[i]] == list(times[:k]) + [0] * (cap - k), (i, [int(x) for x in tim[i]], times)
        assert tuple(int(res[f][i]) for f in ("verdict", "clock_ns", "steps", "msg_count", "rng_calls")) == (r.verdict, r.clock_ns, r.steps, r.msg_count, r.rng_calls)


@pytest.mark.parametrize("name", SW.NAMES)
def test_the_time_row_is_the_stamped_twins_odd_entries(name):
    w, cfg, lim = SW.case(name)
    res, obs, tim, lens, _ = span_emu.timeline(w, SEEDS, 64, cfg, lim)
    check_rows(res, obs, tim, lens, twin_truth(name), 64)
    assert (tim != obs).any()                         # a time log that stored the value would pass nowhere


@pytest.mark.parametrize("name", SW.NAMES)
def test_the_stamped_run_holds_each_time_twice(name):
    w, cfg, lim = SW.case(name, stamp=True)
    res, obs, tim, lens, _ = span_emu.timeline(w, SEEDS[:20], 128, cfg, lim)
    check_rows(res, obs, tim, lens, twin_truth(name)[:20], 128, twice=True)
    assert (tim[:, 0::2] == tim[:, 1::2]).all() and (obs[:, 1::2] == tim[:, 1::2]).all()


def test_the_five_workloads_run_the_five_trace_builds():
    feats = set()
    for name in SW.NAMES:
        w, cfg, lim = SW.case(name)
        feats.add(span_emu.timeline(w, [1], 8, cfg, lim)[4])
    assert len(feats) == 5, feats


@pytest.mark.parametrize("cap", [1, 7, 19, 40])
def test_both_rows_are_cut_at_the_same_index(cap):
    """The ping-pong's lists hold 19 to 36 entries: caps below every length, inside the lengths' range and above them all."""
    w, cfg, lim = SW.case("pingpong")
    truth = twin_truth("pingpong")
    assert min(len(v) for v, _, _ in truth) >= 19 and max(len(v) for v, _, _ in truth) < 40
    res, obs, tim, lens, _ = span_emu.timeline(w, SEEDS, cap, cfg, lim)
    check_rows(res, obs, tim, lens, truth, cap)
    assert (lens > cap).any() == (cap < 40) and ((lens < cap).any() == (cap > 19))


def test_times_never_decrease_and_a_late_tick_lies_before_its_time():
    w, cfg, lim = SW.case("ticker")
    _, obs, tim, lens, _ = span_emu.timeline(w, SEEDS, 16, cfg, lim)
    assert (lens == 11).all() and (np.diff(tim[:, :11].astype(np.int64), axis=1) >= 0).all()
    ticks_v, ticks_t = obs[:, 1:9], tim[:, 1:9]
    assert (ticks_v < ticks_t).all() and (ticks_t - ticks_v > 1_000_000).any()        # the deadline a tick was scheduled for; some ran milliseconds late


def test_a_null_time_log_stores_nothing_and_changes_nothing():
    w, cfg, lim = SW.case("pingpong")
    a = span_emu.timeline(w, SEEDS[:12], 64, cfg, lim)
    b = span_emu.timeline(w, SEEDS[:12], 64, cfg, lim, times=False)
    assert a[0].tobytes() == b[0].tobytes() and (a[1] == b[1]).all() and (a[3] == b[3]).all() and not b[2].any() and a[2].any()


def test_duplicates_and_any_order():
    w, cfg, lim = SW.case("scope")
    seeds = [5, 3, 5, 0, 3]
    res, obs, tim, lens, _ = span_emu.timeline(w, seeds, 16, cfg, lim)
    check_rows(res, obs, tim, lens, twin_truth("scope", tuple(seeds)), 16)
    assert (tim[0] == tim[2]).all() and (tim[1] == tim[4]).all()


def test_a_runner_verdict_is_reported_as_such():
    w, cfg, _ = SW.case("pingpong")
    lim = A.Limits()
    lim.max_steps = 40
    res, obs, tim, lens, _ = span_emu.timeline(w, [1, 2], 16, cfg, lim)
    assert (res["verdict"] == A.STEP_LIMIT).all() and ((tim != 0) <= (np.arange(16)[None, :] < lens[:, None])).all()
