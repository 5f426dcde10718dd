"""Timelines and probe spans through the public calls on the device.  The truth is never the code under test: it is the oracle's
observation list of each workload's stamped twin (tests/spans_workloads.py, tests/test_spans.py) — values at the even entries, times at
the odd ones."""
import numpy as np
import pytest

from madsim_amd import _abi as A
from madsim_amd import runtime
from tests import spans_ref as R
from tests import spans_workloads as SW
from tests import test_spans as T

pytestmark = pytest.mark.gpu


def check_timelines(got, seeds, truth, cap):
    assert [t.seed for t in got] == list(seeds)
    for t, (vals, times, r) in zip(got, truth):
        assert t.result.astuple()[:6] == r.astuple()[:6], (t.seed, t.result.astuple(), r.astuple())
        assert t.n_observations == len(vals) and t.observations == list(vals[:cap]) and t.times == list(times[:cap]), (t.seed, t.events(), vals, times)


# ---- 1. timelines ---------------------------------------------------------------------------------------------------------------------------
def test_timeline_of_the_pingpong_against_the_stamped_twin(hip):
    w, cfg, lim = SW.case("pingpong")
    seeds = list(range(T.PINGPONG_SEEDS))
    truth = T.pingpong_truth()
    got = hip.timeline(w, seeds, config=cfg, limits=lim, obs_cap=64)
    check_timelines(got, seeds, truth, 64)
    plain = hip.trace_seeds(w, seeds, config=cfg, limits=lim, obs_cap=64)                  # the same values, the same results, no time log asked for
    assert [(p.observations, p.n_observations, p.result.astuple()) for p in plain] == [(t.observations, t.n_observations, t.result.astuple()) for t in got]
    d = [t.span(0x10, 0x20) for t in got]
    assert sum(x is not None for x in d) == 533 and (min(x for x in d if x is not None), max(x for x in d if x is not None)) == (194_016_059, 295_504_218)
    assert got[0].span(None, 0x10) == got[0].times[got[0].observations.index(0x10)] and got[0].span(0x20, 0x10) is None


@pytest.mark.parametrize("name", [n for n in SW.NAMES if n != "pingpong"])
def test_timeline_of_every_trace_build_against_the_stamped_twin(hip, name):
    w, cfg, lim = SW.case(name)
    seeds = list(range(96))
    got = hip.timeline(w, seeds, config=cfg, limits=lim, obs_cap=16)
    check_timelines(got, seeds, T.twin_truth(name, tuple(seeds)), 16)
    plain = hip.trace_seeds(w, seeds, config=cfg, limits=lim, obs_cap=16)
    assert [p.observations for p in plain] == [t.observations for t in got]
    assert any(v != t for tl in got for t, v in tl.events())


def test_timeline_cut_rows_any_order_duplicates_and_a_context(hip):
    w, cfg, lim = SW.case("pingpong")
    seeds = [599, 3, 3, 0, 70, 599]
    truth = T.pingpong_truth()
    want = [truth[s] for s in seeds]
    for cap in (1, 19, 25):                                                            # below every length; where some lists are cut and some are not
        check_timelines(hip.timeline(w, seeds, config=cfg, limits=lim, obs_cap=cap), seeds, want, cap)
    with runtime.Context(0) as ctx:
        check_timelines(ctx.timeline(w, seeds, config=cfg, limits=lim, obs_cap=40), seeds, want, 40)
        # behind a time-log launch on the same context the older calls give what they gave
        assert [p.observations for p in ctx.trace_seeds(w, seeds, config=cfg, limits=lim, obs_cap=40)] == [list(v) for v, _, _ in want]
    with pytest.raises(runtime.MadsimHipError):
        hip.timeline(w, seeds, config=cfg, obs_cap=0)


def test_timeline_resolve_settles_the_seeds_that_overflow_first(hip):
    w, cfg, lim = SW.scope_small_limits()
    seeds = list(range(96))
    raw = hip.timeline(w, seeds, config=cfg, limits=lim, obs_cap=16, resolve=None)
    assert any(t.result.verdict == A.OVERFLOW for t in raw)                             # the premise: under these limits some seeds overflow
    check_timelines(hip.timeline(w, seeds, config=cfg, limits=lim, obs_cap=16), seeds, T.twin_truth("scope", tuple(seeds)), 16)


# ---- 2. probe spans --------------------------------------------------------------------------------------------------------------------------
SPAN_SEEDS = 2048


def same(got, want, tag):
    assert got.n_counted == want.n_counted and (got.n_truncated, got.n_runner) == (want.n_truncated, want.n_runner), (tag, got.n_counted, want.n_counted)
    assert [int(s) for s in got.runner_seeds] == [int(s) for s in want.runner_seeds], tag
    for f in got.spans.dtype.names:
        assert (got.spans[f] == want.spans[f]).all(), (tag, f, got.spans[f], want.spans[f])
    assert got.tobytes() == want.tobytes(), tag


@pytest.mark.parametrize("chunk", [0, 64, 1000])
def test_probe_spans_of_the_pingpong_whatever_the_chunk(hip, chunk):
    w, cfg, lim = SW.case("pingpong")
    want = T.pingpong_ref(SPAN_SEEDS)
    got = hip.probe_spans(w, T.SPANS, 0, SPAN_SEEDS, config=cfg, limits=lim, chunk=chunk)
    same(got, want, chunk)
    assert got.closed(0) > 1700 and got.states(0)["OPEN"] > 150 and got.never_closed(0) == int(want.spans["first_open_seed"][0])


def test_probe_spans_forms_contexts_masks_and_caps(hip):
    w, cfg, lim = SW.case("pingpong")
    want = T.pingpong_ref(SPAN_SEEDS)
    seeds = list(range(SPAN_SEEDS))
    same(hip.probe_spans(w, T.SPANS, seeds=seeds, config=cfg, limits=lim, chunk=700), want, "list")
    pick = sorted(set(range(0, SPAN_SEEDS, 7)) | {1, 2, 3, SPAN_SEEDS - 1})
    same(hip.probe_spans(w, T.SPANS, seeds=pick, config=cfg, limits=lim, chunk=33), T.pingpong_ref(SPAN_SEEDS, pick=pick), "sparse")
    with runtime.Context(0) as ctx:
        a = ctx.probe_spans(w, T.SPANS, 0, SPAN_SEEDS, config=cfg, limits=lim, chunk=500)
        b = ctx.probe_spans(w, T.SPANS, seeds=seeds, config=cfg, limits=lim)
        assert a.tobytes() == b.tobytes() == want.tobytes()
        # behind a spans launch on the same context the older reports give what they gave
        assert [p.observations for p in ctx.trace_seeds(w, seeds[:64], config=cfg, limits=lim, obs_cap=64)] == [list(v) for v, _, _ in T.pingpong_truth(SPAN_SEEDS)[:64]]
    with pytest.raises(runtime.MadsimHipError, match="numpy.unique|ascending"):
        hip.probe_spans(w, T.SPANS, seeds=[5, 5], config=cfg)
    for include, mask in (((A.PASS,), 1), ((A.DEADLOCK,), 4), ((A.PANIC, A.TIME_LIMIT), 0xa)):
        same(hip.probe_spans(w, T.SPANS, 0, SPAN_SEEDS, include=include, config=cfg, limits=lim), T.pingpong_ref(SPAN_SEEDS, include=mask), include)
    for cap in (1, 20, 25):                                                            # CUT and spans closed inside a cut prefix
        cut = hip.probe_spans(w, T.SPANS, 0, SPAN_SEEDS, obs_cap=cap, config=cfg, limits=lim)
        same(cut, T.pingpong_ref(SPAN_SEEDS, obs_cap=cap), cap)
    assert cut.states(0)["CUT"] > 0 and cut.n_truncated > 0
    one = hip.probe_spans(w, [(0x10, 0x20)] * 16, 0, 300, config=cfg, limits=lim)
    assert all(one.spans[k].tobytes() == one.spans[0].tobytes() for k in range(16)) and one.closed(0) == T.pingpong_ref(300).spans["n"][0]


def test_probe_spans_resolve_settles_the_seeds_that_overflow_first(hip):
    w, cfg, lim = SW.scope_small_limits()
    n = 512
    truth = T.twin_truth("scope", tuple(range(n)))
    spans = SW.SPANS_OF["scope"]
    want = R.report_of_lists([v for v, _, _ in truth], [t for _, t, _ in truth], [r.verdict for _, _, r in truth], list(range(n)), spans)
    raw = hip.probe_spans(w, spans, 0, n, config=cfg, limits=lim, resolve=None)
    assert raw.n_runner > 0 and len(raw.runner_seeds) == raw.n_runner                  # the premise: under these limits some seeds overflow first
    got = hip.probe_spans(w, spans, 0, n, config=cfg, limits=lim, chunk=100)
    same(got, want, "resolved")
    assert got.n_runner == 0 and got.closed(0) == n and got.closed(2) > 0


@pytest.mark.parametrize("name", [n for n in SW.NAMES if n != "pingpong"])
def test_probe_spans_on_every_trace_build(hip, name):
    w, cfg, lim = SW.case(name)
    n = 200
    truth = T.twin_truth(name, tuple(range(n)))
    spans = SW.SPANS_OF[name]
    want = R.report_of_lists([v for v, _, _ in truth], [t for _, t, _ in truth], [r.verdict for _, _, r in truth], list(range(n)), spans)
    same(hip.probe_spans(w, spans, 0, n, config=cfg, limits=lim, chunk=64), want, name)
    assert int(want.spans["n"][0]) > 0


def test_the_example_prints_what_the_oracle_implies(hip):
    """examples/span_test.cpp (C++ Builder mirror) over seeds 0..1999: every figure it prints, against the reference over the oracle's lists."""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    n = 2000
    out = subprocess.run([os.path.join(root, "examples", "span_test")], env=dict(os.environ, MADSIM_TEST_SEED="0", MADSIM_TEST_NUM=str(n)),
                         capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    ref = T.pingpong_ref(n, spans=[(0x10, 0x20), (0x11, 0x21)])
    p = T.folded([ref], ref.defs)
    want = [f"test lossy_ping_pong: {n} seeds from 0: {p.n_counted[0]} pass, {p.n_counted[1]} panic, {p.n_counted[2]} deadlock, {p.n_counted[3]} time-limit"]
    for i in range(2):
        med, p99 = p.quantile_bounds(i, 0.5), p.quantile_bounds(i, 0.99)
        want.append(f"  pair {i}: {p.closed(i)} seeds finish the loop, {p.states(i)['OPEN']} never do; loop time median {med[0]}..{med[1]} ns, "
                    f"p99 {p99[0]}..{p99[1]} ns, slowest seed {p.slowest(i)} ({int(p.spans['max'][i])} ns); first seed that never finishes: {p.never_closed(i)}")
    assert out.stdout.splitlines() == want, out.stdout
