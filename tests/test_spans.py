"""Timelines and probe spans on the CPU.  The truth of both is the oracle's observation list of a STAMPED TWIN (tests/spans_workloads.py):
a trace_instant() behind every traced value.  This file proves the premise — the stamp changes nothing of a run — workload by workload,
shows that the ping-pong truth is not vacuous, and holds what needs no device: the surface and its argument errors."""
import ctypes as C
import functools

import numpy as np
import pytest

import oracle
from madsim_amd import _abi as A
from madsim_amd import runtime
from tests import cheader as H
from tests import spans_ref as R
from tests import spans_workloads as SW

E_ARG, E_NOINIT, E_LIMITS = (int(H.defines()[k]) for k in ("MADSIM_E_ARG", "MADSIM_E_NOINIT", "MADSIM_E_LIMITS"))
PINGPONG_SEEDS = 600
FIELDS = ("verdict", "clock_ns", "steps", "msg_count", "rng_calls", "trace_hash")


@functools.lru_cache(maxsize=None)
def twin_truth(name, seeds):
    """Per seed (values, times, result) by the oracle alone: the even and the odd entries of the stamped twin's observation list.  Computed
    once per (workload, seed tuple) and shared, read-only, by the tests of this file, tests/test_timeline_emu.py and tests/test_spans_gpu.py."""
    w, cfg, lim = SW.case(name, stamp=True)
    out = []
    for s in seeds:
        o, r = oracle.observe_seed(w, s, cfg, lim)
        assert len(o) % 2 == 0
        out.append((tuple(int(x) for x in o[0::2]), tuple(int(x) for x in o[1::2]), r))
    return tuple(out)


def pingpong_truth(n=PINGPONG_SEEDS):
    return twin_truth("pingpong", tuple(range(n)))


# ---- the premise ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SW.NAMES)
def test_the_stamp_leaves_the_run_unchanged(name):
    n = PINGPONG_SEEDS if name == "pingpong" else 96
    w, cfg, lim = SW.case(name)
    truth = twin_truth(name, tuple(range(n)))
    for s, (vals, times, r2) in enumerate(truth):
        o, r = oracle.observe_seed(w, s, cfg, lim)
        assert all(getattr(r, f) == getattr(r2, f) for f in FIELDS), (s, r.astuple(), r2.astuple())
        assert tuple(int(x) for x in o) == vals, s                                   # the even entries are the plain run's list
        assert all(a <= b for a, b in zip(times, times[1:])), s                        # the odd entries never decrease
        assert not times or times[-1] <= r.clock_ns, s
    assert any(v != t for vals, times, _ in truth for v, t in zip(vals, times))


def test_the_traced_tick_folds_its_deadline_not_the_clock():
    for vals, times, _ in twin_truth("ticker", tuple(range(96))):
        assert len(vals) == 11 and all(v < t for v, t in zip(vals[1:9], times[1:9]))
    assert any(t - v > 1_000_000 for vals, times, _ in twin_truth("ticker", tuple(range(96))) for v, t in zip(vals[1:9], times[1:9]))


def span_of(vals, times, a, b):
    """(state, duration) of the span a -> b by the definition, on whole lists: 'absent', 'closed' or 'open'."""
    if a not in vals:
        return "absent", None
    i = vals.index(a)
    if b not in vals[i + 1:]:
        return "open", None
    j = vals.index(b, i + 1)
    return "closed", times[j] - times[i]


def test_the_pingpong_truth_is_not_vacuous():
    truth = pingpong_truth()
    verdicts = [r.verdict for _, _, r in truth]
    assert len(set(verdicts)) >= 2 and all(v < 4 for v in verdicts)                  # no runner verdict
    assert (verdicts.count(A.PASS), verdicts.count(A.DEADLOCK)) == (484, 116)
    for pair, (closed, opened) in enumerate(((533, 67), (544, 56))):
        st = [span_of(v, t, 0x10 + pair, 0x20 + pair) for v, t, _ in truth]
        assert ([s for s, _ in st].count("closed"), [s for s, _ in st].count("open")) == (closed, opened)
    d = [x for s, x in (span_of(v, t, 0x10, 0x20) for v, t, _ in truth) if s == "closed"]
    assert (min(d), max(d)) == (194_016_059, 295_504_218)


# ---- the reference against the definition ----------------------------------------------------------------------------------------------------
SPANS = [(0x10, 0x20), (0x11, 0x21), (None, 0x20), (0x30, 0x30), (0x20, 0x10), (0x10, 0x21)]


def random_lists(rng, n, max_len):
    vocab = [0, (1 << 64) - 1, 100, 200, 300, 7, 7]
    obs = [[int(x) for x in rng.choice(np.array(vocab, dtype=np.uint64), int(rng.integers(0, max_len + 1)))] for _ in range(n)]
    times = [[int(x) for x in np.cumsum(rng.integers(0, 1 << 40, len(o)).astype(np.uint64))] for o in obs]
    verdicts = [int(v) for v in rng.choice([0, 0, 1, 2, 2, 3, 4, 5, 7, 0xffffffff], n)]
    seeds = [int(s) for s in np.cumsum(rng.integers(1, 50, n))]
    return obs, times, verdicts, seeds


@pytest.mark.parametrize("obs_cap", [1, 5, 12, 40])
def test_the_numpy_reference_is_the_definition(obs_cap):
    rng = np.random.default_rng(obs_cap)
    obs, times, verdicts, seeds = random_lists(rng, 300, 16)
    spans = [(100, 200), (None, 200), (300, 300), (0, (1 << 64) - 1), (200, 100), (None, 7)]
    (rows, lens), (trows, _) = R.pad(obs, 16), R.pad(times, 16)
    for include in (0xf, 0x1, 0x4, 0xa):
        a = R.report(rows, trows, lens, verdicts, seeds, spans, include, obs_cap)
        b = R.report_of_lists(obs, times, verdicts, seeds, spans, include, obs_cap)
        assert a.tobytes() == b.tobytes(), include
    assert a.n_runner and (a.n_truncated > 0) == (obs_cap < 16)


def pingpong_ref(n=PINGPONG_SEEDS, spans=SPANS, include=0xf, obs_cap=256, pick=None):
    truth = pingpong_truth(n)
    idx = range(n) if pick is None else pick
    return R.report_of_lists([truth[i][0] for i in idx], [truth[i][1] for i in idx], [truth[i][2].verdict for i in idx], list(idx), spans, include, obs_cap)


def test_the_pingpong_report_says_what_the_truth_says():
    want = pingpong_ref()
    s0, s1 = want.spans[0], want.spans[1]
    assert (int(s0["n"]), int(s0["min"]), int(s0["max"])) == (533, 194_016_059, 295_504_218) and int(s1["n"]) == 544
    assert int(s0["n_state"][:, R.OPEN].sum()) == 67 and int(s1["n_state"][:, R.OPEN].sum()) == 56 and want.n_runner == 0
    assert int(s0["first_open_seed"]) < PINGPONG_SEEDS and int(want.spans[4]["n"]) == 0            # a loop never ends before it has begun
    assert int(want.spans[3]["n"]) > 500                                                          # the period of a round
    cut = pingpong_ref(obs_cap=20)
    assert int(cut.spans[0]["n_state"][:, R.CUT].sum()) > 0 and cut.n_truncated > 0


# ---- the records, the header, the surface ----------------------------------------------------------------------------------------------------
def test_record_sizes_and_header_constants():
    d = H.defines()
    assert (int(d["MADSIM_PROBE_SPANS_MAX"].rstrip("u")), int(d["MADSIM_SPAN_FROM_START"].rstrip("u"))) == (A.PROBE_SPANS_MAX, A.SPAN_FROM_START)
    assert [int(d[f"MADSIM_SPAN_{k}"].rstrip("u")) for k in ("ABSENT", "CLOSED", "OPEN", "CUT")] == [A.SPAN_ABSENT, A.SPAN_CLOSED, A.SPAN_OPEN, A.SPAN_CUT]
    assert (C.sizeof(A.SpanDef), C.sizeof(A.Span), C.sizeof(A.ProbeSpans)) == (24, 2240, 104)
    assert (np.dtype(A.SPAN_DEF_DTYPE).itemsize, np.dtype(A.SPAN_DTYPE).itemsize) == (24, 2240) and A.SPAN_REC_WORDS * 8 == 2240
    for name, st in (("madsim_span_def_t", A.SpanDef), ("madsim_span_t", A.Span), ("madsim_probe_spans_t", A.ProbeSpans)):
        assert A.HEADER_STRUCTS[name] is st
    e = runtime.empty_spans(2)
    assert all(int(e[f][1]) == (1 << 64) - 1 for f in ("min", "min_seed", "max_seed", "first_open_seed")) and not e["hist"].any() and int(e["max"][0]) == 0


def call(range_form=True, seeds=None, **kw):
    """madsim_hip_probe_spans_range / _seeds with one argument made wrong, no device initialised: the return code."""
    w, cfg, lim = SW.case("pingpong")
    a = dict(include=0xf, obs_cap=64, n_spans=2, flags=0, runner_cap=0, runner=True, defs=True, spans=True)
    a.update(kw)
    defs, recs, runner = R.defs_of([(1, 2)] * 16), np.zeros(16, dtype=A.SPAN_DTYPE), np.zeros(4, dtype=np.uint64)
    defs["flags"] = a["flags"]
    ps = A.ProbeSpans(include=a["include"], obs_cap=a["obs_cap"], n_spans=a["n_spans"], runner_cap=a["runner_cap"])
    if a["defs"]:
        ps.defs = defs.ctypes.data_as(C.POINTER(A.SpanDef))
    if a["spans"]:
        ps.spans = recs.ctypes.data_as(C.POINTER(A.Span))
    if a["runner"]:
        ps.runner_seeds = runner.ctypes.data_as(C.POINTER(C.c_uint64))
    L = runtime.lib()
    if range_form:
        return L.madsim_hip_probe_spans_range(w.ref(), C.byref(cfg), 0, 10, 0, C.byref(lim), C.byref(ps))
    s = np.array(seeds, dtype=np.uint64)
    return L.madsim_hip_probe_spans_seeds(w.ref(), C.byref(cfg), s.ctypes.data_as(C.POINTER(C.c_uint64)), len(s), 0, C.byref(lim), C.byref(ps))


def test_argument_errors_need_no_device():
    for bad in (dict(n_spans=0), dict(n_spans=17), dict(flags=2), dict(flags=0x80000000), dict(include=0), dict(include=0x10), dict(include=0x1f),
                dict(obs_cap=0), dict(obs_cap=A.CENSUS_MAX_OBS_CAP + 1), dict(runner_cap=4, runner=False), dict(defs=False), dict(spans=False)):
        assert call(**bad) == E_ARG, bad
    assert call(range_form=False, seeds=[3, 2]) == E_ARG and call(range_form=False, seeds=[2, 2]) == E_ARG
    L = runtime.lib()
    w, cfg, lim = SW.case("pingpong")
    assert L.madsim_hip_probe_spans_range(w.ref(), C.byref(cfg), 0, 10, 0, C.byref(lim), None) == E_ARG
    s = np.arange(4, dtype=np.uint64)
    o, t = np.zeros((4, 8), dtype=np.uint64), np.zeros((4, 8), dtype=np.uint64)
    p = lambda x: x.ctypes.data_as(C.c_void_p)          # noqa: E731
    sp = s.ctypes.data_as(C.POINTER(C.c_uint64))
    assert L.madsim_hip_timeline_seeds(w.ref(), C.byref(cfg), sp, 4, C.byref(lim), p(o), None, 8, None, None) == E_ARG
    assert L.madsim_hip_timeline_seeds(w.ref(), C.byref(cfg), sp, 4, C.byref(lim), None, p(t), 8, None, None) == E_ARG
    assert L.madsim_hip_timeline_seeds(w.ref(), C.byref(cfg), sp, 4, C.byref(lim), p(o), p(t), 0, None, None) == E_ARG
    assert L.madsim_hip_timeline_seeds(w.ref(), C.byref(cfg), None, 4, C.byref(lim), p(o), p(t), 8, None, None) == E_ARG
    assert L.madsim_hip_timeline_seeds(w.ref(), C.byref(cfg), sp, 1 << 22, C.byref(lim), p(o), p(t), 64, None, None) == E_LIMITS
    assert L.madsim_hip_timeline_seeds(w.ref(), C.byref(cfg), sp, 0, C.byref(lim), None, None, 0, None, None) == 0
    with pytest.raises(runtime.MadsimHipError):
        runtime.span_defs([])
    with pytest.raises(runtime.MadsimHipError):
        runtime.span_defs([(1, 2)] * 17)
    assert [tuple(int(x) for x in d) for d in runtime.span_defs([(None, 5), (3, 3)])] == [(0, 5, 1, 0), (3, 3, 0, 0)]


# ---- the host fold ---------------------------------------------------------------------------------------------------------------------------
def folded(chunks, defs, include=0xf, obs_cap=256):
    """runtime.ProbeSpans of reference-made device words and records, chunk after chunk through madsim_k_fold_probe_spans."""
    spans = runtime.empty_spans(len(defs))
    ps = A.ProbeSpans(include=include, obs_cap=obs_cap, n_spans=len(defs))
    ps.defs, ps.spans = defs.ctypes.data_as(C.POINTER(A.SpanDef)), spans.ctypes.data_as(C.POINTER(A.Span))
    runner = []
    for ref in chunks:
        recs, words = np.ascontiguousarray(ref.records()), ref.words()
        assert runtime.lib().madsim_k_fold_probe_spans(C.byref(ps), words.ctypes.data_as(C.c_void_p), recs.ctypes.data_as(C.c_void_p), len(defs)) == 0
        runner += [int(s) for s in ref.runner_seeds]
    return runtime.ProbeSpans(defs, spans, ps.n_counted, ps.n_truncated, ps.n_runner, np.array(sorted(runner), dtype=np.uint64), include, obs_cap)


@pytest.mark.parametrize("chunk", [1, 64, 1000])
def test_a_range_cut_into_chunks_folds_to_the_bytes_of_the_whole(chunk):
    rng = np.random.default_rng(7)
    obs, times, verdicts, seeds = random_lists(rng, 1500, 24)
    spans = [(100, 200), (None, 200), (300, 300), (0, (1 << 64) - 1)]
    whole = R.report_of_lists(obs, times, verdicts, seeds, spans, 0xf, 16)
    parts = [R.report_of_lists(obs[i:i + chunk], times[i:i + chunk], verdicts[i:i + chunk], seeds[i:i + chunk], spans, 0xf, 16) for i in range(0, 1500, chunk)]
    got = folded(parts, whole.defs, obs_cap=16)
    assert got.tobytes() == whole.tobytes()
    assert got.tobytes() == folded(parts[::-1], whole.defs, obs_cap=16).tobytes()                # in either order
    assert folded([whole], whole.defs, obs_cap=16).tobytes() == whole.tobytes()
    ps = A.ProbeSpans(n_spans=3)
    assert runtime.lib().madsim_k_fold_probe_spans(C.byref(ps), None, None, 4) == -1


def test_ties_of_an_extreme_across_chunks_go_to_the_smaller_seed():
    mk = lambda seed, d: R.report_of_lists([[1, 2]], [[10, 10 + d]], [0], [seed], [(1, 2)])          # noqa: E731
    for order in ([mk(9, 50), mk(4, 50), mk(6, 50)], [mk(4, 50), mk(9, 50)], [mk(9, 50), mk(4, 70), mk(3, 50), mk(2, 70), mk(1, 60)]):
        got = folded(order, order[0].defs)
        ds = {9: 50, 6: 50}
        want_min = min(int(r.spans["min_seed"][0]) for r in order if int(r.spans["min"][0]) == int(got.spans["min"][0]))
        want_max = min(int(r.spans["max_seed"][0]) for r in order if int(r.spans["max"][0]) == int(got.spans["max"][0]))
        assert (got.fastest(0), got.slowest(0)) == (want_min, want_max), ds
    got = folded([mk(9, 50), mk(4, 70), mk(3, 50), mk(2, 70), mk(1, 60)], mk(1, 1).defs)
    assert (got.fastest(0), got.slowest(0), got.closed(0), got.total(0), got.mean(0)) == (3, 2, 5, 300, 60)


def test_merge_and_the_readers():
    whole = pingpong_ref()
    half = PINGPONG_SEEDS // 2
    a = folded([pingpong_ref(pick=range(0, half))], whole.defs)
    b = folded([pingpong_ref(pick=range(half, PINGPONG_SEEDS))], whole.defs)
    assert a.merge(b).tobytes() == b.merge(a).tobytes() == whole.tobytes()
    got = a.merge(b)
    truth = pingpong_truth()
    d = sorted(x for s, x in (span_of(v, t, 0x10, 0x20) for v, t, _ in truth) if s == "closed")
    assert got.closed(0) == len(d) and got.states(0)["OPEN"] == 67 and got.states(0, A.DEADLOCK)["OPEN"] == 67 and got.states(0, A.PASS)["CLOSED"] == 484
    assert got.mean(0) * len(d) == sum(d) and got.total(0) == sum(d)
    for q in (0, 0.5, 0.99, 1):
        lo, hi = got.quantile_bounds(0, q)
        exact = d[max(1, -(-int(q * 1000) * len(d) // 1000)) - 1]
        assert lo <= exact <= hi and hi < lo * 1.26 + 4, (q, lo, exact, hi)
    slow = got.slowest(0)
    assert span_of(*truth[slow][:2], 0x10, 0x20) == ("closed", d[-1]) and span_of(*truth[got.fastest(0)][:2], 0x10, 0x20) == ("closed", d[0])
    never = got.never_closed(0)
    assert span_of(*truth[never][:2], 0x10, 0x20)[0] == "open" and all(span_of(*truth[s][:2], 0x10, 0x20)[0] != "open" for s in range(never))
    assert got.slowest(4) is None and got.fastest(4) is None and got.mean(4) is None and got.quantile_bounds(4, 0.5) is None
    assert got.never_closed(4) == min(s for s, (v, _, _) in enumerate(truth) if 0x20 in v)          # 0x20 -> 0x10: open wherever 0x20 fires
    absent = folded([pingpong_ref(spans=[(0x99, 0x10)])], R.defs_of([(0x99, 0x10)]))
    assert absent.never_closed(0) is None and absent.states(0) == {"ABSENT": 600, "CLOSED": 0, "OPEN": 0, "CUT": 0}
    assert got.definitions == SPANS
    with pytest.raises(runtime.MadsimHipError):
        a.merge(folded([pingpong_ref(spans=SPANS[:2])], R.defs_of(SPANS[:2])))


def test_the_time_log_parameter_moves_no_kernel_argument():
    """Every field of KParams keeps its kernel-argument offset and the block its size: obs_time_words takes the word that was padding between
    has_clog and lat_low, and the block still ends with the task log's fields (tests/test_stall.py holds it to that)."""
    import os
    kh = open(os.path.join(os.path.dirname(os.path.abspath(runtime.__file__)), "csrc", "sim_kernel.h")).read()
    body = kh[kh.index("struct KParams {"):kh.index("// The compiled builds")]
    assert "uint32_t lat_mode; uint32_t has_clog_link; uint32_t has_clog; uint32_t obs_time_words; uint64_t lat_low, lat_range, lat_zone;" in body
    assert "pad0" not in body and body.rstrip().endswith("uint64_t* task_log; uint64_t task_cap; uint64_t* task_len;\n};")
