"""Campaign statistics (madsim_hip_run_campaign_stats and its _ctx_ / _multi forms) without a GPU: the three structs against the header,
the exported symbols, the bucket rule of the two host helpers, the argument errors that need no device, the loud failure of a valid call
on a host without one — and the host-side truth itself (tests/stats_ref.py) on the oracle's results.  What the GPU answers is
tests/test_campaign_stats_gpu.py's business."""
import collections
import ctypes as C
import math
import random
import re

import numpy as np
import pytest

from madsim_amd import _abi as A
from madsim_amd import runtime, workload
from tests import cheader as H
from tests import stats_ref as R

E_ARG, E_HIP, E_NOINIT = -1, -2, -3
U64_MAX = (1 << 64) - 1


def _no_gpu():
    import torch
    return not torch.cuda.is_available()


def test_structs_and_constants_match_the_header():
    # madsim_stats_t holds madsim_metric_t by value and is declared in two statements: joined here, laid out with the inner sizes given
    joined = re.sub(r"\bstruct\s+(madsim_stats)\s*\{([^{}]*)\}\s*;\s*typedef\s+struct\s+\1\s+(\w+)\s*;", r"typedef struct \1 {\2} \3;", H.header_text())
    S = H.structs(joined)
    assert [f[:3] for f in S["madsim_extreme_t"]] == [("value", "uint64_t", 0), ("seed", "uint64_t", 0)]
    assert [f[:3] for f in S["madsim_metric_t"]] == [("min", "uint64_t", 0), ("max", "uint64_t", 0), ("sum_lo", "uint64_t", 0), ("sum_hi", "uint64_t", 0),
                                                     ("hist", "uint64_t", 256)]
    assert [(f[0], f[1], f[2], f[3]) for f in S["madsim_stats_t"]] == [
        ("include", "uint32_t", 0, False), ("top_k", "uint32_t", 0, False), ("top", "madsim_extreme_t", 0, True), ("n", "uint64_t", 0, False),
        ("n_top", "uint64_t", 0, False), ("metric", "madsim_metric_t", 4, False)]
    inner = {"madsim_extreme_t": (H.layout(S["madsim_extreme_t"])[1], 8), "madsim_metric_t": (H.layout(S["madsim_metric_t"])[1], 8)}
    assert inner["madsim_extreme_t"][0] == 16 and inner["madsim_metric_t"][0] == 2080
    for name, cls, want_size in (("madsim_extreme_t", A.Extreme, 16), ("madsim_metric_t", A.Metric, 2080), ("madsim_stats_t", A.Stats, 8 + 8 + 8 + 8 + 4 * 2080)):
        offs, size = H.layout(S[name], inner)
        assert size == want_size == C.sizeof(cls), (name, size, C.sizeof(cls))
        assert [f[0] for f in cls._fields_] == [f[0] for f in S[name]], name
        for fname, _, _, _ in S[name]:
            assert getattr(cls, fname).offset == offs[fname], (name, fname)
    assert (A.Stats.top.offset, A.Stats.n.offset, A.Stats.metric.offset, A.Metric.hist.offset) == (8, 16, 32, 32)
    dt = np.dtype(A.EXTREME_DTYPE)
    assert dt.itemsize == 16 and dt.names == ("value", "seed") and dt.fields["seed"][1] == A.Extreme.seed.offset == 8
    D = {k: int(v.rstrip("u")) for k, v in H.defines().items() if k.startswith("MADSIM_STAT_") or k == "MADSIM_HIP_ABI_VERSION"}
    assert [D["MADSIM_STAT_" + k] for k in ("CLOCK", "STEPS", "MSGS", "RNG", "METRICS", "BUCKETS", "MAX_TOP")] == [0, 1, 2, 3, 4, 256, 16]
    assert (A.STAT_CLOCK, A.STAT_STEPS, A.STAT_MSGS, A.STAT_RNG, A.STAT_METRICS, A.STAT_BUCKETS, A.STAT_MAX_TOP) == (0, 1, 2, 3, 4, 256, 16)
    assert A.STAT_NAMES == R.METRICS == ("clock_ns", "steps", "msg_count", "rng_calls")
    assert D["MADSIM_HIP_ABI_VERSION"] == A.ABI_VERSION == 7                            # additive: the version stays


def test_library_exports_the_entry_points():
    L = runtime.lib()
    fns = H.functions()
    collect = fns["madsim_hip_run_campaign_collect"][1]
    assert fns["madsim_hip_run_campaign_stats"] == ("int", collect + ["madsim_stats_t*"])
    assert fns["madsim_hip_ctx_run_campaign_stats"] == ("int", ["madsim_hip_ctx_t*"] + collect + ["madsim_stats_t*"])
    assert fns["madsim_hip_run_campaign_stats_multi"] == ("int", ["madsim_hip_ctx_t* const*", "int"] + collect + ["madsim_stats_t*"])
    assert fns["madsim_hip_stat_bucket"] == ("uint32_t", ["uint64_t"]) and fns["madsim_hip_stat_bucket_floor"] == ("uint64_t", ["uint32_t"])
    for name in ("madsim_hip_run_campaign_stats", "madsim_hip_ctx_run_campaign_stats", "madsim_hip_run_campaign_stats_multi",
                 "madsim_hip_stat_bucket", "madsim_hip_stat_bucket_floor"):
        assert hasattr(L, name), name


def _py_bucket(v):
    """The rule as include/madsim_hip.h states it."""
    if v < 4:
        return v
    e = v.bit_length() - 1
    return 4 * (e - 1) + ((v >> (e - 2)) & 3)


def _py_floor(b):
    if b < 4:
        return b
    return U64_MAX if b >= 252 else (4 + b % 4) << (b // 4 - 1)


def test_bucket_and_floor_follow_the_rule():
    L = runtime.lib()
    values = set(range(65))
    for e in range(2, 64):
        values |= {(1 << e) - 1, 1 << e, (1 << e) + 1, 3 << (e - 1)}
    values.add(U64_MAX)
    rng = random.Random(20261017)
    values |= {rng.getrandbits(64) for _ in range(100_000)}
    values |= {rng.getrandbits(rng.randrange(1, 65)) for _ in range(10_000)}        # every magnitude, not only the top octaves
    values = sorted(values)
    got = [L.madsim_hip_stat_bucket(v) for v in values]
    assert got == [_py_bucket(v) for v in values] == [A.stat_bucket(v) for v in values] == [R.bucket(v) for v in values]
    assert (R.buckets(np.array(values, dtype=np.uint64)) == np.array(got)).all()
    assert L.madsim_hip_stat_bucket(U64_MAX) == 251 and L.madsim_hip_stat_bucket(0) == 0 and max(got) == 251
    assert all(a <= b for a, b in zip(got, got[1:]))                                  # monotone
    floors = [L.madsim_hip_stat_bucket_floor(b) for b in range(300)]
    assert floors == [_py_floor(b) for b in range(300)] == [A.stat_bucket_floor(b) for b in range(300)] == [R.bucket_floor(b) for b in range(300)]
    assert floors[252] == floors[255] == floors[299] == U64_MAX and floors[251] == 7 << 61
    assert all(floors[b] < floors[b + 1] for b in range(251))
    assert all(L.madsim_hip_stat_bucket(floors[b]) == b and (floors[b] == 0 or L.madsim_hip_stat_bucket(floors[b] - 1) == b - 1) for b in range(252))
    for v, b in zip(values, got):
        assert floors[b] <= v and (v < floors[b + 1] or b == 251), v
        assert b < 4 or (floors[b + 1] - floors[b]) * 4 <= floors[b] or b == 251      # at most 25 % wide


def _stats(include=1, top_k=0, with_array=True):
    st = A.Stats()
    st.include, st.top_k = include, top_k
    st._keep = (A.Extreme * (4 * max(top_k, 1)))()
    if with_array:
        st.top = C.cast(st._keep, C.POINTER(A.Extreme))
    return st


def _collect(cap, with_array=True):
    col = A.Collect()
    col.cap = cap
    col._keep = (A.Failure * max(cap, 1))()
    if with_array:
        col.failures = C.cast(col._keep, C.POINTER(A.Failure))
    return col


def _call(st, col=None, flags=0, in_flight=0):
    """Every form of the call with the same arguments: the default context, an explicit (null) context, a list of contexts."""
    L = runtime.lib()
    w, cfg, lim, rep = workload.pingpong(4, 8), A.Config.default(), A.Limits(), A.Campaign()
    stp = C.byref(st) if st is not None else None
    colp = C.byref(col) if col is not None else None
    arr = (C.c_void_p * 1)(None)
    return (L.madsim_hip_run_campaign_stats(w.ref(), C.byref(cfg), 0, 100, 0, in_flight, flags, C.byref(lim), C.byref(rep), colp, stp),
            L.madsim_hip_ctx_run_campaign_stats(None, w.ref(), C.byref(cfg), 0, 100, 0, in_flight, flags, C.byref(lim), C.byref(rep), colp, stp),
            L.madsim_hip_run_campaign_stats_multi(arr, 1, w.ref(), C.byref(cfg), 0, 100, 0, in_flight, flags, C.byref(lim), C.byref(rep), colp, stp))


def test_argument_errors_need_no_gpu():
    """Told before any context is looked at, so these hold with and without a device (the contexts here are null)."""
    assert _call(None) == (E_ARG,) * 3                                                     # null st
    assert _call(_stats(include=0)) == (E_ARG,) * 3                                        # nothing counted
    for bad in (16, 1 | 16, 1 << 7, 1 << 31):
        assert _call(_stats(include=bad)) == (E_ARG,) * 3, bad                             # a bit at or above 4: runner verdicts are never counted
    assert _call(_stats(top_k=17)) == (E_ARG,) * 3                                         # top_k > MADSIM_STAT_MAX_TOP
    assert _call(_stats(top_k=4, with_array=False)) == (E_ARG,) * 3                        # top_k > 0 without top
    # collect's own errors when col is given
    assert _call(_stats(), _collect(4, with_array=False)) == (E_ARG,) * 3
    assert _call(_stats(), _collect(0), flags=A.CAMPAIGN_STOP_AT_CAP) == (E_ARG,) * 3
    assert _call(_stats(), _collect(4), in_flight=9) == (E_ARG,) * 3
    assert _call(_stats(), None, in_flight=9) == (E_ARG,) * 3
    L = runtime.lib()
    w, cfg, lim, st = workload.pingpong(4, 8), A.Config.default(), A.Limits(), _stats()
    assert L.madsim_hip_run_campaign_stats(w.ref(), C.byref(cfg), 0, 100, 0, 0, 0, C.byref(lim), None, None, C.byref(st)) == E_ARG        # null report
    # the mirror raises for the same things
    w = workload.pingpong(4, 8)
    for kw in (dict(include=()), dict(include=(A.OVERFLOW,)), dict(include=(A.PASS, 9)), dict(top_k=17), dict(top_k=-1),
               dict(collect=0, stop_at_cap=True), dict(in_flight=9)):
        with pytest.raises(runtime.MadsimHipError):
            runtime.run_campaign_stats_multi([], w, 0, 100, **kw)


def test_a_valid_call_without_a_context_fails_loudly():
    """Null contexts: never statistics of nothing that look like an answer."""
    for st, col in ((_stats(), None), (_stats(15, 16), None), (_stats(1, 3), _collect(4))):
        rcs = _call(st, col)
        assert rcs[1] == E_NOINIT and rcs[2] == E_NOINIT
        assert rcs[0] in (E_NOINIT, E_HIP) or not _no_gpu()
    if _no_gpu():
        w = workload.pingpong(4, 8)
        for kw in (dict(), dict(top_k=16, include=(A.PASS, A.DEADLOCK)), dict(collect=16)):
            with pytest.raises(runtime.MadsimHipError, match="HIP|context|initiali"):
                runtime.run_campaign_stats(w, 0, 1000, **kw)


def test_the_mirror_has_the_three_forms():
    import inspect
    for fn in (runtime.run_campaign_stats, runtime.run_campaign_stats_multi, runtime.Context.run_campaign_stats):
        p = inspect.signature(fn).parameters
        assert (p["include"].default, p["top_k"].default, p["collect"].default) == ((A.PASS,), 0, None)
    names = list(inspect.signature(runtime.run_campaign_stats).parameters)
    assert names[:8] == ["workload", "seed0", "total", "batch", "in_flight", "stop_at_failure", "config", "limits"]


# ---- the host-side truth ---------------------------------------------------------------------------------------------------

PASS, DEADLOCK = R.mask(A.PASS), R.mask(A.DEADLOCK)
ALL = R.mask(A.PASS, A.PANIC, A.DEADLOCK, A.TIME_LIMIT)


def test_the_truth_on_the_lossy_pingpong_range():
    """What the range exercises (the table of the GPU tests): counts, ties at the maximum, a total tie, the bit lengths covered."""
    _, _, want = R.lossy_pingpong()
    v = want["verdict"]
    assert (int((v == A.PASS).sum()), int((v == A.DEADLOCK).sum())) == (35_330, 4_670)
    t = R.stats_truth(want, R.SEED0, PASS, 16)
    assert (t["n"], t["n_top"]) == (35_330, 16)
    ok = want[v == A.PASS]
    seeds = R.SEED0 + np.nonzero(v == A.PASS)[0]
    assert len(set(ok["clock_ns"].tolist())) == 35_315 and len({e[0] for e in t["clock_ns"]["top"]}) == 16
    assert set(ok["steps"].tolist()) == {402, 403} and int((ok["steps"] == 403).sum()) == 17_722
    assert t["steps"]["top"] == [(403, int(s)) for s in seeds[ok["steps"] == 403][:16]]          # the 16 smallest seeds of the tie
    assert set(ok["msg_count"].tolist()) == {64} and t["msg_count"]["top"] == [(64, int(s)) for s in seeds[:16]]
    assert len(set(ok["rng_calls"].tolist())) == 183 and {int(x).bit_length() for x in ok["rng_calls"]} == {10, 11}
    both = R.stats_truth(want, R.SEED0, PASS | DEADLOCK, 16)
    counted = want[(v == A.PASS) | (v == A.DEADLOCK)]
    assert both["n"] == 40_000 and {int(x).bit_length() for x in counted["rng_calls"]} == set(range(7, 12))
    assert {int(x).bit_length() for x in counted["msg_count"]} == set(range(2, 8))
    for name in R.METRICS:                                                                        # the fields against plain Python
        vals = [int(x) for x in ok[name]]
        m = t[name]
        assert (m["min"], m["max"], m["sum"]) == (min(vals), max(vals), sum(vals)) and int(m["hist"].sum()) == len(vals)
        per_bucket = collections.Counter(map(_py_bucket, vals))
        assert [int(c) for c in m["hist"]] == [per_bucket.get(k, 0) for k in range(256)]
        assert m["top"] == sorted(zip(vals, map(int, seeds)), key=lambda e: (-e[0], e[1]))[:16]
    # nothing counted: the neutral elements
    none = R.stats_truth(want, R.SEED0, R.mask(A.PANIC), 16)
    assert (none["n"], none["n_top"]) == (0, 0) and all(none[m]["min"] == U64_MAX and none[m]["max"] == 0 and none[m]["sum"] == 0 and none[m]["top"] == []
                                                        and not none[m]["hist"].any() for m in R.METRICS)


@pytest.mark.parametrize("batch", [100, 4096])
@pytest.mark.parametrize("include", [PASS, DEADLOCK, ALL])
def test_folding_the_batches_gives_the_truth_of_the_whole(batch, include):
    _, _, want = R.lossy_pingpong()
    for top_k in (0, 1, 16):
        whole = R.stats_truth(want, R.SEED0, include, top_k)
        parts = [R.stats_truth(want[lo:lo + batch], R.SEED0 + lo, include, top_k) for lo in range(0, R.TOTAL, batch)]
        assert R.same(R.fold(parts, top_k), whole), (batch, include, top_k)
        assert R.same(R.fold(parts[::-1], top_k), whole)                                          # the fold does not depend on the order either


def test_quantile_bounds_contain_the_element():
    _, _, want = R.lossy_pingpong()
    for include in (PASS, PASS | DEADLOCK):
        t = R.stats_truth(want, R.SEED0, include, 0)
        v = want["verdict"]
        counted = want[(v < 4) & (((include >> np.minimum(v, 31)) & 1) != 0)]
        st = A.Stats()                                                                            # the mirror's quantile over the same histogram
        st.include, st.n = include, t["n"]
        for m, name in enumerate(R.METRICS):
            st.metric[m].min, st.metric[m].max = t[name]["min"], t[name]["max"]
            st.metric[m].sum_lo, st.metric[m].sum_hi = t[name]["sum"] & U64_MAX, t[name]["sum"] >> 64
            for b in range(256):
                st.metric[m].hist[b] = int(t[name]["hist"][b])
        stats = runtime.CampaignStats(st, np.zeros((4, 0), dtype=A.EXTREME_DTYPE))
        assert R.same(R.of_stats(stats), t) and stats.mean["steps"] == t["steps"]["sum"] / t["n"]
        for name in R.METRICS:
            s = np.sort(counted[name])
            for q in (0.001, 0.5, 0.99, 1):
                x = int(s[math.ceil(q * t["n"]) - 1])
                lo, hi = R.quantile_bounds(t, name, q)
                assert lo <= x <= hi and (lo, hi) == stats.quantile(name, q), (name, q, lo, x, hi)
                assert t[name]["min"] <= lo and hi <= t[name]["max"] and (lo < 4 or hi - lo < lo / 4 + 1)
            assert stats.quantile(name, 1)[1] == t[name]["max"]
        with pytest.raises(ValueError):
            stats.quantile("steps", 0)
