#!/usr/bin/env python3
"""What "how long from this traced value to that one?" costs.  The library is the one MADSIM_HIP_LIB names (default: this tree's), loaded
with ctypes so that the parent commit's build — which has neither madsim_hip_timeline_seeds nor madsim_hip_probe_spans_range — can be
measured too: that process prints the legs it has.

N seeds of the traced lossy ping-pong of tests/spans_workloads.py (two pairs, 16 rounds, loss 0.004; 0x10 + pair before a client's loop,
0x30 + pair in every round, 0x20 + pair behind it) from seed 5 000 000, obs_cap 256, the spans 0x10 -> 0x20, 0x11 -> 0x21, start -> 0x20
and the period 0x30 -> 0x30:

    trace_seeds    madsim_hip_trace_seeds (obs_cap 256, no log), in as few calls as fit MADSIM_TRACE_MAX_BYTES, every row copied to the host:
                   the untouched path, before and after (no time log: obs_time_words 0)
    census         madsim_hip_census_range (obs_cap 256): an untouched reduction, before and after
    probe_order    madsim_hip_probe_order_range over the five probe values: the nearest report, before and after
    stall_census   madsim_hip_stall_census_range (task_cap 32): the other trace launch, before and after
    timeline       madsim_hip_timeline_seeds over the same seeds: both rows of every seed copied to the host — the call probe_spans replaces
    rows+numpy     ... and the spans of the returned rows on the host (numpy, the arithmetic of tests/spans_ref.py)
    probe_spans    one madsim_hip_probe_spans_range call: the same trace launches, span_fold_kernel with its accumulator in LDS and
                   span_witness_kernel, 2 240 bytes per span back
    fold_lds / fold_direct   the two kernels alone (madsim_k_launch_probe_spans_form) over the rows of the first min(N, 65 536) seeds, uploaded
                   once: the workgroup accumulator in LDS against every update sent straight to global memory

The legs alternate inside one sample; one JSON line per leg and sample, then one summary line per leg: median, minimum and maximum.
wall_ms is the call's wall time on the host (every call ends in its own stream synchronisation).

    python tools/spans_ab.py [samples] [seeds]
    MADSIM_HIP_LIB=<parent>/madsim_amd/libmadsim_hip.so python tools/spans_ab.py [samples] [seeds]
"""
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

try:                                                     # (before the library: torch's wheel carries a HIP runtime of its own, and the first one loaded wins)
    import torch
except ImportError:
    torch = None

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from madsim_amd import _abi as A  # noqa: E402
from tests import spans_ref as R  # noqa: E402
from tests import spans_workloads as SW  # noqa: E402

SEED0, OBS_CAP, MAX_ENTRIES, TASK_CAP = 5_000_000, 256, 4096, 32
SPANS = [(0x10, 0x20), (0x11, 0x21), (None, 0x20), (0x30, 0x30)]
VOCAB = [0x10, 0x11, 0x20, 0x21, 0x30]


def main():
    samples = int(sys.argv[1]) if len(sys.argv) > 1 else 7
    n = int(sys.argv[2]) if len(sys.argv) > 2 else 65536
    path = os.environ.get("MADSIM_HIP_LIB", os.path.join(ROOT, "madsim_amd", "libmadsim_hip.so"))
    L = C.CDLL(path)
    u64p, vp, u64, u32 = C.POINTER(C.c_uint64), C.c_void_p, C.c_uint64, C.c_uint32
    head = [C.POINTER(A.Workload), C.POINTER(A.Config)]
    L.madsim_hip_trace_seeds.argtypes = head + [u64p, u64, C.POINTER(A.Limits), vp, u64, vp, u64, vp, vp, vp]
    L.madsim_hip_census_range.argtypes = head + [u64, u64, u64, C.POINTER(A.Limits), C.POINTER(A.Census)]
    L.madsim_hip_probe_order_range.argtypes = head + [u64, u64, u64, C.POINTER(A.Limits), C.POINTER(A.ProbeOrder)]
    L.madsim_hip_stall_census_range.argtypes = head + [u64, u64, u64, C.POINTER(A.Limits), C.POINTER(A.StallCensus)]
    has = hasattr(L, "madsim_hip_probe_spans_range")
    if has:
        L.madsim_hip_timeline_seeds.argtypes = head + [u64p, u64, C.POINTER(A.Limits), vp, vp, u64, vp, vp]
        L.madsim_hip_probe_spans_range.argtypes = head + [u64, u64, u64, C.POINTER(A.Limits), C.POINTER(A.ProbeSpans)]
        L.madsim_k_launch_probe_spans_form.argtypes = [vp, vp, u64, vp, vp, vp, u64, u32, vp, u64, vp, vp, vp, vp, vp, C.c_int]
    assert L.madsim_hip_init(0) == 0
    w, cfg, lim = SW.case("pingpong")
    seeds = np.arange(SEED0, SEED0 + n, dtype=np.uint64)
    res = np.zeros(n, dtype=A.RESULT_DTYPE)
    obs, tim, obs_len = np.zeros((n, OBS_CAP), dtype=np.uint64), np.zeros((n, OBS_CAP), dtype=np.uint64), np.zeros(n, dtype=np.uint64)
    values, pairs = np.zeros(MAX_ENTRIES, dtype=A.CENSUS_VALUE_DTYPE), np.zeros(len(VOCAB) ** 2, dtype=A.PROBE_ORDER_PAIR_DTYPE)
    sites, shapes = np.zeros(MAX_ENTRIES, dtype=A.CENSUS_VALUE_DTYPE), np.zeros(MAX_ENTRIES, dtype=A.CENSUS_VALUE_DTYPE)
    vocab, defs, recs = np.array(VOCAB, dtype=np.uint64), R.defs_of(SPANS), np.zeros(len(SPANS), dtype=A.SPAN_DTYPE)
    ptr = lambda a: a.ctypes.data_as(vp)                                        # noqa: E731

    def in_calls(per_seed_bytes, call):
        per_call = min(n, A.TRACE_MAX_BYTES // per_seed_bytes)
        for lo in range(0, n, per_call):
            assert call(lo, min(per_call, n - lo)) == 0
        return {"calls": -(-n // per_call)}

    def trace_seeds():
        return in_calls(8 * OBS_CAP + 72, lambda lo, m: L.madsim_hip_trace_seeds(w.ref(), C.byref(cfg), seeds[lo:].ctypes.data_as(u64p), m, C.byref(lim), None, 0,
                                                                                 ptr(obs[lo:]), OBS_CAP, None, ptr(obs_len[lo:]), ptr(res[lo:])))

    def census():
        cen = A.Census(include=0xf, obs_cap=OBS_CAP, cap=MAX_ENTRIES)
        cen.values = values.ctypes.data_as(C.POINTER(A.CensusValue))
        assert L.madsim_hip_census_range(w.ref(), C.byref(cfg), SEED0, n, 0, C.byref(lim), C.byref(cen)) == 0
        return {"values": int(cen.n_values), "n_counted": [int(x) for x in cen.n_counted]}

    def probe_order():
        po = A.ProbeOrder(include=0xf, obs_cap=OBS_CAP, n_vocab=len(VOCAB), cap=len(pairs))
        po.vocab, po.pairs = vocab.ctypes.data_as(u64p), pairs.ctypes.data_as(C.POINTER(A.ProbeOrderPair))
        assert L.madsim_hip_probe_order_range(w.ref(), C.byref(cfg), SEED0, n, 0, C.byref(lim), C.byref(po)) == 0
        return {"pairs": int(po.n_pairs)}

    def stall_census():
        sc = A.StallCensus(include=0xe, task_cap=TASK_CAP, site_cap=MAX_ENTRIES, shape_cap=MAX_ENTRIES)
        sc.sites, sc.shapes = sites.ctypes.data_as(C.POINTER(A.CensusValue)), shapes.ctypes.data_as(C.POINTER(A.CensusValue))
        assert L.madsim_hip_stall_census_range(w.ref(), C.byref(cfg), SEED0, n, 0, C.byref(lim), C.byref(sc)) == 0
        return {"sites": int(sc.n_sites)}

    def timeline():
        return in_calls(16 * OBS_CAP + 72, lambda lo, m: L.madsim_hip_timeline_seeds(w.ref(), C.byref(cfg), seeds[lo:].ctypes.data_as(u64p), m, C.byref(lim),
                                                                                     ptr(obs[lo:]), ptr(tim[lo:]), OBS_CAP, ptr(obs_len[lo:]), ptr(res[lo:])))

    def rows_numpy():
        timeline()
        ref = R.report(obs, tim, obs_len, res["verdict"], seeds, defs, 0xf, OBS_CAP)
        return {"closed": [int(x) for x in ref.spans["n"]]}

    def probe_spans():
        ps = A.ProbeSpans(include=0xf, obs_cap=OBS_CAP, n_spans=len(SPANS))
        ps.defs, ps.spans = defs.ctypes.data_as(C.POINTER(A.SpanDef)), recs.ctypes.data_as(C.POINTER(A.Span))
        assert L.madsim_hip_probe_spans_range(w.ref(), C.byref(cfg), SEED0, n, 0, C.byref(lim), C.byref(ps)) == 0
        return {"closed": [int(x) for x in recs["n"]], "n_counted": [int(x) for x in ps.n_counted]}

    legs = [("trace_seeds", trace_seeds), ("census", census), ("probe_order", probe_order), ("stall_census", stall_census)]
    if has:
        legs += [("timeline", timeline), ("rows+numpy", rows_numpy), ("probe_spans", probe_spans)]
    name_of = "this commit" if os.path.abspath(path) == os.path.join(ROOT, "madsim_amd", "libmadsim_hip.so") else "parent"
    for _, f in legs:
        f()                                                  # warm-up: tables uploaded, buffers allocated, kernels loaded
    if has:                                                  # the two routes agree before either is timed; then the kernels' own legs
        assert torch is not None, "the kernels' own legs upload their rows through torch"
        timeline()
        ref = R.report(obs, tim, obs_len, res["verdict"], seeds, defs, 0xf, OBS_CAP)
        probe_spans()
        assert recs.tobytes() == ref.spans.tobytes(), (recs["n"], ref.spans["n"])
        k = min(n, 65536)
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()          # noqa: E731
        d_obs, d_tim, d_len, d_res, d_seeds = up(obs[:k]), up(tim[:k]), up(obs_len[:k]), up(res[:k]), up(seeds[:k])
        m = len(SPANS)
        d_st, d_dur = torch.zeros(4 * k * m, dtype=torch.uint8, device="cuda"), torch.zeros(8 * k * m, dtype=torch.uint8, device="cuda")
        d_recs, d_words = torch.zeros(2240 * m, dtype=torch.uint8, device="cuda"), torch.zeros(64, dtype=torch.uint8, device="cuda")

        def kernels(direct):
            def leg():
                d_words.zero_()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                assert L.madsim_k_launch_probe_spans_form(d_obs.data_ptr(), d_tim.data_ptr(), OBS_CAP, d_len.data_ptr(), d_res.data_ptr(), d_seeds.data_ptr(), k,
                                                          0xf, defs.ctypes.data, m, d_st.data_ptr(), d_dur.data_ptr(), d_recs.data_ptr(), d_words.data_ptr(),
                                                          torch.cuda.current_stream().cuda_stream, direct) == 0
                torch.cuda.synchronize()
                return {"rows": k, "kernel_ms": round((time.perf_counter() - t0) * 1e3, 4)}
            return leg

        legs += [("fold_lds", kernels(0)), ("fold_direct", kernels(1))]
        kernels(0)(), kernels(1)()
    took = {}
    for i in range(samples):
        for name, f in legs:
            t0 = time.perf_counter()
            extra = f()
            ms = extra.get("kernel_ms", (time.perf_counter() - t0) * 1e3)
            took.setdefault(name, []).append(ms)
            line = {"lib": name_of, "leg": name, "sample": i, "seeds": n, "wall_ms": round(ms, 3)}
            line.update(extra)
            print(json.dumps(line), flush=True)
    for name, ms in took.items():
        print(json.dumps({"lib": name_of, "summary": name, "seeds": n, "samples": len(ms), "median_ms": round(statistics.median(ms), 3),
                          "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3)}), flush=True)
    L.madsim_hip_shutdown()


if __name__ == "__main__":
    main()
