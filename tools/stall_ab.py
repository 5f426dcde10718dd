#!/usr/bin/env python3
"""What "where do the tasks of the failing seeds stand?" costs.  The library is the one MADSIM_HIP_LIB names (default: this tree's), loaded
with ctypes so that the parent commit's build — which has neither madsim_hip_task_states nor madsim_hip_stall_census_range — can be
measured too: that process prints the legs it has.

N seeds of the traced lossy ping-pong of tests/groups_ref.py (two pairs, 16 rounds, loss 0.002, each client tracing its pair number behind
its loop) from seed 5 000 000, task rows of TASK_CAP words:

    trace_floor    madsim_hip_trace_seeds with log_cap 0 and obs_cap 0 over the seeds, in as few calls as fit MADSIM_TRACE_MAX_BYTES: the
                   trace launches and the results alone — the floor, and the untouched path before and after (a null task_log)
    trace_seeds    ... with observation rows of 64 words, every row copied to the host: the untouched path with a log, before and after
    census         madsim_hip_census_range (obs_cap 64): the untouched reduction, before and after
    task_states    madsim_hip_task_states over the same seeds, every task row copied to the host
    rows+numpy     ... and the stall census of the returned rows on the host (numpy: one sort of the (site, row) pairs, one of the shapes):
                   what one would do with the list form alone
    stall_census   one madsim_hip_stall_census_range call: the same trace launches, stall_sites_kernel and the two census passes on the
                   device, 64 bytes per distinct site and shape back

The legs alternate inside one sample; one JSON line per leg and sample, then one summary line per leg: median, minimum and maximum.
wall_ms is the call's wall time on the host (every call ends in its own stream synchronisation).

    python tools/stall_ab.py [samples] [seeds] [task_cap]
    MADSIM_HIP_LIB=<parent>/madsim_amd/libmadsim_hip.so python tools/stall_ab.py [samples] [seeds] [task_cap]
"""
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from madsim_amd import _abi as A  # noqa: E402
from madsim_amd import workload as W  # noqa: E402

SEED0, LOSS, OBS_CAP, MAX_ENTRIES = 5_000_000, 0.002, 64, 4096


def traced_pingpong(rounds=16):
    wl = W.WorkloadBuilder()
    tasks = []
    for pair in range(2):
        n1, n2 = wl.create_node(), wl.create_node()
        a1, a2 = wl.addr(n1, 1), wl.addr(n2, 1)
        t1 = wl.task(n1)
        t1.bind(a1).sleep(secs=1).set(0, rounds)
        top1 = t1.label()
        t1.send_to(a1, a2, 1, W.PING).recv_from(a1, 1).assert_val(W.PONG).djnz(0, top1).trace(pair).done()
        t2 = wl.task(n2)
        t2.bind(a2).set(0, rounds)
        top2 = t2.label()
        t2.recv_from(a2, 1).assert_val(W.PING).reply(a2, 1, W.PONG).djnz(0, top2).done()
        tasks += [t1, t2]
    m = wl.main()
    for t in tasks:
        m.spawn(t)
    for t in tasks:
        m.join(t)
    m.done()
    return wl.build()


def mix(z):
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def numpy_stall_census(rows, lens, verdicts, include, task_cap):
    """({site: (n_seeds[4], n_total)}, {shape: n_seeds[4]}) of the returned rows: the host's side of the list-form route."""
    counted = (verdicts < 4) & (((include >> np.minimum(verdicts, 31)) & 1) != 0)
    vis = np.where(counted, np.minimum(lens, task_cap), 0)
    keep = np.arange(rows.shape[1], dtype=np.uint64)[None, :] < vis[:, None]
    sites = np.where(keep, rows >> np.uint64(32), np.uint64(0))
    with np.errstate(over="ignore"):
        shape = np.where(keep, mix(sites), np.uint64(0)).sum(axis=1, dtype=np.uint64)
    r, c = np.nonzero(keep)
    vals = sites[r, c]
    order = np.lexsort((r, vals))
    v, rr = vals[order], r[order]
    first = np.ones(len(v), dtype=bool)
    first[1:] = (v[1:] != v[:-1]) | (rr[1:] != rr[:-1])
    uniq, total = np.unique(v, return_counts=True)
    by_site = {int(x): [[0, 0, 0, 0], int(t)] for x, t in zip(uniq, total)}
    by_shape = {}
    for k in range(4):
        u, n = np.unique(v[first & (verdicts[rr] == k)], return_counts=True)
        for x, y in zip(u, n):
            by_site[int(x)][0][k] = int(y)
        u, n = np.unique(shape[counted & (verdicts == k)], return_counts=True)
        for x, y in zip(u, n):
            by_shape.setdefault(int(x), [0, 0, 0, 0])[k] = int(y)
    return {k: (v[0], v[1]) for k, v in by_site.items()}, by_shape


def main():
    samples = int(sys.argv[1]) if len(sys.argv) > 1 else 7
    n = int(sys.argv[2]) if len(sys.argv) > 2 else 65536
    task_cap = int(sys.argv[3]) if len(sys.argv) > 3 else 32
    include = 0xe
    path = os.environ.get("MADSIM_HIP_LIB", os.path.join(ROOT, "madsim_amd", "libmadsim_hip.so"))
    L = C.CDLL(path)
    u64p, vp, u64 = C.POINTER(C.c_uint64), C.c_void_p, C.c_uint64
    head = [C.POINTER(A.Workload), C.POINTER(A.Config)]
    L.madsim_hip_trace_seeds.argtypes = head + [u64p, u64, C.POINTER(A.Limits), vp, u64, vp, u64, vp, vp, vp]
    L.madsim_hip_census_range.argtypes = head + [u64, u64, u64, C.POINTER(A.Limits), C.POINTER(A.Census)]
    has = hasattr(L, "madsim_hip_stall_census_range")
    if has:
        L.madsim_hip_task_states.argtypes = head + [u64p, u64, C.POINTER(A.Limits), vp, u64, vp, vp]
        L.madsim_hip_stall_census_range.argtypes = head + [u64, u64, u64, C.POINTER(A.Limits), C.POINTER(A.StallCensus)]
    assert L.madsim_hip_init(0) == 0
    w, lim, cfg = traced_pingpong(), A.Limits(), A.Config.default(packet_loss_rate=LOSS)
    seeds = np.arange(SEED0, SEED0 + n, dtype=np.uint64)
    res = np.zeros(n, dtype=A.RESULT_DTYPE)
    obs, obs_len = np.zeros((n, OBS_CAP), dtype=np.uint64), np.zeros(n, dtype=np.uint64)
    rows, lens = np.zeros((n, task_cap), dtype=np.uint64), np.zeros(n, dtype=np.uint64)
    values = np.zeros(MAX_ENTRIES, dtype=A.CENSUS_VALUE_DTYPE)
    sites, shapes = np.zeros(MAX_ENTRIES, dtype=A.CENSUS_VALUE_DTYPE), np.zeros(MAX_ENTRIES, dtype=A.CENSUS_VALUE_DTYPE)
    ptr = lambda a: a.ctypes.data_as(vp)                                        # noqa: E731

    def in_calls(per_seed_bytes, call):
        per_call = min(n, A.TRACE_MAX_BYTES // per_seed_bytes)
        for lo in range(0, n, per_call):
            assert call(lo, min(per_call, n - lo)) == 0
        return {"calls": -(-n // per_call)}

    def trace_floor():
        return in_calls(72, lambda lo, m: L.madsim_hip_trace_seeds(w.ref(), C.byref(cfg), seeds[lo:].ctypes.data_as(u64p), m, C.byref(lim), None, 0, None, 0,
                                                                   None, None, ptr(res[lo:])))

    def trace_seeds():
        return in_calls(8 * OBS_CAP + 72, lambda lo, m: L.madsim_hip_trace_seeds(w.ref(), C.byref(cfg), seeds[lo:].ctypes.data_as(u64p), m, C.byref(lim), None, 0,
                                                                                 ptr(obs[lo:]), OBS_CAP, None, ptr(obs_len[lo:]), ptr(res[lo:])))

    def census():
        cen = A.Census(include=0xf, obs_cap=OBS_CAP, cap=MAX_ENTRIES)
        cen.values = values.ctypes.data_as(C.POINTER(A.CensusValue))
        assert L.madsim_hip_census_range(w.ref(), C.byref(cfg), SEED0, n, 0, C.byref(lim), C.byref(cen)) == 0
        return {"values": int(cen.n_values), "n_counted": [int(x) for x in cen.n_counted]}

    def task_states():
        return in_calls(8 * task_cap + 72, lambda lo, m: L.madsim_hip_task_states(w.ref(), C.byref(cfg), seeds[lo:].ctypes.data_as(u64p), m, C.byref(lim),
                                                                                  ptr(rows[lo:]), task_cap, ptr(lens[lo:]), ptr(res[lo:])))

    def rows_numpy():
        task_states()
        a, b = numpy_stall_census(rows, lens, res["verdict"], include, task_cap)
        return {"sites": len(a), "shapes": len(b)}

    def stall_census():
        sc = A.StallCensus(include=include, task_cap=task_cap, site_cap=MAX_ENTRIES, shape_cap=MAX_ENTRIES)
        sc.sites, sc.shapes = sites.ctypes.data_as(C.POINTER(A.CensusValue)), shapes.ctypes.data_as(C.POINTER(A.CensusValue))
        assert L.madsim_hip_stall_census_range(w.ref(), C.byref(cfg), SEED0, n, 0, C.byref(lim), C.byref(sc)) == 0
        return {"sites": int(sc.n_sites), "shapes": int(sc.n_shapes), "n_counted": [int(x) for x in sc.n_counted], "n_tasks": int(sc.n_tasks)}

    legs = [("trace_floor", trace_floor), ("trace_seeds", trace_seeds), ("census", census)]
    if has:
        legs += [("task_states", task_states), ("rows+numpy", rows_numpy), ("stall_census", stall_census)]
    name_of = "this commit" if os.path.abspath(path) == os.path.join(ROOT, "madsim_amd", "libmadsim_hip.so") else "parent"
    for _, f in legs:
        f()                                                  # warm-up: tables uploaded, buffers allocated, kernels loaded
    if has:                                                  # the two routes agree before either is timed
        a, b = numpy_stall_census(rows, lens, res["verdict"], include, task_cap)
        got = stall_census()
        dev_a = {int(e["value"]): ([int(x) for x in e["n_seeds"]], int(e["n_total"])) for e in sites[:got["sites"]]}
        dev_b = {int(e["value"]): [int(x) for x in e["n_seeds"]] for e in shapes[:got["shapes"]]}
        assert dev_a == a and dev_b == b, (dev_a, a, dev_b, b)
    took = {}
    for i in range(samples):
        for name, f in legs:
            t0 = time.perf_counter()
            extra = f()
            ms = (time.perf_counter() - t0) * 1e3
            took.setdefault(name, []).append(ms)
            line = {"lib": name_of, "leg": name, "sample": i, "seeds": n, "task_cap": task_cap, "wall_ms": round(ms, 3)}
            line.update(extra)
            print(json.dumps(line), flush=True)
    for name, ms in took.items():
        print(json.dumps({"lib": name_of, "summary": name, "seeds": n, "task_cap": task_cap, "samples": len(ms),
                          "median_ms": round(statistics.median(ms), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3)}), flush=True)
    L.madsim_hip_shutdown()


if __name__ == "__main__":
    main()
