#!/usr/bin/env python3
"""What "which probes did the range reach?" costs.  The library is the one MADSIM_HIP_LIB names (default: this tree's), loaded with ctypes
so that the parent commit's build — which has no madsim_hip_census_range — can be measured too: that process prints the legs it has.

N seeds of the traced lossy ping-pong (two pairs, 16 rounds, loss 0.02, each client tracing 0x10 + pair before its loop and 0x20 + pair
behind it) from seed 1, observation rows of OBS_CAP words:

    run_campaign   madsim_hip_run_campaign over the seeds (no trace build): the untouched path, before and after
    trace_seeds    the only route the parent commit has: madsim_hip_trace_seeds over the same seeds, in as few calls as fit
                   MADSIM_TRACE_MAX_BYTES, every row copied to the host — also the floor the trace launches set
    trace+numpy    ... and the census of the returned rows on the host (numpy: one sort of the (value, row) pairs)
    census         one madsim_hip_census_range call: the same trace launches, the reduction on the device, 64 bytes per distinct value back
                   (MADSIM_HIP_CENSUS_DIRECT=1 in the environment: the fold kernel's direct form instead of the wave accumulator)
    fold:...       the two census kernels alone through madsim_k_launch_census_form, HIP-event time of one launch over 65 536 synthetic rows
                   of 16 observations: a ten-value vocabulary and rows of all-distinct values, in the accumulator and the direct form

The legs alternate inside one sample; one JSON line per leg and sample, then one summary line per leg: median, minimum and maximum.
wall_ms is the call's wall time on the host (every call ends in its own stream synchronisation).

    python tools/census_ab.py [samples] [seeds] [obs_cap]
    MADSIM_HIP_LIB=<parent>/madsim_amd/libmadsim_hip.so python tools/census_ab.py [samples] [seeds] [obs_cap]
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

SEED0, LOSS, MAX_VALUES = 1, 0.02, 4096
KERNEL_ROWS, KERNEL_LEN = 65536, 16


def traced_pingpong(rounds=16):
    wl = W.WorkloadBuilder()
    tasks = []
    for pair in range(2):
        n1, n2 = wl.create_node(), wl.create_node()
        a1, a2 = wl.addr(n1, 1), wl.addr(n2, 1)
        t1 = wl.task(n1)
        t1.bind(a1).sleep(secs=1).trace(0x10 + pair).set(0, rounds)
        top1 = t1.label()
        t1.send_to(a1, a2, 1, W.PING).recv_from(a1, 1).assert_val(W.PONG).djnz(0, top1).trace(0x20 + pair).done()
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


def numpy_census(rows, lens, verdicts, obs_cap):
    """{value: (n_seeds[4], n_total)} of the returned rows: the host's side of the parent's route."""
    vis = np.minimum(lens, obs_cap)
    keep = (np.arange(rows.shape[1], dtype=np.uint64)[None, :] < vis[:, None]) & (verdicts < 4)[:, None]
    r, c = np.nonzero(keep)
    vals = rows[r, c]
    order = np.lexsort((r, vals))
    v, rr = vals[order], r[order]
    first = np.ones(len(v), dtype=bool)
    first[1:] = (v[1:] != v[:-1]) | (rr[1:] != rr[:-1])                      # the first occurrence of a (value, row) pair
    uniq, total = np.unique(v, return_counts=True)
    out = {}
    for k in range(4):
        sel = first & (verdicts[rr] == k)
        u, n = np.unique(v[sel], return_counts=True)
        for x, y in zip(u, n):
            out.setdefault(int(x), [0, 0, 0, 0])[k] = int(y)
    return {int(x): (out[int(x)], int(t)) for x, t in zip(uniq, total)}


def main():
    samples = int(sys.argv[1]) if len(sys.argv) > 1 else 7
    n = int(sys.argv[2]) if len(sys.argv) > 2 else 65536
    obs_cap = int(sys.argv[3]) if len(sys.argv) > 3 else 64
    path = os.environ.get("MADSIM_HIP_LIB", os.path.join(ROOT, "madsim_amd", "libmadsim_hip.so"))
    import torch                                             # (the kernel legs' device buffers; initialised first, as under the test suite, so that
    torch.cuda.init()                                        #  the library binds to the HIP runtime already in the process)
    L = C.CDLL(path)
    u64p, vp, u64, u32 = C.POINTER(C.c_uint64), C.c_void_p, C.c_uint64, C.c_uint32
    head = [C.POINTER(A.Workload), C.POINTER(A.Config)]
    L.madsim_hip_trace_seeds.argtypes = head + [u64p, u64, C.POINTER(A.Limits), vp, u64, vp, u64, vp, vp, vp]
    L.madsim_hip_run_campaign.argtypes = head + [u64, u64, u64, u32, u32, C.POINTER(A.Limits), C.POINTER(A.Campaign)]
    has = hasattr(L, "madsim_hip_census_range")
    if has:
        L.madsim_hip_census_range.argtypes = head + [u64, u64, u64, C.POINTER(A.Limits), C.POINTER(A.Census)]
        L.madsim_k_launch_census_form.argtypes = [vp, u64, vp, vp, vp, u64, u32, vp, u64, vp, u64, vp, vp, vp, C.c_int]
        L.madsim_k_census_slots.argtypes, L.madsim_k_census_slots.restype = [u64], u64
    assert L.madsim_hip_init(0) == 0
    w, lim, cfg = traced_pingpong(), A.Limits(), A.Config.default(packet_loss_rate=LOSS)
    per_call = min(n, A.TRACE_MAX_BYTES // (8 * obs_cap + 72))
    rows, lens, res = np.zeros((n, obs_cap), dtype=np.uint64), np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=A.RESULT_DTYPE)
    seeds = np.arange(SEED0, SEED0 + n, dtype=np.uint64)
    ptr = lambda a: a.ctypes.data_as(vp)                                        # noqa: E731
    values = np.zeros(MAX_VALUES, dtype=A.CENSUS_VALUE_DTYPE)
    form = "direct" if os.environ.get("MADSIM_HIP_CENSUS_DIRECT", "0").strip() not in ("", "0") else "accumulator"

    def run_campaign():
        rep = A.Campaign()
        assert L.madsim_hip_run_campaign(w.ref(), C.byref(cfg), SEED0, n, 0, 0, 0, C.byref(lim), C.byref(rep)) == 0
        return {"n_failed": int(rep.n_failed)}

    def trace_seeds():
        for lo in range(0, n, per_call):
            m = min(per_call, n - lo)
            assert L.madsim_hip_trace_seeds(w.ref(), C.byref(cfg), seeds[lo:].ctypes.data_as(u64p), m, C.byref(lim), None, 0, ptr(rows[lo:]), obs_cap, None,
                                            ptr(lens[lo:]), ptr(res[lo:])) == 0
        return {"calls": -(-n // per_call)}

    def trace_numpy():
        trace_seeds()
        return {"values": len(numpy_census(rows, lens, res["verdict"], obs_cap))}

    def census():
        cen = A.Census(include=0xf, obs_cap=obs_cap, cap=MAX_VALUES)
        cen.values = values.ctypes.data_as(C.POINTER(A.CensusValue))
        assert L.madsim_hip_census_range(w.ref(), C.byref(cfg), SEED0, n, 0, C.byref(lim), C.byref(cen)) == 0
        return {"form": form, "values": int(cen.n_values), "n_counted": [int(x) for x in cen.n_counted], "n_observations": int(cen.n_observations)}

    legs = [("run_campaign", run_campaign), ("trace_seeds", trace_seeds), ("trace+numpy", trace_numpy)] + ([("census", census)] if has else [])
    name_of = os.path.relpath(path, ROOT) if path.startswith(ROOT) else "parent"
    for _, f in legs:
        f()                                                  # warm-up: tables uploaded, buffers allocated, kernels loaded
    if has:                                                  # the two routes agree before either is timed
        host = numpy_census(rows, lens, res["verdict"], obs_cap)
        census()
        dev = {int(e["value"]): ([int(x) for x in e["n_seeds"]], int(e["n_total"])) for e in values[:len(host)]}
        assert dev == host, (dev, host)
    took = {}
    for i in range(samples):
        for name, f in legs:
            t0 = time.perf_counter()
            extra = f()
            ms = (time.perf_counter() - t0) * 1e3
            took.setdefault(name, []).append(ms)
            line = {"lib": name_of, "leg": name, "sample": i, "seeds": n, "obs_cap": obs_cap, "wall_ms": round(ms, 3)}
            line.update(extra)
            print(json.dumps(line), flush=True)
    if has and not os.environ.get("CENSUS_AB_NO_KERNEL_LEGS"):
        R, K = KERNEL_ROWS, KERNEL_LEN
        rng = np.random.default_rng(20261020)
        vocab = rng.integers(0, 1 << 64, 10, dtype=np.uint64)
        inputs = {"ten-values": vocab[rng.integers(0, 10, (R, K))], "all-distinct": (np.arange(R * K, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)).reshape(R, K)}
        st = torch.cuda.current_stream().cuda_stream
        for what, host_rows in inputs.items():
            cap = 16 if what == "ten-values" else R * K
            slots = int(L.madsim_k_census_slots(cap))
            d_rows = torch.from_numpy(host_rows.view(np.int64).copy()).cuda()
            d_len = torch.full((R,), K, dtype=torch.int64, device="cuda")
            d_res = torch.zeros(48 * R, dtype=torch.uint8, device="cuda")
            d_seeds = torch.arange(R, dtype=torch.int64, device="cuda")
            table, lst = torch.zeros(32 * slots, dtype=torch.uint8, device="cuda"), torch.zeros(cap, dtype=torch.int32, device="cuda")
            words, ent = torch.zeros(16, dtype=torch.int64, device="cuda"), torch.zeros(64 * cap, dtype=torch.uint8, device="cuda")
            for direct in (0, 1):
                leg = f"fold:{what}:{'direct' if direct else 'accumulator'}"
                for i in range(-2, samples):                 # (two warm-up launches)
                    words.zero_()
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    assert L.madsim_k_launch_census_form(d_rows.data_ptr(), K, d_len.data_ptr(), d_res.data_ptr(), d_seeds.data_ptr(), R, 0xf, table.data_ptr(),
                                                         slots, lst.data_ptr(), cap, words.data_ptr(), ent.data_ptr(), st, direct) == 0
                    e1.record()
                    torch.cuda.synchronize()
                    got = words.cpu().numpy()
                    assert got[1] == 0 and got[0] == (10 if what == "ten-values" else R * K) and got[11] == R * K, got
                    if i >= 0:
                        ms = e0.elapsed_time(e1)
                        took.setdefault(leg, []).append(ms)
                        print(json.dumps({"lib": name_of, "leg": leg, "sample": i, "rows": R, "row_len": K, "kernel_ms": round(ms, 4)}), flush=True)
    for name, ms in took.items():
        print(json.dumps({"lib": name_of, "summary": name, "seeds": n, "obs_cap": obs_cap, "form": form, "samples": len(ms),
                          "median_ms": round(statistics.median(ms), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3)}), flush=True)
    L.madsim_hip_shutdown()


if __name__ == "__main__":
    main()
