#!/usr/bin/env python3
"""What a sweep campaign costs beside the campaigns it replaces.  The library is the one MADSIM_HIP_LIB names (default: this tree's), loaded
with ctypes alone so that the parent commit's build — which has no sweep entry points — can be measured too: that leg then prints the
legs it has.  Every leg runs BATCHES x 65 536 seeds of the headline ping-pong (4 nodes, 64 rounds), 65 536 per batch, the library's own
number of batches in flight; variant v runs under packet loss LOSSES[v].

    range      madsim_hip_run_campaign, loss 0
    diff       madsim_hip_run_campaign_diff under MADSIM_DIFF_ALL, loss 0 against loss 0.002
    sweep2     madsim_hip_run_sweep_campaign of the same two variants under MADSIM_DIFF_ALL, listing what differs
    plain4 / 8 V plain campaigns back to back, one per loss rate: what a user ran to get the failures per setting
    sweep4 / 8 the V-variant sweep under MADSIM_DIFF_VERDICT, listing the mixed seeds

One JSON line per sample: wall_ms is the call's (or the V calls') wall time on the host, kernel_ms the sum of the simulation kernels'
HIP-event durations.

    python tools/sweep_ab.py [samples] [batches]
    MADSIM_HIP_LIB=<parent>/madsim_amd/libmadsim_hip.so python tools/sweep_ab.py [samples] [batches]
"""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("GPU_MAX_HW_QUEUES", "16")             # as madsim_amd/runtime.py sets it before HIP loads
from madsim_amd import _abi as A  # noqa: E402
from madsim_amd import workload as W  # noqa: E402

BATCH, SEED0, LISTED = 65536, 1, 64
LOSSES = (0.0, 0.002, 0.0005, 0.01, 0.001, 0.004, 0.006, 0.008)      # (the first two are the diff's sides; sweep4 / sweep8 take a prefix)


def main():
    samples = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    batches = int(sys.argv[2]) if len(sys.argv) > 2 else 100
    total = batches * BATCH
    path = os.environ.get("MADSIM_HIP_LIB", os.path.join(ROOT, "madsim_amd", "libmadsim_hip.so"))
    L = C.CDLL(path)
    plain = [C.POINTER(A.Workload), C.POINTER(A.Config), C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint32, C.POINTER(A.Limits), C.POINTER(A.Campaign)]
    side = [C.POINTER(A.Workload), C.POINTER(A.Config), C.POINTER(A.Limits)]
    L.madsim_hip_run_campaign.argtypes = plain
    L.madsim_hip_run_campaign_diff.argtypes = side + side + [C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint32, C.POINTER(A.Campaign), C.POINTER(A.Campaign),
                                                             C.POINTER(A.Diff)]
    has_sweep = hasattr(L, "madsim_hip_run_sweep_campaign")
    if has_sweep:
        L.madsim_hip_run_sweep_campaign.argtypes = [C.POINTER(A.SweepVariant), C.c_uint32, C.c_uint64, C.c_uint64, C.POINTER(C.c_uint64), C.c_uint64, C.c_uint32,
                                                    C.c_uint32, C.POINTER(A.Sweep)]
    assert L.madsim_hip_init(0) == 0
    w, lim = W.pingpong(4, 64), A.Limits()
    cfgs = [A.Config.default(packet_loss_rate=p) for p in LOSSES]

    def run_range(v=0):
        rep = A.Campaign()
        assert L.madsim_hip_run_campaign(w.ref(), C.byref(cfgs[v]), SEED0, total, BATCH, 0, 0, C.byref(lim), C.byref(rep)) == 0
        return rep.kernel_ms, int(rep.batches_run), {"failed": [int(rep.n_failed)]}

    def run_plain(V):
        got = [run_range(v) for v in range(V)]
        return sum(g[0] for g in got), got[0][1], {"failed": [g[2]["failed"][0] for g in got]}

    def run_diff():
        ra, rb, d = A.Campaign(), A.Campaign(), A.Diff()
        rec = np.zeros(LISTED, dtype=A.DIFF_RECORD_DTYPE)
        d.fields, d.cap, d.records = A.DIFF_ALL, LISTED, rec.ctypes.data_as(C.POINTER(A.DiffRecord))
        assert L.madsim_hip_run_campaign_diff(w.ref(), C.byref(cfgs[0]), C.byref(lim), w.ref(), C.byref(cfgs[1]), C.byref(lim), SEED0, total, BATCH, 0, 0,
                                              C.byref(ra), C.byref(rb), C.byref(d)) == 0
        return ra.kernel_ms + rb.kernel_ms, int(ra.batches_run), {"failed": [int(ra.n_failed), int(rb.n_failed)], "differ": int(d.n_differ)}

    def run_sweep(V, fields, rule):
        var, reps, s = (A.SweepVariant * V)(), [A.Campaign() for _ in range(V)], A.Sweep()
        for v in range(V):
            var[v].w, var[v].cfg, var[v].lim, var[v].out = C.pointer(w.struct), C.pointer(cfgs[v]), C.pointer(lim), C.pointer(reps[v])
        rec = np.zeros(LISTED, dtype=A.SWEEP_RECORD_DTYPE)
        s.fields, s.list_rule, s.cap, s.records = fields, rule, LISTED, rec.ctypes.data_as(C.POINTER(A.SweepRecord))
        assert L.madsim_hip_run_sweep_campaign(var, V, SEED0, total, None, BATCH, 0, 0, C.byref(s)) == 0
        return sum(r.kernel_ms for r in reps), int(reps[0].batches_run), {"failed": [int(r.n_failed) for r in reps], "selected": int(s.n_selected),
                                                                          "differ": [int(x) for x in s.n_differ_from_first[:V]]}

    legs = [("range", run_range), ("diff", run_diff), ("plain4", lambda: run_plain(4)), ("plain8", lambda: run_plain(8))]
    if has_sweep:
        legs += [("sweep2", lambda: run_sweep(2, A.DIFF_ALL, A.SWEEP_LIST_DIFFERING)), ("sweep4", lambda: run_sweep(4, A.DIFF_VERDICT, A.SWEEP_LIST_MIXED)),
                 ("sweep8", lambda: run_sweep(8, A.DIFF_VERDICT, A.SWEEP_LIST_MIXED))]
    for _, f in legs:
        f()                                                  # warm-up: tables uploaded, buffers allocated, kernels loaded
    for i in range(samples):
        for name, f in legs:
            t0 = time.perf_counter()
            kernel_ms, n_batches, extra = f()
            line = {"lib": os.path.relpath(path, ROOT) if path.startswith(ROOT) else "parent", "leg": name, "sample": i,
                    "wall_ms": round((time.perf_counter() - t0) * 1e3, 3), "kernel_ms": round(kernel_ms, 3), "batches": n_batches}
            line.update(extra)
            print(json.dumps(line), flush=True)
    L.madsim_hip_shutdown()


if __name__ == "__main__":
    main()
