#!/usr/bin/env python3
"""What a paired campaign costs beside the differential campaign it extends.  The library is the one MADSIM_HIP_LIB names (default: this
tree's), loaded with ctypes alone so that the parent commit's build — which has no paired entry points — can be measured too: that leg
then prints the legs it has.  Every leg runs BATCHES x 65 536 seeds of the headline ping-pong (4 nodes, 64 rounds), 65 536 per batch, the
library's own number of batches in flight; side A under the default send latency (1 .. 10 ms), side B under 2 .. 10 ms.

    range          madsim_hip_run_campaign, side A's config
    diff           madsim_hip_run_campaign_diff under MADSIM_DIFF_ALL, 64 records
    paired0 / 16   madsim_hip_run_paired_campaign, include PASS on both sides, top_k 0 / 16, no diff report
    paired0d / 16d the same with the diff report of the `diff` leg beside it

One JSON line per sample: wall_ms is the call's wall time on the host, kernel_ms the sum of the simulation kernels' HIP-event durations,
report_bytes what a batch's one report copy carries.

    python tools/paired_ab.py [samples] [batches]
    MADSIM_HIP_LIB=<parent>/madsim_amd/libmadsim_hip.so python tools/paired_ab.py [samples] [batches]
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
DIFF_REP_WORDS, PAIRED_WORDS, PAIRED_TOP_WORDS = 64 + 74, 1466, 8 * 16 * 3      # csrc/madsim_hip.cpp, csrc/sim_kernel.h


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
    has_paired = hasattr(L, "madsim_hip_run_paired_campaign")
    if has_paired:
        L.madsim_hip_run_paired_campaign.argtypes = L.madsim_hip_run_campaign_diff.argtypes + [C.POINTER(A.Paired)]
    assert L.madsim_hip_init(0) == 0
    w, lim = W.pingpong(4, 64), A.Limits()
    cfg_a, cfg_b = A.Config.default(), A.Config.default(lat_lo_ns=2_000_000, lat_hi_ns=10_000_000)

    def run_range():
        rep = A.Campaign()
        assert L.madsim_hip_run_campaign(w.ref(), C.byref(cfg_a), SEED0, total, BATCH, 0, 0, C.byref(lim), C.byref(rep)) == 0
        return rep.kernel_ms, int(rep.batches_run), {"failed": [int(rep.n_failed)], "report_bytes": 8 * 6}

    def new_diff():
        d = A.Diff()
        d._rec = np.zeros(LISTED, dtype=A.DIFF_RECORD_DTYPE)
        d.fields, d.cap, d.records = A.DIFF_ALL, LISTED, d._rec.ctypes.data_as(C.POINTER(A.DiffRecord))
        return d

    def run_diff():
        ra, rb, d = A.Campaign(), A.Campaign(), new_diff()
        assert L.madsim_hip_run_campaign_diff(w.ref(), C.byref(cfg_a), C.byref(lim), w.ref(), C.byref(cfg_b), C.byref(lim), SEED0, total, BATCH, 0, 0,
                                              C.byref(ra), C.byref(rb), C.byref(d)) == 0
        return ra.kernel_ms + rb.kernel_ms, int(ra.batches_run), {"failed": [int(ra.n_failed), int(rb.n_failed)], "differ": int(d.n_differ),
                                                                 "report_bytes": 8 * DIFF_REP_WORDS}

    def run_paired(top_k, with_diff):
        ra, rb, pr = A.Campaign(), A.Campaign(), A.Paired()
        d = new_diff() if with_diff else None
        top = np.zeros((4, 2, top_k), dtype=A.PAIRED_EXTREME_DTYPE)
        pr.include_a = pr.include_b = 1 << A.PASS
        pr.top_k, pr.top = top_k, top.ctypes.data_as(C.POINTER(A.PairedExtreme)) if top_k else None
        assert L.madsim_hip_run_paired_campaign(w.ref(), C.byref(cfg_a), C.byref(lim), w.ref(), C.byref(cfg_b), C.byref(lim), SEED0, total, BATCH, 0, 0,
                                                C.byref(ra), C.byref(rb), C.byref(d) if with_diff else None, C.byref(pr)) == 0
        up, down = pr.delta[0], pr.delta[1]
        net = ((int(up.sum_hi) << 64) | int(up.sum_lo)) - ((int(down.sum_hi) << 64) | int(down.sum_lo))
        extra = {"failed": [int(ra.n_failed), int(rb.n_failed)], "paired": int(pr.n_paired), "clock_up_down_equal": [int(pr.n[0]), int(pr.n[1]), int(pr.n_equal[0])],
                 "clock_net_ns": net, "report_bytes": 8 * (DIFF_REP_WORDS + PAIRED_WORDS - (0 if top_k else PAIRED_TOP_WORDS))}
        if with_diff:
            extra["differ"] = int(d.n_differ)
        return ra.kernel_ms + rb.kernel_ms, int(ra.batches_run), extra

    legs = [("range", run_range), ("diff", run_diff)]
    if has_paired:
        legs += [("paired0", lambda: run_paired(0, False)), ("paired16", lambda: run_paired(16, False)), ("paired0d", lambda: run_paired(0, True)),
                 ("paired16d", lambda: run_paired(16, True))]
    for _, f in legs:
        f()                                                  # warm-up: tables uploaded, buffers allocated, kernels loaded
    for i in range(samples):
        for name, f in legs:
            t0 = time.perf_counter()
            kernel_ms, n_batches, extra = f()
            line = {"lib": os.path.relpath(path, ROOT) if path.startswith(ROOT) and "parent" not in path else "parent", "leg": name, "sample": i,
                    "wall_ms": round((time.perf_counter() - t0) * 1e3, 3), "kernel_ms": round(kernel_ms, 3), "batches": n_batches}
            line.update(extra)
            print(json.dumps(line), flush=True)
    L.madsim_hip_shutdown()


if __name__ == "__main__":
    main()
