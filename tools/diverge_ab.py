#!/usr/bin/env python3
"""What "where do the two runs part?" costs.  The library is the one MADSIM_HIP_LIB names (default: this tree's), loaded with ctypes so
that the parent commit's build — which has no madsim_hip_diverge_seeds — can be measured too: that process then prints the legs it has.

N seeds of the headline ping-pong (4 nodes, 64 rounds), loss 0 (side A) against loss 0.002 (side B), log_cap 16 384, obs_cap 256:

    trace_a      one madsim_hip_trace_seeds call of side A, rows copied back: the untouched path, before and after
    two_traces   the only route the parent commit has: two madsim_hip_trace_seeds calls with both sides' rows copied to the host ...
    two_traces+compare   ... and the host compare of the rows (numpy: first differing index per row, both channels)
    diverge      one madsim_hip_diverge_seeds call (window 4): the same two trace launches, the compare on the device, ~200 bytes per seed back
    kernel       diverge_kernel alone at its worst case, through madsim_k_launch_diverge: ROWS all-equal row pairs of full length, so every
                 byte of both sides is read; HIP-event time of one launch, and the bytes read over it as GB/s (beside tools/ubench_issue's
                 float4 read rate of the same box)

The legs alternate inside one sample; one JSON line per leg and sample.  wall_ms is the call's wall time on the host (every call ends in
its own stream synchronisation).

    python tools/diverge_ab.py [samples] [seeds]
    MADSIM_HIP_LIB=<parent>/madsim_amd/libmadsim_hip.so python tools/diverge_ab.py [samples] [seeds]
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

SEED0, LOSS, LOG_CAP, OBS_CAP, WIN = 1, 0.002, 16384, 256, 4
KERNEL_ROWS = 16384                                          # 2 x 16 384 x (16 384 + 8 x 256) bytes = 604 MB read: more than the last-level cache


def first_difference(a, b, la, lb):
    """The host compare of the parent's route: per row the first index < min(len_a, len_b, cap) at which the rows differ, or that bound."""
    m = np.minimum(np.minimum(la, lb), a.shape[1])
    ne = (a != b) & (np.arange(a.shape[1], dtype=np.uint64)[None, :] < m[:, None])
    return np.where(ne.any(axis=1), ne.argmax(axis=1), m)


def main():
    samples = int(sys.argv[1]) if len(sys.argv) > 1 else 7
    n = int(sys.argv[2]) if len(sys.argv) > 2 else 4096
    path = os.environ.get("MADSIM_HIP_LIB", os.path.join(ROOT, "madsim_amd", "libmadsim_hip.so"))
    import torch                                             # (the kernel leg's device buffers; initialised first, as under the test suite, so that
    torch.cuda.init()                                        #  the library binds to the HIP runtime already in the process)
    L = C.CDLL(path)
    u64p, vp = C.POINTER(C.c_uint64), C.c_void_p
    side = [C.POINTER(A.Workload), C.POINTER(A.Config), C.POINTER(A.Limits)]
    L.madsim_hip_trace_seeds.argtypes = [C.POINTER(A.Workload), C.POINTER(A.Config), u64p, C.c_uint64, C.POINTER(A.Limits), vp, C.c_uint64, vp, C.c_uint64,
                                         vp, vp, vp]
    has = hasattr(L, "madsim_hip_diverge_seeds")
    if has:
        L.madsim_hip_diverge_seeds.argtypes = side + side + [u64p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint32, vp, vp]
        L.madsim_k_launch_diverge.argtypes = [vp, vp, C.c_uint64, vp, vp, C.c_uint64, vp, vp, vp, vp, vp, vp, vp, C.c_uint64, C.c_uint32, vp, vp, vp]
    assert L.madsim_hip_init(0) == 0
    w, lim = W.pingpong(4, 64), A.Limits()
    cfg = [A.Config.default(packet_loss_rate=0.0), A.Config.default(packet_loss_rate=LOSS)]
    seeds = np.arange(SEED0, SEED0 + n, dtype=np.uint64)
    sp = seeds.ctypes.data_as(u64p)
    logs = [np.zeros((n, LOG_CAP), dtype=np.uint8) for _ in range(2)]
    obs = [np.zeros((n, OBS_CAP), dtype=np.uint64) for _ in range(2)]
    llen, olen = [np.zeros(n, dtype=np.uint64) for _ in range(2)], [np.zeros(n, dtype=np.uint64) for _ in range(2)]
    res = [np.zeros(n, dtype=A.RESULT_DTYPE) for _ in range(2)]
    recs, rows = np.zeros(n, dtype=A.DIVERGENCE_DTYPE), np.zeros((n, 3 * WIN), dtype=np.uint64)
    ptr = lambda a: a.ctypes.data_as(vp)                                        # noqa: E731

    def trace(s):
        assert L.madsim_hip_trace_seeds(w.ref(), C.byref(cfg[s]), sp, n, C.byref(lim), ptr(logs[s]), LOG_CAP, ptr(obs[s]), OBS_CAP, ptr(llen[s]),
                                        ptr(olen[s]), ptr(res[s])) == 0

    def trace_a():
        trace(0)
        return {"log_bytes": int(llen[0].sum())}

    def two_traces():
        trace(0); trace(1)
        return {}

    def two_traces_compare():
        trace(0); trace(1)
        at = first_difference(logs[0], logs[1], llen[0], llen[1])
        first_difference(obs[0], obs[1], olen[0], olen[1])
        return {"differ": int((at < np.minimum(np.minimum(llen[0], llen[1]), LOG_CAP)).sum())}

    def diverge():
        assert L.madsim_hip_diverge_seeds(w.ref(), C.byref(cfg[0]), C.byref(lim), w.ref(), C.byref(cfg[1]), C.byref(lim), sp, n, LOG_CAP, OBS_CAP, WIN,
                                          ptr(recs), ptr(rows)) == 0
        return {"differ": int((recs["log_status"] == A.DIVERGE_DIFFER).sum()), "same": int((recs["log_status"] == A.DIVERGE_SAME).sum()),
                "prefix": int((recs["log_status"] == A.DIVERGE_PREFIX).sum()), "beyond_cap": int((recs["log_status"] == A.DIVERGE_BEYOND_CAP).sum())}

    legs = [("trace_a", trace_a), ("two_traces", two_traces), ("two_traces+compare", two_traces_compare)] + ([("diverge", diverge)] if has else [])
    name_of = os.path.relpath(path, ROOT) if path.startswith(ROOT) else "parent"
    for _, f in legs:
        f()                                                  # warm-up: tables uploaded, buffers allocated, kernels loaded
    if has:                                                  # the two routes agree before either is timed
        at = first_difference(logs[0], logs[1], llen[0], llen[1])
        hit = at < np.minimum(np.minimum(llen[0], llen[1]), LOG_CAP)
        assert ((recs["log_status"] == A.DIVERGE_DIFFER) == hit).all() and (recs["log_at"][hit] == at[hit]).all()
    for i in range(samples):
        for name, f in legs:
            t0 = time.perf_counter()
            extra = f()
            line = {"lib": name_of, "leg": name, "sample": i, "seeds": n, "wall_ms": round((time.perf_counter() - t0) * 1e3, 3)}
            line.update(extra)
            print(json.dumps(line), flush=True)
    if has:
        R = KERNEL_ROWS
        dev = lambda nbytes, fill: torch.full((nbytes,), fill, dtype=torch.uint8, device="cuda")      # noqa: E731
        la, lb, oa, ob = dev(R * LOG_CAP, 7), dev(R * LOG_CAP, 7), dev(8 * R * OBS_CAP, 9), dev(8 * R * OBS_CAP, 9)
        ll = torch.full((R,), LOG_CAP, dtype=torch.int64, device="cuda")
        ol = torch.full((R,), OBS_CAP, dtype=torch.int64, device="cuda")
        rs, sd = dev(48 * R, 0), dev(8 * R, 1)
        out, ctx = dev(184 * R, 0), dev(24 * WIN * R, 0)
        bytes_read = 2 * R * (LOG_CAP + 8 * OBS_CAP)
        st = torch.cuda.current_stream().cuda_stream

        def launch():
            assert L.madsim_k_launch_diverge(la.data_ptr(), lb.data_ptr(), LOG_CAP, oa.data_ptr(), ob.data_ptr(), OBS_CAP, ll.data_ptr(), ll.data_ptr(),
                                             ol.data_ptr(), ol.data_ptr(), rs.data_ptr(), rs.data_ptr(), sd.data_ptr(), R, WIN, out.data_ptr(), ctx.data_ptr(),
                                             st) == 0
        for _ in range(3):
            launch()
        torch.cuda.synchronize()
        for i in range(samples):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); launch(); e1.record(); torch.cuda.synchronize()
            ms = e0.elapsed_time(e1)
            print(json.dumps({"lib": name_of, "leg": "kernel", "sample": i, "rows": R, "kernel_ms": round(ms, 4), "bytes_read": bytes_read,
                              "gb_s": round(bytes_read / (ms * 1e-3) / 1e9, 1)}), flush=True)
        status = out.cpu().numpy().view(A.DIVERGENCE_DTYPE)
        assert (status["log_status"] == A.DIVERGE_SAME).all() and (status["log_at"] == LOG_CAP).all() and (status["obs_at"] == OBS_CAP).all()
    L.madsim_hip_shutdown()


if __name__ == "__main__":
    main()
