#!/usr/bin/env python3
"""Wall time of replaying 256 seeds of the traced lossy ping-pong on the trace build: one madsim_hip_trace_seeds call (obs_cap 64, log_cap 0)
against 256 madsim_hip_trace_seed calls (no log buffer: the leanest form of the per-seed path).  The library is the one MADSIM_HIP_LIB names
(default: this tree's), loaded with ctypes alone so that a build without madsim_hip_trace_seeds — the parent commit's — can be measured too:
that leg then prints the per-seed path only.  One JSON line per sample.

    python tools/observe_ab.py [samples]                                   # this commit: both paths
    MADSIM_HIP_LIB=<parent>/madsim_amd/libmadsim_hip.so python tools/observe_ab.py [samples]
"""
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from madsim_amd import _abi as A  # noqa: E402
from tests import groups_ref as G  # noqa: E402

N, OBS_CAP = 256, 64


def main():
    samples = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    path = os.environ.get("MADSIM_HIP_LIB", os.path.join(ROOT, "madsim_amd", "libmadsim_hip.so"))
    L = C.CDLL(path)
    L.madsim_hip_trace_seed.restype = C.c_int64
    L.madsim_hip_trace_seed.argtypes = [C.POINTER(A.Workload), C.POINTER(A.Config), C.c_uint64, C.POINTER(A.Limits), C.c_void_p, C.c_uint64,
                                        C.POINTER(A.Result)]
    has_list = hasattr(L, "madsim_hip_trace_seeds")
    if has_list:
        L.madsim_hip_trace_seeds.argtypes = [C.POINTER(A.Workload), C.POINTER(A.Config), C.POINTER(C.c_uint64), C.c_uint64, C.POINTER(A.Limits),
                                             C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p]
    assert L.madsim_hip_init(0) == 0
    w, cfg, lim = G.traced_pingpong_workload(), A.Config.default(packet_loss_rate=G.LOSS), A.Limits()
    seeds = (C.c_uint64 * N)(*range(G.SEED0, G.SEED0 + N))
    res, one = (A.Result * N)(), A.Result()
    obs, olen = (C.c_uint64 * (N * OBS_CAP))(), (C.c_uint64 * N)()

    def per_seed():
        for s in seeds:
            assert L.madsim_hip_trace_seed(w.ref(), C.byref(cfg), s, C.byref(lim), None, 0, C.byref(one)) >= 0

    def one_call():
        assert L.madsim_hip_trace_seeds(w.ref(), C.byref(cfg), seeds, N, C.byref(lim), None, 0, obs, OBS_CAP, None, olen, res) == 0

    legs = [("256 x madsim_hip_trace_seed", per_seed)] + ([("madsim_hip_trace_seeds(256)", one_call)] if has_list else [])
    for _, f in legs:
        f()                                                  # warm-up: tables uploaded, buffers allocated, kernels loaded
    for i in range(samples):
        for name, f in legs:
            t0 = time.perf_counter()
            f()
            print(json.dumps({"lib": os.path.relpath(path, ROOT) if path.startswith(ROOT) else "parent", "leg": name, "sample": i,
                              "wall_ms": round((time.perf_counter() - t0) * 1e3, 3)}), flush=True)
    L.madsim_hip_shutdown()


if __name__ == "__main__":
    main()
