#!/usr/bin/env python3
"""What "which probe came first?" costs.  The library is the one MADSIM_HIP_LIB names (default: this tree's), loaded with ctypes so that the
parent commit's build — which has no madsim_hip_probe_order_range — can be measured too: that process prints the legs it has.

N seeds of the traced lossy ping-pong (tools/census_ab.py's: two pairs, 16 rounds, loss 0.02, each client tracing 0x10 + pair before its
loop and 0x20 + pair behind it) from seed 1, observation rows of OBS_CAP words, vocabulary (0x10, 0x11, 0x20, 0x21, 0x30):

    run_campaign   madsim_hip_run_campaign over the seeds (no trace build): the untouched path, before and after
    census         one madsim_hip_census_range call: the untouched path, before and after
    probe_sets     one madsim_hip_probe_sets_range call with the same vocabulary: the untouched path, and the nearest yardstick (c)
    trace_seeds    (a) the only route the parent commit has: madsim_hip_trace_seeds over the same seeds, in as few calls as fit
                   MADSIM_TRACE_MAX_BYTES, every row copied to the host — also the floor the trace launches set
    trace+numpy    (b) ... and the first-occurrence arithmetic on the returned rows on the host (numpy: one compare of the rows per
                   vocabulary value, an argmax, one comparison of firsts per cell)
    probe_order    one madsim_hip_probe_order_range call: the same trace launches, the reduction on the device, 72 bytes per cell back
    fold:...       (d) the two probe-order kernels alone through madsim_k_launch_probe_order_form, HIP-event time of one launch over
                   65 536 synthetic rows of 64 observations under a vocabulary of 32: all rows identical (every row on the same 528
                   cells) and random rows (each its own permutation), with the workgroup accumulator in LDS and with every update
                   straight to the global matrix

The legs alternate inside one sample; one JSON line per leg and sample, then one summary line per leg: median, minimum and maximum.
wall_ms is the call's wall time on the host (every call ends in its own stream synchronisation).  With a fourth argument the summary
lines are also written there as a markdown table.

    python tools/order_ab.py [samples] [seeds] [obs_cap] [summary.md]
    MADSIM_HIP_LIB=<parent>/madsim_amd/libmadsim_hip.so python tools/order_ab.py [samples] [seeds] [obs_cap] [summary.md]
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
sys.path.insert(0, os.path.join(ROOT, "tools"))
from madsim_amd import _abi as A  # noqa: E402
from census_ab import traced_pingpong  # noqa: E402

SEED0, LOSS, MAX_SETS, MAX_VALUES = 1, 0.02, 4096, 4096
VOCAB = (0x10, 0x11, 0x20, 0x21, 0x30)
KERNEL_ROWS, KERNEL_LEN, KERNEL_VOCAB = 65536, 64, 32


def numpy_order(rows, lens, verdicts, obs_cap):
    """{(a, b): n_seeds[4]} of the returned rows: the host's side of the parent's route."""
    vis = np.minimum(lens, obs_cap)
    visible = np.arange(rows.shape[1], dtype=np.uint64)[None, :] < vis[:, None]
    first = np.full((len(rows), len(VOCAB)), 1 << 62, dtype=np.int64)
    for j, v in enumerate(VOCAB):
        hit = (rows == np.uint64(v)) & visible
        first[:, j] = np.where(hit.any(axis=1), hit.argmax(axis=1), 1 << 62)
    have = first < 1 << 62
    out = {}
    for a in range(len(VOCAB)):
        for b in range(len(VOCAB)):
            rel = have[:, a] if a == b else have[:, a] & have[:, b] & (first[:, a] < first[:, b])
            n = [int((rel & (verdicts == k)).sum()) for k in range(4)]
            if any(n):
                out[(a, b)] = n
    return out


def main():
    samples = int(sys.argv[1]) if len(sys.argv) > 1 else 7
    n = int(sys.argv[2]) if len(sys.argv) > 2 else 65536
    obs_cap = int(sys.argv[3]) if len(sys.argv) > 3 else 256
    md = sys.argv[4] if len(sys.argv) > 4 else None
    path = os.environ.get("MADSIM_HIP_LIB", os.path.join(ROOT, "madsim_amd", "libmadsim_hip.so"))
    import torch                                             # (the kernel legs' device buffers; initialised first, as under the test suite, so that
    torch.cuda.init()                                        #  the library binds to the HIP runtime already in the process)
    L = C.CDLL(path)
    u64p, vp, u64, u32 = C.POINTER(C.c_uint64), C.c_void_p, C.c_uint64, C.c_uint32
    head = [C.POINTER(A.Workload), C.POINTER(A.Config)]
    L.madsim_hip_trace_seeds.argtypes = head + [u64p, u64, C.POINTER(A.Limits), vp, u64, vp, u64, vp, vp, vp]
    L.madsim_hip_run_campaign.argtypes = head + [u64, u64, u64, u32, u32, C.POINTER(A.Limits), C.POINTER(A.Campaign)]
    L.madsim_hip_census_range.argtypes = head + [u64, u64, u64, C.POINTER(A.Limits), C.POINTER(A.Census)]
    L.madsim_hip_probe_sets_range.argtypes = head + [u64, u64, u64, C.POINTER(A.Limits), C.POINTER(A.ProbeSets)]
    has = hasattr(L, "madsim_hip_probe_order_range")
    if has:
        L.madsim_hip_probe_order_range.argtypes = head + [u64, u64, u64, C.POINTER(A.Limits), C.POINTER(A.ProbeOrder)]
        L.madsim_k_launch_probe_order_form.argtypes = [vp, u64, vp, vp, vp, u64, u32, vp, u64, vp, vp, vp, vp, C.c_int]
    assert L.madsim_hip_init(0) == 0
    w, lim, cfg = traced_pingpong(), A.Limits(), A.Config.default(packet_loss_rate=LOSS)
    per_call = min(n, A.TRACE_MAX_BYTES // (8 * obs_cap + 72))
    rows, lens, res = np.zeros((n, obs_cap), dtype=np.uint64), np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=A.RESULT_DTYPE)
    seeds = np.arange(SEED0, SEED0 + n, dtype=np.uint64)
    ptr = lambda a: a.ctypes.data_as(vp)                                        # noqa: E731
    values, sets, vocab = np.zeros(MAX_VALUES, dtype=A.CENSUS_VALUE_DTYPE), np.zeros(MAX_SETS, dtype=A.PROBE_SET_DTYPE), np.array(VOCAB, dtype=np.uint64)
    pairs = np.zeros(len(VOCAB) ** 2, dtype=A.PROBE_ORDER_PAIR_DTYPE)

    def run_campaign():
        rep = A.Campaign()
        assert L.madsim_hip_run_campaign(w.ref(), C.byref(cfg), SEED0, n, 0, 0, 0, C.byref(lim), C.byref(rep)) == 0
        return {"n_failed": int(rep.n_failed)}

    def census():
        cen = A.Census(include=0xf, obs_cap=obs_cap, cap=MAX_VALUES)
        cen.values = values.ctypes.data_as(C.POINTER(A.CensusValue))
        assert L.madsim_hip_census_range(w.ref(), C.byref(cfg), SEED0, n, 0, C.byref(lim), C.byref(cen)) == 0
        return {"values": int(cen.n_values)}

    def probe_sets():
        ps = A.ProbeSets(include=0xf, obs_cap=obs_cap, n_vocab=len(vocab), cap=MAX_SETS)
        ps.vocab, ps.sets = vocab.ctypes.data_as(u64p), sets.ctypes.data_as(C.POINTER(A.ProbeSet))
        assert L.madsim_hip_probe_sets_range(w.ref(), C.byref(cfg), SEED0, n, 0, C.byref(lim), C.byref(ps)) == 0
        return {"sets": int(ps.n_sets)}

    def trace_seeds():
        for lo in range(0, n, per_call):
            m = min(per_call, n - lo)
            assert L.madsim_hip_trace_seeds(w.ref(), C.byref(cfg), seeds[lo:].ctypes.data_as(u64p), m, C.byref(lim), None, 0, ptr(rows[lo:]), obs_cap, None,
                                            ptr(lens[lo:]), ptr(res[lo:])) == 0
        return {"calls": -(-n // per_call)}

    def trace_numpy():
        trace_seeds()
        return {"cells": len(numpy_order(rows, lens, res["verdict"], obs_cap))}

    def probe_order():
        po = A.ProbeOrder(include=0xf, obs_cap=obs_cap, n_vocab=len(vocab), cap=len(pairs))
        po.vocab, po.pairs = vocab.ctypes.data_as(u64p), pairs.ctypes.data_as(C.POINTER(A.ProbeOrderPair))
        assert L.madsim_hip_probe_order_range(w.ref(), C.byref(cfg), SEED0, n, 0, C.byref(lim), C.byref(po)) == 0
        return {"cells": int(po.n_pairs), "n_counted": [int(x) for x in po.n_counted]}

    legs = [("run_campaign", run_campaign), ("census", census), ("probe_sets", probe_sets), ("trace_seeds", trace_seeds), ("trace+numpy", trace_numpy)]
    legs += [("probe_order", probe_order)] if has else []
    name_of = os.path.relpath(path, ROOT) if path.startswith(ROOT) else "parent"
    for _, f in legs:
        f()                                                  # warm-up: tables uploaded, buffers allocated, kernels loaded
    if has:                                                  # the two routes agree before either is timed
        host = numpy_order(rows, lens, res["verdict"], obs_cap)
        got = probe_order()
        dev = {(int(e["a"]), int(e["b"])): [int(x) for x in e["n_seeds"]] for e in pairs[:got["cells"]]}
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
    if has and not os.environ.get("ORDER_AB_NO_KERNEL_LEGS"):
        R, K, M = KERNEL_ROWS, KERNEL_LEN, KERNEL_VOCAB
        rng = np.random.default_rng(20261022)
        kv = np.arange(1, M + 1, dtype=np.uint64) * np.uint64(0x0101010101010101)
        one = np.concatenate([kv[::-1], np.full(K - M, 0xF0F0, dtype=np.uint64)])
        perm = np.full((R, K), 0xF0F0, dtype=np.uint64)
        perm[:, :M] = kv[np.argsort(rng.random((R, M)), axis=1)]
        inputs = {"identical": np.tile(one, (R, 1)), "random": perm}
        st = torch.cuda.current_stream().cuda_stream
        for what, host_rows in inputs.items():
            d_rows = torch.from_numpy(np.ascontiguousarray(host_rows).view(np.int64).copy()).cuda()
            d_len = torch.full((R,), K, dtype=torch.int64, device="cuda")
            d_res = torch.zeros(48 * R, dtype=torch.uint8, device="cuda")
            d_seeds = torch.arange(R, dtype=torch.int64, device="cuda")
            matrix = torch.zeros(8192, dtype=torch.int32, device="cuda")
            words, ent = torch.zeros(12, dtype=torch.int64, device="cuda"), torch.zeros(72 * M * M, dtype=torch.uint8, device="cuda")
            n_cells = M * (M + 1) // 2 if what == "identical" else M * M
            for direct in (0, 1):
                leg = f"fold:{what}:{'direct' if direct else 'lds'}"
                for i in range(-2, samples):                 # (two warm-up launches)
                    words.zero_()
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    assert L.madsim_k_launch_probe_order_form(d_rows.data_ptr(), K, d_len.data_ptr(), d_res.data_ptr(), d_seeds.data_ptr(), R, 0xf, kv.ctypes.data,
                                                              M, matrix.data_ptr(), words.data_ptr(), ent.data_ptr(), st, direct) == 0
                    e1.record()
                    torch.cuda.synchronize()
                    got = words.cpu().numpy()
                    assert got[1] == 0 and got[0] == n_cells and got[2] == R, got
                    if i >= 0:
                        ms = e0.elapsed_time(e1)
                        took.setdefault(leg, []).append(ms)
                        print(json.dumps({"lib": name_of, "leg": leg, "sample": i, "rows": R, "row_len": K, "vocab": M, "kernel_ms": round(ms, 4)}), flush=True)
    table = ["| lib | leg | seeds | obs_cap | samples | median ms | min ms | max ms |", "|---|---|---|---|---|---|---|---|"]
    for name, ms in took.items():
        s = {"lib": name_of, "summary": name, "seeds": n, "obs_cap": obs_cap, "samples": len(ms), "median_ms": round(statistics.median(ms), 3),
             "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3)}
        print(json.dumps(s), flush=True)
        table.append(f"| {name_of} | {name} | {n} | {obs_cap} | {len(ms)} | {s['median_ms']} | {s['min_ms']} | {s['max_ms']} |")
    if md:
        with open(md, "w") as f:
            f.write("\n".join(table) + "\n")
    L.madsim_hip_shutdown()


if __name__ == "__main__":
    main()
