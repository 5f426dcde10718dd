#!/usr/bin/env python3
"""What a seed list costs a campaign.  The library is the one MADSIM_HIP_LIB names (default: this tree's), loaded with ctypes alone so that
the parent commit's build — which has no list entry points — can be measured too: that leg then prints the range campaign only.

    range      madsim_hip_run_campaign over BATCHES x 65 536 seeds of the headline ping-pong (4 nodes, 64 rounds), 65 536 per batch
    list       madsim_hip_run_seeds_campaign over the same seeds, given as a list (8 bytes per seed ride each flight's stream)
    corpus     the fix check the list forms exist for, on the lossy two-pair ping-pong of examples/fix_check_test.cpp (loss 0.002): the
               failing seeds of the range as a list, diffed against the body with a timeout and a resend — beside
    range-diff the diff of the whole range a user had to run instead

One JSON line per sample: wall_ms is the call's wall time on the host, kernel_ms the sum of its simulation kernels' HIP-event durations.

    python tools/seedlist_ab.py [samples] [batches]
    MADSIM_HIP_LIB=<parent>/madsim_amd/libmadsim_hip.so python tools/seedlist_ab.py [samples] [batches]
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

BATCH, SEED0, LOSS = 65536, 1, 0.002


def two_pairs(fixed, rounds=16):
    """The two bodies of examples/fix_check_test.cpp."""
    wl = W.WorkloadBuilder()
    tasks = []
    for _ in range(2):
        n1, n2 = wl.create_node(), wl.create_node()
        a1, a2 = wl.addr(n1, 1), wl.addr(n2, 1)
        t1, t2 = wl.task(n1), wl.task(n2)
        t1.bind(a1).sleep(secs=1).set(0, rounds)
        t2.bind(a2)
        top1 = t1.label()
        if not fixed:
            t1.send_to(a1, a2, 1, W.PING).recv_from(a1, 1).assert_val(W.PONG).djnz(0, top1).done()
            t2.set(0, rounds)
            top2 = t2.label()
            t2.recv_from(a2, 1).assert_val(W.PING).reply(a2, 1, W.PONG).djnz(0, top2).done()
        else:
            t1.send_to(a1, a2, 1, W.PING).recv_from_timeout(a1, 1, ms=100).jeq(A.VAL_TIMEOUT, top1).assert_val(W.PONG).djnz(0, top1).done()
            top2 = t2.label()
            t2.recv_from_timeout(a2, 1, secs=5).jeq(A.VAL_TIMEOUT, top2 + 5).assert_val(W.PING).reply(a2, 1, W.PONG).jmp(top2).done()
        tasks += [t1, t2]
    m = wl.main()
    for t in tasks:
        m.spawn(t)
    for t in tasks:
        m.join(t)
    m.done()
    return wl.build()


def main():
    samples = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    batches = int(sys.argv[2]) if len(sys.argv) > 2 else 100
    total = batches * BATCH
    path = os.environ.get("MADSIM_HIP_LIB", os.path.join(ROOT, "madsim_amd", "libmadsim_hip.so"))
    L = C.CDLL(path)
    u64p = C.POINTER(C.c_uint64)
    plain = [C.POINTER(A.Workload), C.POINTER(A.Config), C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint32, C.POINTER(A.Limits), C.POINTER(A.Campaign)]
    side = [C.POINTER(A.Workload), C.POINTER(A.Config), C.POINTER(A.Limits)]
    tail = [C.c_uint64, C.c_uint32, C.c_uint32, C.POINTER(A.Campaign), C.POINTER(A.Campaign), C.POINTER(A.Diff)]
    L.madsim_hip_run_campaign.argtypes = plain
    L.madsim_hip_run_campaign_collect.argtypes = plain + [C.POINTER(A.Collect)]
    L.madsim_hip_run_campaign_diff.argtypes = side + side + [C.c_uint64, C.c_uint64] + tail
    has_list = hasattr(L, "madsim_hip_run_seeds_campaign")
    if has_list:
        L.madsim_hip_run_seeds_campaign.argtypes = plain[:2] + [u64p, C.c_uint64] + plain[4:] + [C.c_void_p] * 3
        L.madsim_hip_run_seeds_campaign_diff.argtypes = side + side + [u64p, C.c_uint64] + tail
    assert L.madsim_hip_init(0) == 0
    w, cfg, lim = W.pingpong(4, 64), A.Config.default(), A.Limits()
    seeds = np.arange(SEED0, SEED0 + total, dtype=np.uint64)
    # the corpus legs: the capacities examples/fix_check_test.cpp gives the fixed body
    w_a, w_b, cfg_l, lim_l = two_pairs(False), two_pairs(True), A.Config.default(packet_loss_rate=LOSS), A.Limits()
    lim_l.heap_spill_slots, lim_l.mbox_regs, lim_l.mbox_msgs = 128, 8, 4
    rec = np.zeros(total, dtype=A.FAILURE_DTYPE)
    col = A.Collect()
    col.failures, col.cap = rec.ctypes.data_as(C.POINTER(A.Failure)), total
    rep0 = A.Campaign()
    assert L.madsim_hip_run_campaign_collect(w_a.ref(), C.byref(cfg_l), SEED0, total, BATCH, 0, 0, C.byref(lim_l), C.byref(rep0), C.byref(col)) == 0
    corpus = np.ascontiguousarray(rec["seed"][:col.n_listed])

    def diff_struct():
        d = A.Diff()
        d.fields = A.DIFF_VERDICT
        return d

    def run_range():
        rep = A.Campaign()
        assert L.madsim_hip_run_campaign(w.ref(), C.byref(cfg), SEED0, total, BATCH, 0, 0, C.byref(lim), C.byref(rep)) == 0
        return rep, {"seeds": int(rep.seeds_run), "failed": int(rep.n_failed)}

    def run_list():
        rep = A.Campaign()
        assert L.madsim_hip_run_seeds_campaign(w.ref(), C.byref(cfg), seeds.ctypes.data_as(u64p), total, BATCH, 0, 0, C.byref(lim), C.byref(rep), None, None, None) == 0
        return rep, {"seeds": int(rep.seeds_run), "failed": int(rep.n_failed)}

    def run_range_diff():
        ra, rb, d = A.Campaign(), A.Campaign(), diff_struct()
        assert L.madsim_hip_run_campaign_diff(w_a.ref(), C.byref(cfg_l), C.byref(lim_l), w_b.ref(), C.byref(cfg_l), C.byref(lim_l), SEED0, total, BATCH, 0, 0,
                                              C.byref(ra), C.byref(rb), C.byref(d)) == 0
        ra.kernel_ms += rb.kernel_ms
        return ra, {"seeds": int(ra.seeds_run), "fixed": int(sum(d.transitions[v][0] for v in range(1, 8))), "broken": int(sum(d.transitions[0][1:]))}

    def run_corpus():
        ra, rb, d = A.Campaign(), A.Campaign(), diff_struct()
        assert L.madsim_hip_run_seeds_campaign_diff(w_a.ref(), C.byref(cfg_l), C.byref(lim_l), w_b.ref(), C.byref(cfg_l), C.byref(lim_l),
                                                    corpus.ctypes.data_as(u64p), len(corpus), BATCH, 0, 0, C.byref(ra), C.byref(rb), C.byref(d)) == 0
        ra.kernel_ms += rb.kernel_ms
        return ra, {"seeds": int(ra.seeds_run), "fixed": int(sum(d.transitions[v][0] for v in range(1, 8))), "broken": int(sum(d.transitions[0][1:]))}

    legs = [("range", run_range)] + ([("list", run_list)] if has_list else []) + [("range-diff", run_range_diff)] + ([("corpus", run_corpus)] if has_list else [])
    for _, f in legs:
        f()                                                  # warm-up: tables uploaded, buffers allocated, kernels loaded
    for i in range(samples):
        for name, f in legs:
            t0 = time.perf_counter()
            rep, extra = f()
            line = {"lib": os.path.relpath(path, ROOT) if path.startswith(ROOT) else "parent", "leg": name, "sample": i,
                    "wall_ms": round((time.perf_counter() - t0) * 1e3, 3), "kernel_ms": round(rep.kernel_ms, 3), "batches": int(rep.batches_run)}
            line.update(extra)
            print(json.dumps(line), flush=True)
    L.madsim_hip_shutdown()


if __name__ == "__main__":
    main()
