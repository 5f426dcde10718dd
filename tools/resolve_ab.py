#!/usr/bin/env python3
"""Cost of self-resolving campaigns (MADSIM_CAMPAIGN_RESOLVE).  One process measures the tree it is started from in ONE mode and prints one
JSON line per sample; alternate processes (and checkouts: `plain` uses nothing this tool's tree adds — tools/diff_ab.py plain of the parent
commit is the same leg there) to compare.
Usage: resolve_ab.py plain|flag|lossy|twostep|lossy-tight|twostep-tight [samples]
    plain:   the headline workload — the bench.py ping-pong case, 65 536-seed batches, 200 batches, batches in flight = auto, loss 0 — without the flag
    flag:    the same with the flag: no seed has a runner verdict, so no round runs — the same path plus one branch per harvest
    lossy:   streaming_topology on a 5 % lossy network under its own limits, 65 536-seed batches, 16 batches, with the flag: whatever the first
             pass leaves with a runner verdict is settled by the rounds
    twostep: what `lossy` replaces — the collecting campaign without the flag, listing the runner verdicts, then madsim_hip_run_batch_auto
             over every batch that holds one (48 bytes per seed to the host, no report kernels)
    lossy-tight, twostep-tight: the same pair with the workload's heap-spill quota cut from 161 entries to 56, under which the first pass
             answers about two seeds in five with an overflow (under the workload's own limits it is about one seed in a million)
ms_per_batch is the call's wall time over its batches (twostep: of both steps)."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from madsim_amd import _abi as A          # noqa: E402
from madsim_amd import runtime as R       # noqa: E402
from madsim_amd import workload as W      # noqa: E402

BATCH, BATCHES, LOSSY_BATCHES = 65536, 200, 16


def headline(mode, seed0, total, w, cfg, lim):
    rep = R.run_campaign(w, seed0, total, BATCH, 0, False, cfg, lim, resolve=True if mode == "flag" else None)
    return rep, R.campaign_resolved(), rep.wall_s, {}


def lossy(mode, seed0, total, w, cfg, lim):
    if mode.startswith("lossy"):
        rep = R.run_campaign(w, seed0, total, BATCH, 0, False, cfg, lim, resolve=True)
        return rep, R.campaign_resolved(), rep.wall_s, {}
    t0 = time.perf_counter()
    rep, fails, hist = R.run_campaign(w, seed0, total, BATCH, 0, False, cfg, lim, collect=total, list_runner=True)
    runner = fails["seed"][fails["verdict"] >= A.OVERFLOW]
    batches = sorted({int(s - seed0) // BATCH for s in runner})
    left = 0
    for k in batches:                                                                   # the second step: whole batches, as the header advised
        out, _ = R.run_batch_auto(w, seed0 + k * BATCH, min(BATCH, total - k * BATCH), cfg, lim)
        left += int((out["verdict"] >= A.OVERFLOW).sum())
    return rep, R.campaign_resolved(), time.perf_counter() - t0, {"batches_rerun": len(batches), "first_pass_runner": int(rep.n_runner), "left": left}


def main():
    mode, samples = sys.argv[1], int(sys.argv[2]) if len(sys.argv) > 2 else 1
    R.init(0)
    if mode in ("plain", "flag"):
        (w, lim, _), cfg, run, batches = W.bench_case("pingpong"), A.Config.default(), headline, BATCHES
    else:
        w, cfg, lim, run, batches = W.streaming_topology(), A.Config.default(packet_loss_rate=0.05), W.streaming_topology_limits(), lossy, LOSSY_BATCHES
        if mode.endswith("-tight"):
            lim.heap_spill_slots = 56
    run(mode, 1 << 40, 6 * BATCH, w, cfg, lim)                                          # warm-up: streams, buffers, tables, re-run scratch
    for i in range(samples):
        rep, acct, wall, extra = run(mode, (1 << 41) + i * BATCH * batches, BATCH * batches, w, cfg, lim)
        line = {"mode": mode, "seeds": int(rep.seeds_run), "wall_s": round(wall, 6), "mseeds_per_s": round(rep.seeds_run / wall / 1e6, 3),
                "ms_per_batch": round(wall * 1e3 / max(int(rep.batches_run), 1), 4), "n_failed": int(rep.n_failed), "n_runner": int(rep.n_runner),
                "batches": int(rep.batches_run), "batches_resolved": int(acct.batches_resolved), "n_first_pass": int(acct.n_first_pass),
                "n_by_round": [int(x) for x in acct.n_by_round][:4], "n_unresolved": int(acct.n_unresolved),
                "rerun_kernel_ms": round(acct.rerun_kernel_ms, 3), "kernel_ms": round(rep.kernel_ms, 3)}
        line.update(extra)
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
