#!/usr/bin/env python3
"""Cost of the grouping campaign (madsim_hip_run_campaign_groups) next to the plain one on the headline workload — the bench.py
ping-pong case, 65 536-seed batches, 200 batches per campaign, batches in flight = auto, loss 0 (every seed passes).  One process
measures the tree it is started from in ONE mode and prints one JSON line per sample; alternate processes (and checkouts: `plain` needs
nothing this tool's tree adds — tools/stats_ab.py of the parent commit is the same leg there) to compare.
Usage: groups_ab.py plain|floor|obs|trace [samples]
    floor: include = failures — nothing is counted, what the feature costs a healthy campaign
    obs:   include = PASS, key obs_hash — every seed lands in one group, the contention path
    trace: include = PASS, key trace_hash, max_groups 1024 — nearly every seed its own group, most of them end in n_ungrouped"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from madsim_amd import _abi as A          # noqa: E402
from madsim_amd import runtime as R       # noqa: E402
from madsim_amd import workload as W      # noqa: E402

BATCH, BATCHES, CAP = 65536, 200, 1024
MODES = {"floor": dict(include=(A.PANIC, A.DEADLOCK, A.TIME_LIMIT), key="obs"), "obs": dict(include=(A.PASS,), key="obs"),
         "trace": dict(include=(A.PASS,), key="trace")}


def run(mode, w, seed0, total, cfg, lim):
    if mode == "plain":
        return R.run_campaign(w, seed0, total, BATCH, 0, False, cfg, lim), None
    return R.run_campaign_groups(w, seed0, total, BATCH, 0, False, cfg, lim, max_groups=CAP, **MODES[mode])


def main():
    mode, samples = sys.argv[1], int(sys.argv[2]) if len(sys.argv) > 2 else 1
    w, lim, _ = W.bench_case("pingpong")
    cfg = A.Config.default()
    R.init(0)
    run(mode, w, 1 << 40, 6 * BATCH, cfg, lim)                                          # warm-up: streams, buffers, tables
    for i in range(samples):
        rep, groups = run(mode, w, (1 << 41) + i * BATCH * BATCHES, BATCH * BATCHES, cfg, lim)
        line = {"mode": mode, "seeds": int(rep.seeds_run), "wall_s": round(rep.wall_s, 6), "mseeds_per_s": round(rep.seeds_run / rep.wall_s / 1e6, 2),
                "n_failed": int(rep.n_failed), "n_runner": int(rep.n_runner)}
        if groups is not None:
            line.update(n_groups=len(groups), n_grouped=groups.n_grouped, n_ungrouped=groups.n_ungrouped,
                        largest=max((int(c) for c in groups.groups["count"]), default=0))
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
