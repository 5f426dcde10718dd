#!/usr/bin/env python3
"""Cost of the statistics campaign (madsim_hip_run_campaign_stats) next to the plain and the collecting one on the headline workload —
the bench.py ping-pong case, 65 536-seed batches, 200 batches per campaign, batches in flight = auto.  One process measures the tree it
is started from in ONE mode and prints one JSON line per sample; alternate processes (and checkouts: `plain` needs nothing this tool's
tree adds — tools/collect_ab.py of the parent commit is the same leg there) to compare.
Usage: stats_ab.py plain|collect|stats0|stats16 [samples]        (collect: cap 1024, nothing fails; statsK: include = PASS, top_k = K)"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from madsim_amd import _abi as A          # noqa: E402
from madsim_amd import runtime as R       # noqa: E402
from madsim_amd import workload as W      # noqa: E402

BATCH, BATCHES, CAP = 65536, 200, 1024


def run(mode, w, seed0, total, cfg, lim):
    if mode == "plain":
        return R.run_campaign(w, seed0, total, BATCH, 0, False, cfg, lim), None
    if mode == "collect":
        return R.run_campaign(w, seed0, total, BATCH, 0, False, cfg, lim, collect=CAP)[0], None
    return R.run_campaign_stats(w, seed0, total, BATCH, 0, False, cfg, lim, include=(A.PASS,), top_k=int(mode[5:]))


def main():
    mode, samples = sys.argv[1], int(sys.argv[2]) if len(sys.argv) > 2 else 1
    w, lim, _ = W.bench_case("pingpong")
    cfg = A.Config.default()
    R.init(0)
    run(mode, w, 1 << 40, 6 * BATCH, cfg, lim)                                          # warm-up: streams, buffers, tables
    for i in range(samples):
        rep, stats = run(mode, w, (1 << 41) + i * BATCH * BATCHES, BATCH * BATCHES, cfg, lim)
        line = {"mode": mode, "seeds": int(rep.seeds_run), "wall_s": round(rep.wall_s, 6), "mseeds_per_s": round(rep.seeds_run / rep.wall_s / 1e6, 2),
                "n_failed": int(rep.n_failed), "n_runner": int(rep.n_runner)}
        if stats is not None:
            line.update(n=stats.n, clock_p50=list(stats.quantile("clock_ns", 0.5)), clock_p99=list(stats.quantile("clock_ns", 0.99)),
                        clock_max=stats.max["clock_ns"], slowest=[int(s) for s in stats.top("clock_ns")["seed"][:3]])
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
