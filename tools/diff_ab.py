#!/usr/bin/env python3
"""Cost of the differential campaign (madsim_hip_run_campaign_diff) next to the plain one on the headline workload — the bench.py
ping-pong case, 65 536-seed batches, 200 batches per campaign, batches in flight = auto, loss 0 (every seed passes).  One process
measures the tree it is started from in ONE mode and prints one JSON line per sample; alternate processes (and checkouts: `plain` needs
nothing this tool's tree adds — tools/groups_ab.py plain of the parent commit is the same leg there) to compare.
Usage: diff_ab.py plain|diff|verdict [samples]
    diff:    A = B = the workload, fields = ALL — all 96 bytes per seed are read, nothing differs: the build-against-build check
    verdict: A = B = the workload, fields = VERDICT — 32 bytes per seed are read
ms_per_batch is the call's wall time over its batches; a diff batch is two simulations, so the yardstick is twice the plain figure."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from madsim_amd import _abi as A          # noqa: E402
from madsim_amd import runtime as R       # noqa: E402
from madsim_amd import workload as W      # noqa: E402

BATCH, BATCHES = 65536, 200
FIELDS = {"diff": A.DIFF_ALL, "verdict": A.DIFF_VERDICT}


def run(mode, w, seed0, total, cfg, lim):
    if mode == "plain":
        return R.run_campaign(w, seed0, total, BATCH, 0, False, cfg, lim), None
    rep, _, d = R.run_campaign_diff(w, seed0, total, config=cfg, limits=lim, fields=FIELDS[mode], max_listed=64, batch=BATCH)
    return rep, d


def main():
    mode, samples = sys.argv[1], int(sys.argv[2]) if len(sys.argv) > 2 else 1
    w, lim, _ = W.bench_case("pingpong")
    cfg = A.Config.default()
    R.init(0)
    run(mode, w, 1 << 40, 6 * BATCH, cfg, lim)                                          # warm-up: streams, buffers, tables
    for i in range(samples):
        rep, d = run(mode, w, (1 << 41) + i * BATCH * BATCHES, BATCH * BATCHES, cfg, lim)
        line = {"mode": mode, "seeds": int(rep.seeds_run), "wall_s": round(rep.wall_s, 6), "mseeds_per_s": round(rep.seeds_run / rep.wall_s / 1e6, 2),
                "ms_per_batch": round(rep.wall_s * 1e3 / max(int(rep.batches_run), 1), 4), "n_failed": int(rep.n_failed), "n_runner": int(rep.n_runner)}
        if d is not None:
            line.update(n_differ=d.n_differ, n_compared=d.n_compared, pass_pass=int(d.transitions[0, 0]))
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
