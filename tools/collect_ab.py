#!/usr/bin/env python3
"""Cost of the collecting campaign (madsim_hip_run_campaign_collect) next to the plain one on the headline workload — the bench.py
ping-pong case, 65 536-seed batches, 200 batches per campaign.  One process measures the tree it is started from in ONE mode and prints
one JSON line per sample; alternate processes (and checkouts: `plain` needs nothing this tool's tree adds) to compare.
Usage: collect_ab.py plain|collect0|collect11 [samples]        (collect0: loss 0, nothing fails; collect11: loss 0.002, about 11 % fail)"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from madsim_amd import _abi as A          # noqa: E402
from madsim_amd import runtime as R       # noqa: E402
from madsim_amd import workload as W      # noqa: E402

BATCH, BATCHES, CAP = 65536, 200, 1024


def main():
    mode, samples = sys.argv[1], int(sys.argv[2]) if len(sys.argv) > 2 else 1
    w, lim, _ = W.bench_case("pingpong")
    cfg = A.Config.default(packet_loss_rate=0.002 if mode == "collect11" else 0.0)
    kw = {} if mode == "plain" else {"collect": CAP}
    R.init(0)
    R.run_campaign(w, 1 << 40, 6 * BATCH, BATCH, 0, False, cfg, lim, **kw)              # warm-up: streams, buffers, tables
    for i in range(samples):
        got = R.run_campaign(w, (1 << 41) + i * BATCH * BATCHES, BATCH * BATCHES, BATCH, 0, False, cfg, lim, **kw)
        rep = got if mode == "plain" else got[0]
        line = {"mode": mode, "seeds": int(rep.seeds_run), "wall_s": round(rep.wall_s, 6), "mseeds_per_s": round(rep.seeds_run / rep.wall_s / 1e6, 2),
                "n_failed": int(rep.n_failed), "n_runner": int(rep.n_runner)}
        if mode != "plain":
            line["n_listed"] = len(got[1])
            line["by_verdict"] = [int(x) for x in got[2]]
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
