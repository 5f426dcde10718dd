#!/usr/bin/env python3
"""A/B of the interval-ticker builds (MS_OP_INTERVAL / TICK / INTERVAL_RESET) on the GPU: G steps/s of raft_ticker and lease_keeper at a
full batch on the ticker builds, and of the oracle-rewritable ticker class (straight-line ticker programs, tests/test_interval.py
straight_line) on the ticker build next to its MARK + SLEEP_UNTIL rewrite (tests/interval_sim.py) on the build it selects without
tickers — bit-identical results (tests/test_interval_gpu.py).  One JSON line per case."""
import json
import os
import random
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from madsim_amd import runtime as R       # noqa: E402
from madsim_amd import workload as W      # noqa: E402
from tests import fuzz_interval as F      # noqa: E402
from tests import interval_sim as I       # noqa: E402
from tests.test_interval import straight_line   # noqa: E402


def rate(w, lim, batch, cfg=None, batches=6, reps=3):
    best = None
    R.run_campaign(w, 0, batch, batch=batch, config=cfg, limits=lim)          # warm-up
    for _ in range(reps):
        rep = R.run_campaign(w, 1 << 32, batch * batches, batch=batch, config=cfg, limits=lim)
        r = rep.total_steps / rep.wall_s / 1e9
        best = r if best is None or r > best else best
    return best, rep


def main():
    R.init(0)
    cases = [("raft_ticker", W.raft_ticker(), W.raft_ticker_limits(), 262144, None),
             ("raft_ticker/skip", W.raft_ticker(behavior="skip"), W.raft_ticker_limits(), 262144, None),
             ("lease_keeper", W.lease_keeper(), W.lease_keeper_limits(), 262144, None)]
    w, cfg = straight_line(random.Random(4203))
    lim = F.interval_limits(2)
    lim.lanes_per_wave = 0
    cases.append(("straight_line/ticks", w, lim, 262144, cfg))
    cases.append(("straight_line/sleep_until", I.rewrite_ticks_as_sleep_until(w), lim, 262144, cfg))
    for name, w, lim, batch, cfg in cases:
        g = R.geometry(w, lim)
        r, rep = rate(w, lim, batch, cfg)
        print(json.dumps({"case": name, "kernel": R.variant_name(g), "batch": batch, "gsteps_per_s": round(r, 3),
                          "n_failed": rep.n_failed, "n_runner": rep.n_runner}), flush=True)


if __name__ == "__main__":
    main()
