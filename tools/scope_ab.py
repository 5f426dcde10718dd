#!/usr/bin/env python3
"""A/B of the timeout-scope builds (MS_OP_TIMEOUT_BEGIN / END) on the GPU: G steps/s of tonic_unary at a full batch, and of the
election loop and the streaming topology rewritten into scopes (tests/scope_sim.py rewrite_into_scopes) next to the originals on the
nearest build without scopes (global state, wide heap entries: the narrow / re-registration-count flags off), same in_flight.
One JSON line per case."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from madsim_amd import _abi as A          # noqa: E402
from madsim_amd import runtime as R       # noqa: E402
from madsim_amd import workload as W      # noqa: E402
from tests import scope_sim as S          # noqa: E402


def wide(lim):
    g = A.Limits()
    for f, _ in A.Limits._fields_:
        setattr(g, f, getattr(lim, f))
    g.state_mem &= 0xff
    return g


def rate(w, lim, batch, batches=6, reps=3):
    best = None
    R.run_campaign(w, 0, batch, batch=batch, limits=lim)              # warm-up
    for _ in range(reps):
        rep = R.run_campaign(w, 1 << 32, batch * batches, batch=batch, limits=lim)
        r = rep.total_steps / rep.wall_s / 1e9
        best = r if best is None or r > best else best
    return best, rep


def main():
    R.init(0)
    cases = [("tonic_unary", W.tonic_unary(), W.tonic_unary_limits(), 262144)]
    for name, w, lim, batch in (("raft_election", W.raft_election(), W.raft_election_limits(), 262144),
                                ("streaming_topology", W.streaming_topology(), W.streaming_topology_limits(), 65536)):
        cases.append((name + "/original-wide", w, wide(lim), batch))
        cases.append((name + "/scopes", S.rewrite_into_scopes(w), wide(lim), batch))
        cases.append((name + "/original-own-limits", w, lim, batch))
    for name, w, lim, batch in cases:
        g = R.geometry(w, lim)
        r, rep = rate(w, lim, batch)
        print(json.dumps({"case": name, "kernel": R.variant_name(g), "batch": batch, "gsteps_per_s": round(r, 3),
                          "n_failed": rep.n_failed, "n_runner": rep.n_runner}), flush=True)


if __name__ == "__main__":
    main()
