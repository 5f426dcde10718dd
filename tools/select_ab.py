#!/usr/bin/env python3
"""A/B of the ticker builds after the selects of ABI v7 (MS_OP_RECV_OR_TICK / RECV_TIMEOUT_AT) on the GPU.

    python tools/select_ab.py --parent DIR [--rounds 3]

DIR is a built checkout of the parent commit (its libmadsim_hip.so in DIR/madsim_amd).  raft_ticker and lease_keeper run on the
parent's library and on this tree's, alternately, each round in a fresh child process per tree (one process holds the GPU at a time);
raft_select runs on this tree.  G steps/s of a full batch = total steps / wall time of a 6-batch campaign, best of 3 after a warm-up.
One JSON line per measurement, then one summary line per workload (best rate per tree, this tree against the parent in %)."""
import argparse
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BATCH = 262144


def child(root, cases):
    sys.path.insert(0, root)
    from madsim_amd import runtime as R
    from madsim_amd import workload as W
    R.init(0)
    for name in cases:
        w, lim = getattr(W, name)(), getattr(W, name + "_limits")()
        R.run_campaign(w, 0, BATCH, batch=BATCH, limits=lim)                  # warm-up
        best, rep = None, None
        for _ in range(3):
            rep = R.run_campaign(w, 1 << 32, BATCH * 6, batch=BATCH, limits=lim)
            r = rep.total_steps / rep.wall_s / 1e9
            best = r if best is None or r > best else best
        print(json.dumps({"case": name, "tree": root, "kernel": R.variant_name(R.geometry(w, lim)), "batch": BATCH,
                          "gsteps_per_s": round(best, 3), "n_failed": rep.n_failed, "n_runner": rep.n_runner}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--child", nargs="*")
    ap.add_argument("--root", default=HERE)
    a = ap.parse_args()
    if a.child is not None:
        return child(a.root, a.child)
    parent = os.path.abspath(a.parent)
    best = {}
    for rnd in range(a.rounds):
        for tree, cases in ((parent, ["raft_ticker", "lease_keeper"]), (HERE, ["raft_ticker", "lease_keeper", "raft_select"])):
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--root", tree, "--child", *cases], cwd=tree,
                                 capture_output=True, text=True, timeout=600)
            if out.returncode != 0:                          # a failing child ends the A/B: nothing more is started on the GPU
                sys.stdout.write(out.stdout)
                sys.stderr.write(out.stderr)
                sys.exit(out.returncode)
            for ln in out.stdout.splitlines():
                if ln.startswith("{"):
                    d = json.loads(ln)
                    d["round"] = rnd
                    print(json.dumps(d), flush=True)
                    k = (d["case"], "parent" if tree == parent else "this")
                    best[k] = max(best.get(k, 0.0), d["gsteps_per_s"])
    for case in ("raft_ticker", "lease_keeper", "raft_select"):
        p, t = best.get((case, "parent")), best.get((case, "this"))
        print(json.dumps({"summary": case, "parent": p, "this": t, "delta_pct": round(100 * (t / p - 1), 2) if p and t else None}), flush=True)


if __name__ == "__main__":
    main()
