#!/usr/bin/env python3
"""Cost of the signal builds on the GPU: the yardstick pair at full batch, and graceful_shutdown in both layouts.

    python tools/signal_ab.py [--rounds 3]

The pair is one supervised-nodes workload in two forms that execute the same events: the supervisor stops nodes with MS_OP_KILL (the
every-class build) or with MS_OP_SEND_CTRL_C on nodes that install no handler (kill_id through the signal build).  The two forms run
alternately, each measurement in a fresh child process (one process holds the GPU at a time).  G steps/s of a full batch = total steps
/ wall time of a 6-batch campaign, best of 3 after a warm-up.  One JSON line per measurement, then the summary lines."""
import argparse
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)
BATCH = 262144


def supervised(form, n_nodes=4, rounds=6):
    """`n_nodes` echo servers (init tasks) with a client each; the supervisor stops and restarts every node `rounds` times."""
    from madsim_amd import workload as W
    wl = W.WorkloadBuilder()
    m = wl.main()
    nodes, clients = [], []
    for i in range(n_nodes):
        n = wl.create_node()
        a = wl.addr(n, 1)
        s = wl.task(n, init=True, pre=True)
        s.bind(a)
        top = s.label()
        s.recv_from(a, 7); s.reply(a, 7, 0x70 + i); s.jmp(top)
        nc = wl.create_node()
        ac = wl.addr(nc, 1)
        c = wl.task(nc)
        c.bind(ac); c.set(0, 4 * rounds)
        top = c.label()
        c.send_to(ac, a, 7, i); c.recv_from_timeout(ac, 7, ms=6); c.trace_val(); c.djnz(0, top); c.done()
        nodes.append(n); clients.append(c)
    for c in clients:
        m.spawn(c)
    m.set(0, rounds)
    top = m.label()
    for n in nodes:
        m.sleep(ms=3)
        if form == "kill":
            m.kill(n)
        else:
            m.send_ctrl_c(n)
        m.sleep(ms=2); m.restart(n)
    m.djnz(0, top)
    for c in clients:
        m.join(c)
    m.done()
    return wl.build()


def supervised_limits():
    from madsim_amd import _abi as A
    lim = A.Limits()
    lim.max_tasks = 24
    lim.mbox_regs, lim.mbox_msgs = 16, 8
    lim.heap_lds_slots, lim.heap_spill_slots = 16, 48
    return lim


def cases():
    from madsim_amd import _abi as A
    from madsim_amd import workload as W
    out = {"pair_kill": (supervised("kill"), supervised_limits()), "pair_send_ctrl_c": (supervised("signal"), supervised_limits())}
    for tag, sm in (("lds", A.STATE_LDS), ("global", A.STATE_GLOBAL)):
        lim = W.graceful_shutdown_limits()
        lim.state_mem = sm
        out["graceful_shutdown_" + tag] = (W.graceful_shutdown(), lim)
    return out


def child(names):
    from madsim_amd import runtime as R
    R.init(0)
    C = cases()
    for name in names:
        w, lim = C[name]
        R.run_campaign(w, 0, BATCH, batch=BATCH, limits=lim)                  # warm-up
        best, rep = None, None
        for _ in range(3):
            rep = R.run_campaign(w, 1 << 32, BATCH * 6, batch=BATCH, limits=lim)
            r = rep.total_steps / rep.wall_s / 1e9
            best = r if best is None or r > best else best
        print(json.dumps({"case": name, "kernel": R.variant_name(R.geometry(w, lim)), "batch": BATCH, "gsteps_per_s": round(best, 3),
                          "total_steps": int(rep.total_steps), "n_failed": rep.n_failed, "n_runner": rep.n_runner}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--child", nargs="*")
    a = ap.parse_args()
    if a.child is not None:
        return child(a.child)
    best, steps = {}, {}
    order = [["pair_kill"], ["pair_send_ctrl_c"]]
    for rnd in range(a.rounds):
        for names in order + ([["graceful_shutdown_lds", "graceful_shutdown_global"]] if rnd == 0 else []):
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", *names], cwd=HERE, capture_output=True, text=True, timeout=600)
            if out.returncode != 0:                          # a failing child ends the A/B: nothing more is started on the GPU
                sys.stdout.write(out.stdout)
                sys.stderr.write(out.stderr)
                sys.exit(out.returncode)
            for ln in out.stdout.splitlines():
                if ln.startswith("{"):
                    d = json.loads(ln)
                    d["round"] = rnd
                    print(json.dumps(d), flush=True)
                    best[d["case"]] = max(best.get(d["case"], 0.0), d["gsteps_per_s"])
                    steps[d["case"]] = d["total_steps"]
    k, s = best.get("pair_kill"), best.get("pair_send_ctrl_c")
    print(json.dumps({"summary": "pair", "kill_form": k, "send_ctrl_c_form": s, "ratio": round(s / k, 4) if k and s else None,
                      "same_steps": steps.get("pair_kill") == steps.get("pair_send_ctrl_c")}), flush=True)
    for c in ("graceful_shutdown_lds", "graceful_shutdown_global"):
        print(json.dumps({"summary": c, "gsteps_per_s": best.get(c)}), flush=True)


if __name__ == "__main__":
    main()
