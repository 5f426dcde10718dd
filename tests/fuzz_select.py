"""Random programs with the selects of ABI v7 (MS_OP_RECV_OR_TICK, MS_OP_RECV_TIMEOUT_AT): test infrastructure, compared against
tests/select_sim.py.  Built on tests/fuzz_interval.py: its servers, periods and loop bodies.

Ticker tasks on their own nodes create a ticker of every behaviour and loop over `select! { biased; recv_from(T), tick }` in either
arm order (folding the tick's instant or not), with a body that sometimes overruns the period — so ticks are due at the select's first
poll, and recv-first selects lose the messages they took — and sometimes a `timeout_at` receive from the program's mark.  Peer tasks
send datagrams of tag T to them at random intervals.  The supervisor pauses and resumes a ticking node, clogs links, and kills and
restarts a node.
"""
import random

from madsim_amd import _abi as A
from madsim_amd import workload as W
from tests import fuzz_interval as FI

T = 9


def random_select_workload(rng: random.Random, general_addr=False, hazards=False):
    """-> (workload, config, description).  `general_addr`: the echo and RPC servers bind 0.0.0.0:port and their callers name
    them by the node's IP (fuzz_interval.general_servers): the workload then needs the builds with general address resolution.  `hazards`:
    fuzz_scope.hazard at the end of every selecting task.  Both off, the programs are the ones this generator always made."""
    wl = W.WorkloadBuilder()
    ns = wl.create_node()
    a_dg, a_rpc = wl.addr(ns, 100), wl.addr(ns, 300)
    FI._servers(wl, ns, *(FI.general_servers(wl, ns, (100, 300)) if general_addr else (a_dg, a_rpc)), rng.choice([1, 3, 12]))
    tickers = []
    for i in range(rng.randint(1, 3)):
        nc = wl.create_node()
        acl = wl.addr(nc, 1 + i)
        c = wl.task(nc)
        c.bind(acl)
        c.mark()
        p = FI._period(rng)
        period_us = p.get("secs", 0) * 1_000_000 + p["us"]
        c.interval(behavior=rng.choice(["burst", "delay", "skip"]), **p)
        c.set(0, rng.randint(3, 8))
        top = c.label()
        c.recv_or_tick(acl, T, tick_first=rng.random() < 0.5, trace=rng.random() < 0.6)
        c.trace_val()
        if rng.random() < 0.3:
            c.recv_from_timeout_at(acl, T, us=rng.choice([500, 3000, 20000, 2 * period_us]))
            c.trace_val()
            if rng.random() < 0.5:
                c.mark()
        FI._body(rng, c, acl, a_dg, a_rpc, period_us)
        if rng.random() < 0.15:
            c.interval_reset()
        if rng.random() < 0.1:
            c.tick(trace=True)
        c.djnz(0, top)
        if hazards:
            FI.hazard(rng, c, acl)
        c.done()
        tickers.append((nc, acl, c))
    peers = []
    for i in range(rng.randint(1, 2)):
        npr = wl.create_node()
        ap = wl.addr(npr, 50 + i)
        s = wl.task(npr)
        s.bind(ap)
        s.set(0, rng.randint(3, 12))
        top = s.label()
        s.sleep_rand(lo_ms=0, us=rng.choice([500, 3000, 12000]))
        s.send_to(ap, rng.choice(tickers)[1], T, 0x60 + i)
        s.djnz(0, top)
        s.done()
        peers.append((npr, s))
    m = wl.main()
    for _, _, c in tickers:
        m.spawn(c)
    for _, s in peers:
        m.spawn(s)
    victim = rng.choice(tickers)[0]
    if rng.random() < 0.5:
        m.sleep(us=rng.randint(1, 20000)); m.pause(victim); m.sleep(us=rng.randint(1000, 60000)); m.resume(victim)
    if rng.random() < 0.3:
        m.sleep(us=rng.randint(1, 8000)); m.clog_link(peers[0][0], victim); m.sleep(ms=rng.randint(1, 30)); m.unclog_link(peers[0][0], victim)
    if rng.random() < 0.2:
        m.sleep(us=rng.randint(1, 8000)); m.kill(ns); m.sleep(ms=rng.randint(1, 10)); m.restart(ns)
    if rng.random() < 0.2:
        m.sleep(us=rng.randint(1, 30000)); m.kill(victim)
        if rng.random() < 0.5:
            m.sleep(ms=rng.randint(1, 10)); m.restart(victim)
    else:
        for _, _, c in tickers:
            m.join(c)
    for _, s in peers:
        m.join(s)
    m.done()
    w = wl.build()
    cfg = A.Config.default(packet_loss_rate=rng.choice([0.0, 0.0, 0.1]))
    return w, cfg, f"{len(tickers)}t/{len(peers)}p/{w.struct.n_insns}i" + ("/any" if general_addr else "")


def select_limits(state_mem=0):
    lim = FI.interval_limits(state_mem)
    lim.mbox_regs, lim.mbox_msgs = 16, 16
    return lim
