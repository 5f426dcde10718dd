"""Random programs with interval tickers (MS_OP_INTERVAL / TICK / INTERVAL_RESET): test infrastructure, compared against
tests/interval_sim.py.

One server node runs a datagram echo and a typed-RPC server as init tasks (re-bound after a restart).  Ticker tasks on their own
nodes create `interval` / `interval_at` tickers of every behaviour, with periods below and above the 1 ms floor and periods whose
whole seconds use the `b` operand, then loop: tick (sometimes folding the instant, sometimes inside a timeout scope), and a body
that sometimes overruns the period — sleep_rand, a datagram round trip, an RPC, a channel op, yields — with an occasional reset.
The supervisor pauses and resumes a ticking node, kills and restarts one, and clogs links.
"""
import random

from madsim_amd import _abi as A
from madsim_amd import workload as W
from tests.fuzz_scope import hazard

REQ, RSP, TAG_REQ, TAG_RSP = 0x11, 0x22, 1, 2
PERIODS_US = [300, 999, 1000, 1500, 4000, 10000, 25000, 50000]


def _servers(wl, ns, a_dg, a_rpc, svc_ms):
    dg = wl.task(ns, init=True, pre=True)
    dg.bind(a_dg)
    top = dg.label()
    dg.recv_from(a_dg, TAG_REQ); dg.sleep_rand(lo_ms=0, ms=svc_ms); dg.reply(a_dg, TAG_RSP, RSP); dg.jmp(top)
    rh = wl.task(ns)
    rh.sleep_rand(lo_ms=0, ms=svc_ms); rh.rpc_reply(a_rpc, RSP); rh.done()
    rs = wl.task(ns, init=True, pre=True)
    rs.bind(a_rpc)
    top = rs.label()
    rs.rpc_recv(a_rpc, 1); rs.spawn(rh, move_request=True); rs.jmp(top)


def _period(rng):
    if rng.random() < 0.1:
        return dict(secs=1, us=rng.choice([0, 250000]))       # whole seconds in b
    return dict(us=rng.choice(PERIODS_US))


def _body(rng, c, acl, a_dg, a_rpc, period_us):
    kind = rng.choice(["sleep", "sleep", "dgram", "rpc", "yield", "none"])
    if kind == "sleep":
        c.sleep_rand(lo_ms=0, us=max(2, rng.choice([period_us // 2, period_us, 2 * period_us, 7 * period_us])))
    elif kind == "dgram":
        c.send_to(acl, a_dg, TAG_REQ, REQ); c.recv_from_timeout(acl, TAG_RSP, ms=rng.choice([5, 30]))
    elif kind == "rpc":
        c.rpc_call(acl, a_rpc, 1, REQ, timeout_ms=rng.choice([4, 40]))
    elif kind == "yield":
        c.yield_now(); c.trace(3)
    c.trace_val()


def general_servers(wl, ns, ports):
    """The server's Endpoints bound on 0.0.0.0:port while the clients name them by the node's IP (Network::try_send's
    `.or_else(0.0.0.0:port)` lookup, network.rs:296-313), as tests/fuzz.py random_addr_workload does: entries to bind."""
    return [wl.addr(ns, p, ip="unspecified") for p in ports]


def random_interval_workload(rng: random.Random, general_addr=False, hazards=False):
    """-> (workload, config, description).  `general_addr`: see general_servers — the workload then needs the builds with general
    address resolution.  `hazards`: fuzz_scope.hazard at the end of every ticker task.  Both off, the programs are the ones this
    generator always made."""
    wl = W.WorkloadBuilder()
    ns = wl.create_node()
    a_dg, a_rpc = wl.addr(ns, 100), wl.addr(ns, 300)
    _servers(wl, ns, *(general_servers(wl, ns, (100, 300)) if general_addr else (a_dg, a_rpc)), rng.choice([1, 3, 12]))
    tickers = []
    for i in range(rng.randint(1, 3)):
        nc = wl.create_node()
        acl = wl.addr(nc, 1 + i)
        c = wl.task(nc)
        c.bind(acl)
        at = rng.random() < 0.3
        if at:
            c.mark(); c.sleep(us=rng.randint(1, 3000))
        p = _period(rng)
        period_us = p.get("secs", 0) * 1_000_000 + p["us"]
        c.interval(behavior=rng.choice(["burst", "delay", "skip"]), at_mark=at, **p)
        c.set(0, rng.randint(3, 8))
        top = c.label()
        if rng.random() < 0.25:
            with c.timeout(us=rng.choice([500, 2000, period_us])):
                c.tick(trace=rng.random() < 0.5)
            c.trace_val()
        else:
            c.tick(trace=rng.random() < 0.7)
        c.trace_instant()
        _body(rng, c, acl, a_dg, a_rpc, period_us)
        if rng.random() < 0.2:
            c.interval_reset()
        if rng.random() < 0.1:
            c.interval(behavior=rng.choice(["burst", "delay", "skip"]), us=rng.choice(PERIODS_US))   # replaced ticker
        c.djnz(0, top)
        if hazards:
            hazard(rng, c, acl)
        c.done()
        tickers.append((nc, c))
    m = wl.main()
    for _, c in tickers:
        m.spawn(c)
    victim = rng.choice(tickers)[0]
    if rng.random() < 0.5:
        m.sleep(us=rng.randint(1, 20000)); m.pause(victim); m.sleep(us=rng.randint(1000, 120000)); m.resume(victim)
    if rng.random() < 0.3:
        m.sleep(us=rng.randint(1, 8000)); m.clog_link(ns, victim); m.sleep(ms=rng.randint(1, 40)); m.unclog_link(ns, victim)
    if rng.random() < 0.3:
        m.sleep(us=rng.randint(1, 8000)); m.kill(ns); m.sleep(ms=rng.randint(1, 10)); m.restart(ns)
    if rng.random() < 0.2:
        m.sleep(us=rng.randint(1, 30000)); m.kill(victim)
        if rng.random() < 0.5:
            m.sleep(ms=rng.randint(1, 10)); m.restart(victim)
    else:
        for _, c in tickers:
            m.join(c)
    m.done()
    w = wl.build()
    cfg = A.Config.default(packet_loss_rate=rng.choice([0.0, 0.0, 0.1]))
    return w, cfg, f"{len(tickers)}t/{w.struct.n_insns}i" + ("/any" if general_addr else "")


def interval_limits(state_mem=0):
    lim = A.Limits()
    lim.max_tasks = 40
    lim.mbox_regs, lim.mbox_msgs = 8, 8
    lim.heap_lds_slots, lim.heap_spill_slots = 16, 240
    lim.state_mem = state_mem
    return lim
