"""Random programs with timeout scopes (MS_OP_TIMEOUT_BEGIN / END): test infrastructure, compared against tests/scope_sim.py.

One server node runs three services as init tasks (re-bound after a restart): a datagram echo (recv -> sleep_rand -> reply),
a connection server (accept1 -> a handler per connection: crecv -> sleep_rand -> csend) and a typed-RPC server (a handler per
request).  Client tasks loop over scoped calls of every kind — send + recv, connect1 + csend + crecv with the `?` early return,
an untimed rpc_call, plain sleeps / sleep_rand / yield — with deadlines under, at and over the 1 ms floor, and trace what each
scope left in val.  The supervisor clogs links (the channel receiver's backoff), kills and restarts the server mid-call;
buggify (rand_delay up to 4 s) lets scopes expire inside a send's or a connect1's rand_delay.
"""
import random

from madsim_amd import _abi as A
from madsim_amd import workload as W

REQ, RSP, TAG_REQ, TAG_RSP = 0x11, 0x22, 1, 2
DEADLINES_US = [1, 500, 1000, 1001, 1500, 2000, 5000, 8000, 20000, 60000]


def _servers(wl, ns, a_dg, a_ch, a_rpc, svc_ms):
    dg = wl.task(ns, init=True, pre=True)
    dg.bind(a_dg)
    top = dg.label()
    dg.recv_from(a_dg, TAG_REQ); dg.sleep_rand(lo_ms=0, ms=svc_ms); dg.reply(a_dg, TAG_RSP, RSP); dg.jmp(top)
    h = wl.task(ns)
    h.chan_recv()
    fin = h.label() + 3
    h.jeq(A.VAL_RESET, fin); h.sleep_rand(lo_ms=0, ms=svc_ms); h.chan_send(RSP)
    assert h.label() == fin
    h.done()
    ch = wl.task(ns, init=True, pre=True)
    ch.bind(a_ch)
    top = ch.label()
    ch.accept1(a_ch); ch.spawn(h, move_conn=True); ch.jmp(top)
    rh = wl.task(ns)
    rh.sleep_rand(lo_ms=0, ms=svc_ms); rh.rpc_reply(a_rpc, RSP); rh.done()
    rs = wl.task(ns, init=True, pre=True)
    rs.bind(a_rpc)
    top = rs.label()
    rs.rpc_recv(a_rpc, 1); rs.spawn(rh, move_request=True); rs.jmp(top)


def _scope(rng, c, acl, a_dg, a_ch, a_rpc):
    us = rng.choice(DEADLINES_US)
    kind = rng.choice(["dgram", "conn", "conn", "rpc", "sleep", "mixed"])
    with c.timeout(us=us) as s:
        if kind == "dgram":
            c.send_to(acl, a_dg, TAG_REQ, REQ); c.recv_from(acl, TAG_RSP)
        elif kind == "conn":
            c.connect1(acl, a_ch); c.jeq(A.VAL_REFUSED, s.end); c.chan_send(REQ); c.chan_recv()
            if rng.random() < 0.3:
                c.jeq(A.VAL_RESET, s.end); c.trace_val(); c.chan_send(REQ + 1)
        elif kind == "rpc":
            c.rpc_call(acl, a_rpc, 1, REQ)
        elif kind == "sleep":
            c.sleep(us=rng.choice([500, 1000, 1500, 3000]))
        else:
            c.set(1, rng.randint(1, 3))
            top = c.label()
            c.sleep_rand(lo_ms=0, ms=rng.choice([1, 2, 4])); c.yield_now(); c.trace(7, add_reg=1); c.flag_add(1, 1); c.djnz(1, top)
    c.trace_val()
    if rng.random() < 0.5:                              # branch on the verdict like code after recv_from_timeout does
        j = c.label() + 2
        c.jeq(A.VAL_TIMEOUT, j); c.flag_add(0, 1)
        assert c.label() == j


HAZARD_TAG = 0x3D


def hazard(rng, c, ep):
    """What a client sometimes does last (the generators' `hazards` option): panic unless its last call timed out, or wait for a
    datagram nobody sends — the run is a DEADLOCK once every timer has fired.  The blocks of tests/tier_blocks.py need both verdicts."""
    r = rng.random()
    if r < 0.08:
        skip = c.label() + 2
        c.jeq(A.VAL_TIMEOUT, skip); c.panic(5)
        assert c.label() == skip
    elif r < 0.16:
        c.recv_from(ep, HAZARD_TAG)


def random_scope_workload(rng: random.Random, general_addr=False, hazards=False):
    """-> (workload, config, description).  `general_addr`: the server's Endpoints bind 0.0.0.0:port and the clients name them by the
    node's IP (Network::try_send's `.or_else(0.0.0.0:port)` lookup, network.rs:296-313), as tests/fuzz.py random_addr_workload does: the
    workload then needs the builds with general address resolution.  `hazards`: see hazard().  Both off, the programs are the ones
    this generator always made."""
    wl = W.WorkloadBuilder()
    ns = wl.create_node()
    a_dg, a_ch, a_rpc = wl.addr(ns, 100), wl.addr(ns, 200), wl.addr(ns, 300)
    if general_addr:                                    # (no draw: the programs of one Random differ in their addresses only)
        _servers(wl, ns, *(wl.addr(ns, p, ip="unspecified") for p in (100, 200, 300)), rng.choice([1, 2, 5, 20]))
    else:
        _servers(wl, ns, a_dg, a_ch, a_rpc, rng.choice([1, 2, 5, 20]))
    clients = []
    for i in range(rng.randint(1, 3)):
        nc = wl.create_node()
        acl = wl.addr(nc, 1 + i)
        c = wl.task(nc)
        c.bind(acl); c.sleep(us=rng.randint(0, 3000) + 1)
        loop = rng.random() < 0.6
        if loop:
            c.set(0, rng.randint(2, 4))
        top = c.label()
        for _ in range(rng.randint(1, 3)):
            _scope(rng, c, acl, a_dg, a_ch, a_rpc)
        if loop:
            c.djnz(0, top)
        if hazards:
            hazard(rng, c, acl)
        c.done()
        clients.append((nc, c))
    m = wl.main()
    for _, c in clients:
        m.spawn(c)
    if rng.random() < 0.5:
        nc = rng.choice(clients)[0]
        m.sleep(us=rng.randint(1, 5000)); m.clog_link(ns, nc); m.sleep(ms=rng.randint(1, 40)); m.unclog_link(ns, nc)
    if rng.random() < 0.5:
        m.sleep(us=rng.randint(1, 8000)); m.kill(ns)
        if rng.random() < 0.8:
            m.sleep(ms=rng.randint(1, 10)); m.restart(ns)
    for _, c in clients:
        m.join(c)
    m.done()
    w = wl.build()
    cfg = A.Config.default(packet_loss_rate=rng.choice([0.0, 0.0, 0.1]))
    if rng.random() < 0.2:
        cfg.buggify = 1
    return w, cfg, f"{len(clients)}c/{w.struct.n_insns}i" + ("/any" if general_addr else "") + ("/buggify" if cfg.buggify else "")


def scope_limits():
    lim = A.Limits()
    lim.max_tasks = 40
    lim.mbox_regs, lim.mbox_msgs = 8, 8
    lim.heap_lds_slots, lim.heap_spill_slots = 16, 240
    return lim
