"""Traced workloads for the time log (include/madsim_hip.h "Timelines"), each with its STAMPED TWIN: stamp=True puts a trace_instant()
behind every traced value.  The stamp leaves a run unchanged (tests/test_spans.py proves it on the oracle, workload by workload), so the
odd entries of the oracle's observation list of the twin are the times the device must report for the plain run, and the even entries are
the plain run's values.  Shared by tests/test_spans.py, tests/test_timeline_emu.py and tests/test_spans_gpu.py.

One workload for every trace build of the build table (sim_kernel.h: MADSIM_FEAT_ALL alone and with the scope, tick, select and signal
masks); among them a ticker whose traced ticks run late — the value folded is the deadline the tick was scheduled for, the time entry is
the clock —, and one with trace_system_time, whose value is the clock plus a per-seed base.

A case is (workload, config, limits)."""
from madsim_amd import _abi as A
from madsim_amd import workload as W

PINGPONG_ROUNDS, PINGPONG_LOSS = 16, 0.004
NAMES = ("pingpong", "scope", "ticker", "select", "signal")
TIER_OF = {"pingpong": "base", "scope": "scope", "ticker": "tick", "select": "select", "signal": "signal"}


class _Stamper:
    """t.trace(..) / t.trace_val() / t.trace_system_time() / t.tick(trace=True) through this object get their stamp where asked for."""

    def __init__(self, stamp):
        self.stamp = stamp

    def __call__(self, t):
        if self.stamp:
            t.trace_instant()
        return t


def pingpong(stamp=False, rounds=PINGPONG_ROUNDS, loss=PINGPONG_LOSS):
    """The two-pair lossy ping-pong: a client traces 0x10 + pair before its loop, 0x30 + pair in every round and 0x20 + pair behind it.  A
    lost datagram leaves its pair parked for ever: the seed deadlocks and the span 0x10 -> 0x20 of that pair stays open."""
    st = _Stamper(stamp)
    wl = W.WorkloadBuilder()
    tasks = []
    for pair in range(2):
        n1, n2 = wl.create_node(), wl.create_node()
        a1, a2 = wl.addr(n1, 1), wl.addr(n2, 1)
        t1 = wl.task(n1)
        st(t1.bind(a1).sleep(secs=1).trace(0x10 + pair)).set(0, rounds)
        top1 = t1.label()
        st(t1.send_to(a1, a2, 1, W.PING).recv_from(a1, 1).assert_val(W.PONG).trace(0x30 + pair)).djnz(0, top1)
        st(t1.trace(0x20 + pair)).done()
        t2 = wl.task(n2)
        t2.bind(a2).set(0, rounds)
        top2 = t2.label()
        t2.recv_from(a2, 1).assert_val(W.PING).reply(a2, 1, W.PONG).djnz(0, top2).done()
        tasks += [t1, t2]
    m = wl.main()
    for t in tasks:
        m.spawn(t)
    for t in tasks:
        m.join(t)
    m.done()
    return wl.build(), A.Config.default(packet_loss_rate=loss), A.Limits()


def scope(stamp=False, rounds=6):
    """A client that asks under `timeout(30 ms, recv)` and traces what each round gave it — the answer or VAL_TIMEOUT — on a network that
    loses a fifth of the datagrams: the scope build."""
    st = _Stamper(stamp)
    wl = W.WorkloadBuilder()
    n1, n2 = wl.create_node(), wl.create_node()
    a1, a2 = wl.addr(n1, 1), wl.addr(n2, 1)
    srv = wl.task(n2)
    srv.bind(a2)
    top = srv.label()
    srv.recv_from(a2, 1).reply(a2, 1, W.PONG).jmp(top)
    cl = wl.task(n1)
    st(cl.bind(a1).sleep(ms=5).trace(0x40)).set(0, rounds)
    top = cl.label()
    cl.send_to(a1, a2, 1, W.PING)
    h = cl.timeout_begin(ms=30)
    cl.recv_from(a1, 1)
    cl.timeout_end(h)
    st(cl.trace_val()).djnz(0, top)
    st(cl.trace(0x41)).done()
    m = wl.main()
    m.spawn(srv).spawn(cl).join(cl).done()
    lim = A.Limits()
    lim.mbox_regs = 8            # (a timed-out receive leaves its registration behind: under the default the device answers some seeds with MADSIM_OVERFLOW)
    return wl.build(), A.Config.default(packet_loss_rate=0.2), lim


def scope_small_limits():
    """scope() under the default limits: a share of the seeds overflow the mailbox registrations first — what resolve= is for."""
    w, cfg, _ = scope()
    return w, cfg, A.Limits()


def ticker(stamp=False, rounds=8):
    """A 10 ms ticker whose body sleeps a random 0 .. 25 ms: most ticks run late, so the traced value (the deadline) lies before the clock
    the time row must hold.  Ends with trace_system_time: the clock plus the seed's base time."""
    st = _Stamper(stamp)
    wl = W.WorkloadBuilder()
    t = wl.task(wl.create_node())
    st(t.interval(ms=10).trace(0x70)).set(0, rounds)
    top = t.label()
    st(t.tick(trace=True)).sleep_rand(lo_ms=0, ms=25).djnz(0, top)
    st(t.trace(0x71))
    st(t.trace_system_time()).done()
    m = wl.main()
    m.spawn(t).join(t).done()
    return wl.build(), A.Config.default(), A.Limits()


def select(stamp=False, rounds=8):
    """`select! { recv, tick }` on a 20 ms ticker against a sender that sends after random sleeps: the receiver traces what each select
    gave it, the message or VAL_TIMEOUT.  The select build."""
    st = _Stamper(stamp)
    wl = W.WorkloadBuilder()
    n1, n2 = wl.create_node(), wl.create_node()
    a1, a2 = wl.addr(n1, 1), wl.addr(n2, 1)
    snd = wl.task(n2)
    snd.bind(a2).set(0, rounds)
    top = snd.label()
    snd.sleep_rand(lo_ms=0, ms=40).send_to(a2, a1, 1, W.PING).djnz(0, top).done()
    rcv = wl.task(n1)
    rcv.bind(a1).interval(ms=20).set(0, rounds)
    top = rcv.label()
    rcv.recv_or_tick(a1, 1)
    st(rcv.trace_val()).djnz(0, top)
    st(rcv.trace(0x60)).done()
    m = wl.main()
    m.spawn(snd).spawn(rcv).join(rcv).done()
    lim = A.Limits()
    lim.mbox_regs = 8            # (as in scope(): a select the tick won leaves the receive's registration behind)
    return wl.build(), A.Config.default(), lim


def signal(stamp=False):
    """A task that waits for ctrl-c, and a main that sends it after a random sleep: 0x50 when the handler is about to be installed, 0x51
    when the signal has arrived, then the system time.  The ctrl-c build."""
    st = _Stamper(stamp)
    wl = W.WorkloadBuilder()
    n = wl.create_node()
    t = wl.task(n)
    st(t.trace(0x50)).ctrl_c()
    st(t.trace(0x51))
    st(t.trace_system_time()).done()
    m = wl.main()
    m.spawn(t).sleep_rand(lo_ms=50, ms=500).send_ctrl_c(n).join(t).done()
    return wl.build(), A.Config.default(), A.Limits()


def case(name, stamp=False):
    return {"pingpong": pingpong, "scope": scope, "ticker": ticker, "select": select, "signal": signal}[name](stamp)


# spans worth asking of each workload: constants its test body traces (a traced time is no span end: it differs from seed to seed)
SPANS_OF = {"pingpong": [(0x10, 0x20), (0x11, 0x21), (None, 0x20), (0x30, 0x30)],
            "scope": [(0x40, 0x41), (None, 0x41), (A.VAL_TIMEOUT, A.VAL_TIMEOUT), (0x40, A.VAL_TIMEOUT)],
            "ticker": [(0x70, 0x71), (None, 0x70), (None, 0x71)],
            "select": [(A.VAL_TIMEOUT, 0x60), (None, 0x60), (W.PING, W.PING), (A.VAL_TIMEOUT, W.PING)],
            "signal": [(0x50, 0x51), (None, 0x51), (None, 0x50)]}
