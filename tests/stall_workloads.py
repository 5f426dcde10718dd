"""Directed, seed-independent workloads for the task log (include/madsim_hip.h "Task post-mortems"): each comes with the table every seed
must end with, written by hand from the program text — the pcs are read off the WorkloadBuilder labels, nothing comes from the code
under test.  Shared by tests/test_stall_emu.py (the device code compiled for the host) and tests/test_stall_gpu.py.

A case is (workload, limits, expected verdict, expected records in task-slot order).  Slots: the main task is spawned first (slot 0), a
spawn takes the lowest free slot, and every main below spawns its children in one poll — so the children sit in slots 1, 2, ... in spawn
order."""
from madsim_amd import _abi as A
from madsim_amd import workload as W
from tests import stall_ref as R

S = 1_000_000_000


def _abs(built, task, label):
    """The index into the workload's instruction array of `label` (TaskBuilder.label(): relative to its program)."""
    return built.progs[task.index].entry + label


def leak():
    """(a) The main spawns a task that recv_froms for ever, sleeps 1 s and ends: PASS, one PARKED record."""
    wl = W.WorkloadBuilder()
    n = wl.create_node()
    a = wl.addr(n, 1)
    t = wl.task(n)
    t.bind(a)
    at = t.label()
    t.recv_from(a, 1)
    t.done()
    m = wl.main()
    m.spawn(t); m.sleep(secs=1); m.done()
    b = wl.build()
    return b, A.Limits(), A.PASS, [R.word(R.PARKED, t.index, _abs(b, t, at))]


def panic():
    """(b) The main spawns a child and panics in the same poll: the main PANICKED at the PANIC, the child QUEUED at its entry."""
    wl = W.WorkloadBuilder()
    n = wl.create_node()
    t = wl.task(n)
    t.sleep(secs=100); t.done()
    m = wl.main()
    m.spawn(t)
    at = m.label()
    m.panic(3)
    b = wl.build()
    return b, A.Limits(), A.PANIC, [R.word(R.PANICKED, 0, _abs(b, m, at)), R.word(R.QUEUED, t.index, _abs(b, t, 0))]


def abort():
    """(c) As (b) with a yield and an abort before the panic: the child is CANCELLED — at its entry whether the executor polled it during
    the yield (it parked in the sleep that is its first instruction) or not."""
    wl = W.WorkloadBuilder()
    n = wl.create_node()
    t = wl.task(n)
    t.sleep(secs=100); t.done()
    m = wl.main()
    m.spawn(t); m.yield_now(); m.abort(t)
    at = m.label()
    m.panic(3)
    b = wl.build()
    return b, A.Limits(), A.PANIC, [R.word(R.PANICKED, 0, _abs(b, m, at)), R.word(R.CANCELLED, t.index, _abs(b, t, 0))]


def fused_assert(alone=False):
    """A failing assert_eq!(val, ..): behind an awaiting op (the device fuses it into that op's completion) or, alone=True, behind a
    straight-line op.  Either way the record names the ASSERT_VAL instruction; the loop registers are the panicking poll's."""
    wl = W.WorkloadBuilder()
    m = wl.main()
    m.set(0, 5); m.set(1, 7)
    m.sleep(ms=2)
    if alone:
        m.trace(1)
    at = m.label()
    m.assert_val(123)
    m.done()
    b = wl.build()
    return b, A.Limits(), A.PANIC, [R.word(R.PANICKED, 0, _abs(b, m, at), 5, 7)]


def crowd(n_children):
    """(e) n_children parked children and a main that then panics.  The children are instances of one program, spawned in a djnz loop; each
    sets its loop registers and sleeps.  The main's loop register has counted down to 0 when it panics."""
    wl = W.WorkloadBuilder()
    n = wl.create_node()
    t = wl.task(n)
    t.set(0, 5); t.set(1, 7)
    tat = t.label()
    t.sleep(secs=100); t.done()
    m = wl.main()
    m.set(0, n_children)
    top = m.label()
    m.spawn(t); m.djnz(0, top)
    m.sleep(secs=1)
    at = m.label()
    m.panic(3)
    b = wl.build()
    lim = A.Limits()
    lim.max_tasks = n_children + 4
    lim.heap_lds_slots, lim.heap_spill_slots = 8, 256        # (every child's sleep is a timer: more than the default heap holds)
    return b, lim, A.PANIC, [R.word(R.PANICKED, 0, _abs(b, m, at))] + [R.word(R.PARKED, t.index, _abs(b, t, tat), 5, 7)] * n_children


TIERS = ("base", "scope", "tick", "select", "signal")
ALARM_NS, LIMIT_NS = 20 * S, 10 * S


def time_limit(tier):
    """(d) Under a 10 s time limit one task is parked in every awaiting op the tier's trace build has, each PARKED at its own pc; the "alarm"
    task's 20 s sleep is the first timer past the limit — the executor fires it on the jump that ends the run — so it is QUEUED at its SLEEP.
    Every other timer lies beyond 20 s (the sleep_rand's only for the seeds whose clock the caller has checked: its range begins at
    12.75 s).  The main is parked in the join of the first child."""
    wl = W.WorkloadBuilder()
    tasks = []                                   # (task, label of the instruction it ends at, state)

    def one(body, node=None, state=R.PARKED):
        node = wl.create_node() if node is None else node
        t = wl.task(node)
        at = body(t, node)
        t.done()
        tasks.append((t, at, state))
        return t

    def sleeper(t, node):
        at = t.label(); t.sleep(secs=100); return at

    def until(t, node):
        t.mark(); at = t.label(); t.sleep_until(secs=100); return at

    def recv(t, node):
        a = wl.addr(node, 1); t.bind(a); at = t.label(); t.recv_from(a, 1); return at

    def recv_timeout(t, node):
        a = wl.addr(node, 1); t.bind(a); at = t.label(); t.recv_from_timeout(a, 1, secs=100); return at

    def accept(t, node):
        a = wl.addr(node, 1); t.bind(a); at = t.label(); t.accept1(a); return at

    def rand(t, node):
        at = t.label(); t.sleep_rand(lo_ms=12750, secs=60000); return at

    def alarm(t, node):
        at = t.label(); t.sleep(secs=20); return at

    # the base classes, which every trace build compiles in (the ctrl-c builds too: only the timer tiers are kept apart from them)
    one(sleeper); one(until); one(recv); one(recv_timeout); one(accept); one(rand)
    # a connection whose two ends both wait for a payload nobody sends
    srv_node, cli_node = wl.create_node(), wl.create_node()
    sa, ca = wl.addr(srv_node, 1), wl.addr(cli_node, 1)

    def server(t, node):
        t.bind(sa); t.accept1(sa); at = t.label(); t.chan_recv(); return at

    def client(t, node):
        t.bind(ca); t.sleep(secs=1); t.connect1(ca, sa); at = t.label(); t.chan_recv(); return at

    one(server, srv_node); one(client, cli_node)
    # a typed call to an address nobody has bound: the request is dropped, the response never comes, and there is no timeout
    nobody = wl.addr(wl.create_node(), 9)

    def call(t, node):
        a = wl.addr(node, 1); t.bind(a); at = t.label(); t.rpc_call(a, nobody, 1, 7); return at

    one(call)
    if tier == "signal":
        def ctrl_c(t, node):
            at = t.label(); t.ctrl_c(); return at

        def recv_or_ctrl_c(t, node):
            a = wl.addr(node, 1); t.bind(a); at = t.label(); t.recv_or_ctrl_c(a, 1); return at

        one(ctrl_c); one(recv_or_ctrl_c)
    if tier in ("scope", "tick", "select"):
        def scoped(t, node):                 # the task stands at the await inside the block, not at TIMEOUT_BEGIN
            a = wl.addr(node, 1); t.bind(a)
            h = t.timeout_begin(secs=100); at = t.label(); t.recv_from(a, 1); t.timeout_end(h); return at
        one(scoped)
    if tier in ("tick", "select"):
        def ticker(t, node):                 # the first tick comes at once; the second waits a period
            t.interval(secs=100); t.tick(); at = t.label(); t.tick(); return at
        one(ticker)
    if tier == "select":
        def recv_or_tick(t, node):
            a = wl.addr(node, 1); t.bind(a); t.interval(secs=100); t.tick(); at = t.label(); t.recv_or_tick(a, 1); return at

        def timeout_at(t, node):
            a = wl.addr(node, 1); t.bind(a); t.mark(); at = t.label(); t.recv_from_timeout_at(a, 1, secs=100); return at

        one(recv_or_tick); one(timeout_at)
    one(alarm, state=R.QUEUED)
    m = wl.main()
    for t, _, _ in tasks:
        m.spawn(t)
    at = m.label()
    m.join(tasks[0][0]); m.done()
    b = wl.build()
    lim = A.Limits()
    lim.time_limit_ns = LIMIT_NS
    lim.max_tasks = len(tasks) + 4
    want = [R.word(R.PARKED, 0, _abs(b, m, at))] + [R.word(st, t.index, _abs(b, t, lab)) for t, lab, st in tasks]
    return b, lim, A.TIME_LIMIT, want


def time_limit_seeds(built, lim, n=65, first=1):
    """The first n seeds from `first` whose run, by the oracle's clock, ends on the alarm's timer: the jump to 20 s + 50 ns.  (A seed whose
    sleep_rand drew less than 20 s ends earlier; none of the first hundreds does — the range is 12.75 s .. 60 000 s.)"""
    import oracle
    out, s = [], first
    while len(out) < n:
        res, _ = oracle.run_batch(built, s, 256, limits=lim)
        for i in range(256):
            if len(out) < n and int(res["verdict"][i]) == A.TIME_LIMIT and ALARM_NS <= int(res["clock_ns"][i]) < ALARM_NS + S:
                out.append(s + i)
        s += 256
        assert s < first + 4096, "the oracle finds no seed that ends on the alarm"
    return out
