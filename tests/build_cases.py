"""The cases of tests/test_emu_build_matrix.py and tests/test_gpu_build_matrix.py (test infrastructure): every op family on every kernel build
that compiles it.

sim_kernel is one source compiled into the builds of MADSIM_FOR_EACH_VARIANT (sim_kernel.h) — each its own machine code, register allocation
and spills, with handlers that branch on the build's properties — and a seed says nothing about a build it did not run on.  The fuzz suites
reach every build, but each tier build only with its own family's generator, and the single-class, narrow and stride builds with whatever
happens to select them.  Here every non-trace row of variant_table gets (workload, config, limits) cases that

  * select exactly that row (each case asserts it: the library's geometry, the host-compiled kernel's, and the row it then really ran on),
  * together make the ORACLE poll every opcode the row compiles (oracle.OracleStats.op_polls: the device equals the oracle seed for seed, so
    what the oracle polled in these seeds the device polled too — no build needs instrumenting for the premise), and
  * are compared with parity.expected on all 48 result bytes of 130 seeds, no seed of the pass a runner verdict.

What a row compiles follows from OP_CLASS — per opcode the MADSIM_FEAT_* classes its handler is compiled under, held against the library
(a one-op workload's build carries exactly those classes).  The (row, opcode) pairs left out are EXCLUSIONS, each with its reason: the
handler is not compiled into the row (its `!K::Fx` guard is all the row has), or the host refuses the combination (asserted, with the error
code).  One row, sim_kernel<Variant<false, true, -1, 31, false, false>>, is compiled and named by no parameter block at all
(UNSELECTABLE: select_variant over every block it can read never returns it — asserted on the host-compiled select_variant).

carrier(workload, family) appends one task that uses a family's ops, so that a workload of another family selects the family's build; the
truth is the oracle on the same — carried — workload, so the carrier needs no neutrality argument.

tools/build_coverage.py measures what these cases reach line by line (gcov on the host-compiled kernel, per build); tools/build_mutants.py
shows what they see that the rest of the suite does not; profiles/build_matrix.md records both."""
import numpy as np

import oracle
from madsim_amd import _abi as A
from madsim_amd import workload as W
from tests import lifecycle_workloads as LW
from tests import parity

SEEDS = 130             # two full waves and two lanes at 64 seed lanes per wave
SEED0 = 11
TRACE_SEEDS = 8
GOLDEN_SEEDS = 8        # per sampled workload, against tests/golden/make_golden_async.py

TIME, CHAN, RPC, NODE, ADDR, ALL = 1, 2, 4, 8, 16, 31            # sim_kernel.h MADSIM_FEAT_*
NOLOG, COMPACT, NARROW = 32, 64, 128                             # (layout words of a build's name: no op class)
SCOPE, TICK, SELECT, SIGNAL = 256, 512, 1024, 2048
TIERS = SCOPE | TICK | SELECT
PLAIN = ALL & ~ADDR
E_WORKLOAD = "malformed workload"                                # madsim_hip_strerror(MADSIM_E_WORKLOAD)

# ---- opcode -> the classes its handler is compiled under (0: every build) -------------------------------------------------------------------
OP_CLASS = dict(
    DONE=0, SPAWN=0, JOIN=0, YIELD=0, PANIC=0, SET=0, DJNZ=0, JMP=0, TRACE=0, SLEEP=0, BIND=0, SEND=0, REPLY=0, RECV=0, ASSERT_VAL=0, CLOSE=0,
    CLOG_NODE=0, UNCLOG_NODE=0, CLOG_LINK=0, UNCLOG_LINK=0, SET_LOSS=0, SLEEP_RAND=0, GSET=0, GADD=0, ASSERT_G=0, PANIC_IF_G_LT=0, JEQ=0,
    RAND_BOOL=0, RANDOM=0,
    MARK=TIME, SLEEP_UNTIL=TIME, ASSERT_ELAPSED=TIME, ADVANCE=TIME, RECV_TIMEOUT=TIME, TRACE_TIME=TIME, SET_LATENCY=TIME,
    CONNECT=CHAN, ACCEPT=CHAN, CSEND=CHAN, CRECV=CHAN, CCLOSE=CHAN,
    RPC_CALL=RPC | TIME, RPC_REPLY=RPC | TIME, HOOK_REQ=RPC | TIME, HOOK_RSP=RPC | TIME,
    ABORT=NODE, BUILD=NODE, KILL=NODE, RESTART=NODE, PAUSE=NODE, RESUME=NODE, ASSERT_EXIT=NODE,
    IPVS=ADDR,
    TIMEOUT_BEGIN=SCOPE, TIMEOUT_END=SCOPE,
    INTERVAL=TICK, TICK=TICK, INTERVAL_RESET=TICK,
    RECV_OR_TICK=SELECT | TICK | TIME, RECV_TIMEOUT_AT=SELECT | TICK | TIME,
    CTRL_C=SIGNAL | NODE, SEND_CTRL_C=SIGNAL | NODE, RECV_OR_CTRL_C=SIGNAL | NODE | TIME,
)
assert set(OP_CLASS) == set(A.OP)
OP_NAME = {v: k for k, v in A.OP.items()}


def one_op_workload(op):
    """The smallest valid workload whose only op beyond DONE is `op` (what OP_CLASS is held against the library with)."""
    wl = W.WorkloadBuilder()
    n = wl.create_node()
    s = wl.addr(n, 1)
    m = wl.main()
    other = wl.task(n) if op in ("SPAWN", "JOIN", "ABORT") else None
    if op == "IPVS":
        m.ipvs_add_server(wl.ipvs_service(wl.virtual_addr(1, 80)), s)
    elif op in ("SLEEP_UNTIL", "ASSERT_ELAPSED", "RECV_TIMEOUT_AT"):
        m._emit(op, a=s if op == "RECV_TIMEOUT_AT" else 1)              # (Rust refuses a use of t0 before its assignment: so does validate())
        m.code.insert(0, [A.OP["MARK"], 0, 0, 0, False])
    elif op in ("TICK", "INTERVAL_RESET", "RECV_OR_TICK"):
        m.interval(ms=1)._emit(op, a=s if op == "RECV_OR_TICK" else 0)
    elif op == "TIMEOUT_BEGIN" or op == "TIMEOUT_END":
        with m.timeout(ms=1):
            m.yield_now()
    elif op in ("DJNZ", "JMP", "JEQ"):
        m._emit(op, b=1, reloc=True)
    elif other is not None:
        m._emit(op, a=other.index)
    elif op == "INTERVAL":
        m.interval(ms=1)
    elif op in ("BUILD", "KILL", "RESTART", "PAUSE", "RESUME", "CLOG_NODE", "UNCLOG_NODE", "CLOG_LINK", "UNCLOG_LINK", "ASSERT_EXIT", "SEND_CTRL_C", "HOOK_REQ", "HOOK_RSP"):
        m._emit(op, a=n, b=n if "LINK" in op else 0x8000 if op == "HOOK_REQ" else 0)
    elif op != "DONE":
        m._emit(op, a=s if op in ("BIND", "SEND", "REPLY", "RECV", "CLOSE", "RECV_TIMEOUT", "CONNECT", "ACCEPT", "RPC_CALL", "RPC_REPLY", "RECV_OR_CTRL_C") else 0, b=(s | 0x8000) if op == "RPC_CALL" else s if op in ("SEND", "CONNECT") else 0)
    m.done()
    return wl.build()


# ---- rows: the non-trace builds, each with the limits that select it ------------------------------------------------------------------------
def _lim(**kw):
    lim = A.Limits()
    for k, v in kw.items():
        setattr(lim, k, v)
    return lim


def _v(spill, lws, feat, rq, g, trace=False):
    b = lambda x: "true" if x else "false"      # noqa: E731
    return f"sim_kernel<Variant<{b(trace)}, {b(spill)}, {lws}, {feat}, {b(rq)}, {b(g)}>>"


G, NH, LDS = A.STATE_GLOBAL, A.STATE_NARROW_HEAP, A.STATE_LDS
NO_SPILL = dict(heap_lds_slots=12, heap_spill_slots=0)          # a heap that lives in LDS whole
SPILL = dict(heap_lds_slots=3, heap_spill_slots=61)             # two levels in LDS, the rest spilled: the spill path is walked, not just compiled


class Row:
    """variant: the build's name; sel = (trace, spill, lws, feat, rq, g), its row of variant_table; limits: what selects it within its group
    (lane stride, state_mem, the heap split, MADSIM_STATE_NARROW_HEAP, no_trace_hash); lift: the carriers that bring a workload of fewer
    classes onto it; addr: the row takes workloads with general addresses only (True), without only (False), either (None)."""

    def __init__(self, spill, lws, feat, rq, g, limits, lift=(), addr=None, small=False):
        self.sel = (0, int(spill), lws, feat, int(rq), int(g))
        self.variant, self.feat, self.limits, self.lift, self.addr, self.small = _v(spill, lws, feat, rq, g), feat, limits, tuple(lift), addr, small


def _tier_rows(name, m, fam):
    return {
        f"{name}_lds":    Row(1, -1, ALL | m, 0, 0, dict(state_mem=LDS), lift=("all", fam)),
        f"{name}_g":      Row(1, 6, PLAIN | m, 0, 1, dict(state_mem=G, **SPILL), lift=("all", fam), addr=False),
        f"{name}_g_addr": Row(1, 6, ALL | m, 0, 1, dict(state_mem=G, **SPILL), lift=("all", "addr", fam), addr=True),
    }


ROWS = {
    # base ops on full waves: (spill region) x (register ready queue), the twins without the determinism-log fold, the compact layout
    "queue_lds":        Row(0, 6, 0, 0, 0, dict(max_tasks=16, lanes_per_wave=64, **NO_SPILL)),
    "rq_lds":           Row(0, 6, 0, 1, 0, dict(state_mem=LDS, **NO_SPILL), small=True),
    "queue_lds_nolog":  Row(0, 6, NOLOG, 0, 0, dict(max_tasks=16, lanes_per_wave=64, no_trace_hash=1, **NO_SPILL)),
    "rq_lds_nolog":     Row(0, 6, NOLOG, 1, 0, dict(state_mem=LDS, no_trace_hash=1, **NO_SPILL), small=True),
    "compact":          Row(0, 6, COMPACT, 1, 0, dict(state_mem=A.STATE_COMPACT, **NO_SPILL), small=True),
    "compact_nolog":    Row(0, 6, COMPACT | NOLOG, 1, 0, dict(state_mem=A.STATE_COMPACT, no_trace_hash=1, **NO_SPILL), small=True),
    "rq_spill":         Row(1, 6, 0, 1, 0, dict(**SPILL), small=True),
    "queue_spill":      Row(1, 6, 0, 0, 0, dict(max_tasks=16, lanes_per_wave=64, **SPILL)),
    "stride32":         Row(1, -1, 0, 0, 0, dict(max_tasks=16, lanes_per_wave=32, **SPILL)),
    # single-class builds, LDS-resident
    "time_lds":         Row(1, -1, TIME, 0, 0, dict(state_mem=LDS, **SPILL), lift=("time",)),
    "chan_lds":         Row(1, -1, CHAN, 0, 0, dict(state_mem=LDS, **SPILL), lift=("chan",)),
    # every class, LDS-resident: full waves without and with a spill region, then the compile-time strides 32, 16, 8
    "all_lds64_nospill": Row(0, 6, ALL, 0, 0, dict(state_mem=LDS, lanes_per_wave=64, **NO_SPILL), lift=("all",)),
    "all_lds64":        Row(1, 6, ALL, 0, 0, dict(state_mem=LDS, lanes_per_wave=64, **SPILL), lift=("all",)),
    "all_lds32":        Row(1, 5, ALL, 0, 0, dict(state_mem=LDS, lanes_per_wave=32, **SPILL), lift=("all",)),
    "all_lds16":        Row(1, 4, ALL, 0, 0, dict(state_mem=LDS, lanes_per_wave=16, **SPILL), lift=("all",)),
    "all_lds8":         Row(1, 3, ALL, 0, 0, dict(state_mem=LDS, lanes_per_wave=8, **SPILL), lift=("all",)),
    # global state: the single-class builds (timeouts at 64 and 32 lanes; the channel with and without a spill region), plain and general addresses
    "g_time64":         Row(1, 6, TIME, 0, 1, dict(state_mem=G, **SPILL), lift=("time",)),
    "g_time32":         Row(1, 5, TIME, 0, 1, dict(state_mem=G, lanes_per_wave=32, **SPILL), lift=("time",)),
    "g_chan":           Row(1, 6, CHAN, 0, 1, dict(state_mem=G, **SPILL), lift=("chan",)),
    "g_chan_nospill":   Row(0, 6, CHAN, 0, 1, dict(state_mem=G, heap_lds_slots=8, heap_spill_slots=0), lift=("chan",)),
    "g_plain":          Row(1, 6, PLAIN, 0, 1, dict(state_mem=G, **SPILL), lift=("all",), addr=False),
    "g_addr":           Row(1, 6, ALL, 0, 1, dict(state_mem=G, **SPILL), lift=("all", "addr"), addr=True),
    # ... with narrow (8-byte) heap entries
    "g_time64_nh":      Row(1, 6, TIME | NARROW, 0, 1, dict(state_mem=G | NH, **SPILL), lift=("time",)),
    "g_time32_nh":      Row(1, 5, TIME | NARROW, 0, 1, dict(state_mem=G | NH, lanes_per_wave=32, **SPILL), lift=("time",)),
    "g_plain_nh":       Row(1, 6, PLAIN | NARROW, 0, 1, dict(state_mem=G | NH, **SPILL), lift=("all",), addr=False),
}
ROWS.update(_tier_rows("scope", SCOPE, "scope"))
ROWS.update(_tier_rows("tick", SCOPE | TICK, "tick"))
ROWS.update(_tier_rows("select", TIERS, "select"))
ROWS.update(_tier_rows("signal", SIGNAL, "signal"))

# compiled, and named by no parameter block: select_variant answers the compile-time strides for 8, 16 and 32 seed lanes and the two full-wave
# builds for 64 — make_geometry admits no other stride — so the run-time-stride every-class build has no caller (asserted:
# test_emu_build_matrix.py::test_the_unselectable_row, over every block select_variant can read)
UNSELECTABLE = {(0, 1, -1, ALL, 0, 0): "select_variant never names it: every lane stride make_geometry admits has a compile-time every-class build"}
# the trace rows: (row of variant_table, the non-trace row whose cases it runs — the LDS-resident build of the same tier)
TRACE_ROWS = {"trace": ((1, 1, -1, ALL, 0, 0), "all_lds64"), "trace_scope": ((1, 1, -1, ALL | SCOPE, 0, 0), "scope_lds"),
              "trace_tick": ((1, 1, -1, ALL | SCOPE | TICK, 0, 0), "tick_lds"), "trace_select": ((1, 1, -1, ALL | TIERS, 0, 0), "select_lds"),
              "trace_signal": ((1, 1, -1, ALL | SIGNAL, 0, 0), "signal_lds")}


def compiled_ops(feat):
    """The opcodes whose handlers a build with this FEAT word compiles: every class of the op is among the build's."""
    have = feat & (ALL | TIERS | SIGNAL)
    return sorted(op for op, cls in OP_CLASS.items() if cls & ~have == 0)


# ---- the pairs left out, each with its reason ------------------------------------------------------------------------------------------------
GUARD = "not compiled into this build: its classes are not the build's (a `!K::Fx` guard, or no code at all)"
REFUSED = "the host refuses the combination (MADSIM_E_WORKLOAD): ctrl-c signals and a timer-op tier share no build"


def exclusions():
    """{(row name, opcode): reason} — every pair no case of the row polls.  Two reasons only.  GUARD pairs are decided by OP_CLASS (held
    against the library); REFUSED pairs name the ops of the other side of validate()'s signals / tiers rule, which the row could compile
    only if a build carried both — each is a GUARD pair too, and the refusal itself is a case (refused_workloads)."""
    out = {}
    for name, feat in row_feats().items():
        for op in A.OP:
            if op in compiled_ops(feat):
                continue
            tier_op, sig_op = OP_CLASS[op] & TIERS, OP_CLASS[op] & SIGNAL
            out[name, op] = REFUSED if (sig_op and feat & TIERS) or (tier_op and feat & SIGNAL) else GUARD
    return out


def row_feats():
    """{row name: FEAT word} of every row with cases, the trace rows included."""
    return {**{name: row.feat for name, row in ROWS.items()}, **{name: sel[3] for name, (sel, _) in TRACE_ROWS.items()}}


def refused_workloads():
    """(what, workload) whose geometry the host must refuse with MADSIM_E_WORKLOAD: every signal op beside every tier family."""
    for sig in ("ctrl_c", "send_ctrl_c", "recv_or_ctrl_c"):
        for fam in ("scope", "tick", "select"):
            wl = W.WorkloadBuilder()
            n = wl.create_node()
            s = wl.addr(n, 1)
            t = wl.task(n)
            t.bind(s)
            if sig == "ctrl_c":
                t.ctrl_c()
            elif sig == "send_ctrl_c":
                t.send_ctrl_c(n)
            else:
                t.recv_or_ctrl_c(s, 1)
            m = wl.main()
            m.spawn(t)
            m.sleep(ms=5)
            yield (sig, fam), carrier(wl.build(), fam)


# ---- carriers ---------------------------------------------------------------------------------------------------------------------------------
FAMILIES = ("time", "chan", "all", "addr", "scope", "tick", "select", "signal")


def carrier(w, family):
    """`w` with one more task, spawned before block_on on a node of its own, that uses `family`'s ops — so that geometry.h's uses_op
    selects the family's build for a workload that has none of them:

      time    mark(); sleep_until()                                            (MADSIM_FEAT_TIME, nothing else)
      chan    connect1() to an address nobody listens on: refused              (MADSIM_FEAT_CHAN, nothing else)
      all     mark(); assert_exit(own node, false)                             (TIME | NODE: neither single class, so every class)
      addr    bind(0.0.0.0:7); close()                                         (a table entry that is no node IP: general address resolution)
      scope   a scope around a sleep that completes, one around a sleep that expires
      tick    a ticker loop of five ticks and a reset
      select  recv_or_tick and recv_from_timeout_at on a socket of its own, which nobody sends to
      signal  a ctrl-c handler (nobody sends the signal)

    The instructions are appended behind the table, so no pc of `w` moves."""
    assert family in FAMILIES, family
    n_socks, n_services = w.struct.n_socks, w.struct.n_services
    nodes, progs, socks, insns = list(w.nodes), list(w.progs), list(w.socks)[:n_socks], list(w.insns)
    services = list(w.services)[:n_services]
    node = len(nodes)
    nodes.append(A.Node())
    t = W.TaskBuilder(None, len(progs), node, A.PROG_PRE)
    if family in ("addr", "select", "chan"):
        socks.append(A.Sock(node, A.ADDR_UNSPECIFIED if family == "addr" else A.ADDR_IP, 7))
        if family == "chan":
            socks.append(A.Sock(node, A.ADDR_IP, 8))
    own = len(socks) - 1
    if family == "time":
        t.mark().sleep_until(ms=2)
    elif family == "chan":
        t.bind(own - 1).connect1(own - 1, own).chan_close()
    elif family == "all":
        t.mark().assert_exit(node, False)
    elif family == "addr":
        t.bind(own).close(own)
    elif family == "scope":
        with t.timeout(ms=5):
            t.sleep(ms=2)
        with t.timeout(ms=2):
            t.sleep(ms=5)
    elif family == "tick":
        t.interval(ms=3).set(0, 5)
        top = t.label()
        t.tick().djnz(0, top).interval_reset().tick()
    elif family == "select":
        t.mark().bind(own).interval(ms=3).recv_or_tick(own, 1).recv_from_timeout_at(own, 1, ms=9)
    else:
        t.ctrl_c()
    t.done()
    base = len(insns)
    progs.append(A.Prog(node, A.PROG_PRE, base))
    for op, a, b, imm, reloc in t.code:
        insns.append(A.Insn(op, a, (b + base) if reloc else b, imm))
    pm = (list(w.panic_match) + [0] * 8) if w.panic_match is not None else None
    out = W.BuiltWorkload(nodes, progs, socks, insns, services, pm, w.struct.panic_dyn_max)
    out.carried = getattr(w, "carried", ()) + (family,)
    return out


# ---- directed workloads of one class each (the single-class and base-op rows need workloads with nothing else in them) -----------------------
def base_ops():
    """Every base op but PANIC, in eight tasks at most (the register ready queue's), sleeps below a second (the compact layout's horizon).
    Each network switch is observable: the pinger's first three datagrams leave under a clogged node, a clogged link and a loss rate of 1
    and must never arrive — the ponger asserts that the first value it sees is the fourth."""
    wl = W.WorkloadBuilder()
    n1, n2 = wl.create_node(), wl.create_node()
    a1, a2 = wl.addr(n1, 1), wl.addr(n2, 1)
    pong = wl.task(n2)
    pong.bind(a2).set(0, 3)
    top = pong.label()
    pong.recv_from(a2, 1).assert_val(4).reply(a2, 2, W.PONG).flag_add(1, 1).djnz(0, top).close(a2)
    ping = wl.task(n1)
    ping.bind(a1).sleep(ms=10).send_to(a1, a2, 1, 1).sleep(ms=20).send_to(a1, a2, 1, 2).sleep(ms=20).send_to(a1, a2, 1, 3).sleep(ms=20)
    ping.set(1, 3)
    top = ping.label()
    ping.send_to(a1, a2, 1, 4).recv_from(a1, 2).assert_val(W.PONG).trace(100, add_reg=1).djnz(1, top)
    dice = wl.task(n1)
    dice.random_u32().set(0, 6)
    top = dice.label()
    dice.getrandom_byte()                               # (base ops can only compare a value: one draw in 32 takes the branch that traces)
    hit = dice.label() + 9
    for v in range(8):
        dice.jeq(v, hit)
    dice.jmp(hit + 1)
    assert dice.label() == hit
    dice.trace(50, add_reg=0).djnz(0, top).rand_bool(1)
    skip = dice.label() + 3
    dice.jeq(1, skip).yield_now().trace(7)
    assert dice.label() == skip
    dice.sleep_rand(lo_ms=50, ms=300).rand_bool(2).assert_val(1).rand_bool(0).assert_val(0)
    out = dice.label() + 2
    dice.jmp(out).panic(9)
    assert dice.label() == out
    dice.flag_add(1, 10)
    m = wl.main()
    m.flag_store(1, 0).flag_store(2, 5).assert_flag(2, 5).panic_if_flag_lt(2, 5)
    m.spawn(pong).spawn(ping).spawn(dice)
    m.clog_node(n2, "in").sleep(ms=20).unclog_node(n2, "in").clog_link(n1, n2).sleep(ms=20).unclog_link(n1, n2).set_loss(2).sleep(ms=20).set_loss(0)
    m.join(ping).join(pong).join(dice).assert_flag(1, 13)
    return wl.build(), A.Config.default(loss_table=(0.0, 0.5, 1.0)), None


def base_panic():
    """PANIC on a base-op build: a formatted panic!("{}", flag) behind a sleep, in a spawned task (message code = the flag's value)."""
    wl = W.WorkloadBuilder()
    n1 = wl.create_node()
    t = wl.task(n1)
    t.sleep(ms=3).flag_add(0, 2).panic_with_flag(0, 1)
    m = wl.main()
    m.flag_store(0, 4).spawn(t).join(t)
    return wl.build(), None, None


def time_ops():
    """Every op of the time class, and nothing of another: a receive that times out and one that does not, the t0 family, advance(), the
    two clocks traced, and a latency range switched under a datagram in flight."""
    wl = W.WorkloadBuilder()
    n1, n2 = wl.create_node(), wl.create_node()
    a1, a2 = wl.addr(n1, 1), wl.addr(n2, 1)
    rx = wl.task(n2)
    rx.mark().bind(a2).recv_from_timeout(a2, 1, ms=5).assert_val(A.VAL_TIMEOUT).assert_elapsed(">=", ms=5).assert_elapsed("<", ms=12)
    rx.recv_from_timeout(a2, 1, secs=1).assert_val(0xA).assert_elapsed(">=", ms=120).assert_elapsed("<", ms=140).trace_instant()
    tx = wl.task(n1)
    tx.random_u32().trace_val().mark().bind(a1).sleep_until(ms=20).assert_elapsed(">=", ms=20).assert_elapsed("<", ms=21).trace_system_time().set_latency(0).send_to(a1, a2, 1, 0xA)
    tx.sleep(ms=150).advance(ms=300).assert_elapsed(">=", ms=470).assert_elapsed("<", ms=480).trace_instant()
    m = wl.main()
    m.spawn(rx).spawn(tx).join(rx).join(tx)
    return wl.build(), A.Config.default(lat_table=((100_000_000, 101_000_000),)), None


def chan_ops():
    """Every op of the channel class, and nothing of another: three payloads one way in order, one back, then the client's drop resets
    the server's next receive."""
    wl = W.WorkloadBuilder()
    ns, nc = wl.create_node(), wl.create_node()
    asv, acl = wl.addr(ns, 1), wl.addr(nc, 1)
    srv = wl.task(ns)
    srv.bind(asv).accept1(asv).chan_recv().assert_val(1).chan_recv().assert_val(2).chan_recv().assert_val(3).chan_send(9)
    srv.chan_recv().assert_val(A.VAL_RESET)
    cl = wl.task(nc)
    cl.bind(acl).sleep(ms=10).connect1(acl, asv).assert_val(0).chan_send(1).chan_send(2).sleep(ms=30).chan_send(3).chan_recv().assert_val(9).chan_close()
    m = wl.main()
    m.spawn(srv).spawn(cl).join(srv).join(cl)
    return wl.build(), None, None


def guard_ops():
    """The BindGuard of a listening Endpoint (k_channel.h guard_acquire / guard_release): the server drops its Endpoint while the accepted
    pair lives — the port stays taken (bind: AddrInUse) — and drops the pair, the guard's last owner — the socket closes and the same
    address binds again.  Both answers are asserted."""
    wl = W.WorkloadBuilder()
    ns, nc = wl.create_node(), wl.create_node()
    asv, acl = wl.addr(ns, 1), wl.addr(nc, 1)
    srv = wl.task(ns)
    srv.bind(asv).accept1(asv).close(asv).try_bind(asv).assert_val(A.VAL_ADDR_IN_USE).chan_recv().assert_val(1)
    srv.chan_close().try_bind(asv).assert_val(0)
    cl = wl.task(nc)
    cl.bind(acl).sleep(ms=10).connect1(acl, asv).assert_val(0).chan_send(1).sleep(ms=50).chan_close()
    m = wl.main()
    m.spawn(srv).spawn(cl).join(srv).join(cl)
    return wl.build(), None, None


def scope_around_channel():
    """Channel ops inside a timeout scope (k_poll.h: the pair a connect1 of the scope makes is the async block's, noted for the block's
    end): one scope whose block completes — connect, send, receive the echo — and one that expires in its chan_recv, which drops the pair
    and resets the server's receive."""
    wl = W.WorkloadBuilder()
    ns, nc = wl.create_node(), wl.create_node()
    asv, acl = wl.addr(ns, 1), wl.addr(nc, 1)
    srv = wl.task(ns)
    srv.bind(asv).accept1(asv).chan_recv().assert_val(5).chan_send(6).chan_close()
    srv.accept1(asv).chan_recv().assert_val(7).chan_recv().assert_val(A.VAL_RESET)
    cl = wl.task(nc)
    cl.bind(acl).sleep(ms=10)
    with cl.timeout(secs=1):
        cl.connect1(acl, asv).assert_val(0).chan_send(5).chan_recv()
    cl.assert_val(6).trace_val()
    with cl.timeout(ms=40):
        cl.connect1(acl, asv).assert_val(0).chan_send(7).chan_recv()
    cl.assert_val(A.VAL_TIMEOUT).trace_val().sleep(ms=50)
    m = wl.main()
    m.spawn(srv).spawn(cl).join(cl).join(srv)
    return wl.build(), None, None


def node_ops():
    """Every op of the node class on a millisecond scale (inside the narrow heap's horizon): pause / resume hold a ticker back, kill and
    restart run an init task twice, abort cancels a task parked in a receive, build() starts a node from inside a task."""
    wl = W.WorkloadBuilder()
    n1, n2, n3, n4 = (wl.create_node() for _ in range(4))
    t1 = wl.task(n1, pre=True)
    top = t1.label()
    t1.sleep(ms=20).flag_add(0, 2).jmp(top)
    t2 = wl.task(n2, init=True, pre=True)
    t2.flag_store(1, 0)
    top = t2.label()
    t2.sleep(ms=20).flag_add(1, 2).jmp(top)
    a3 = wl.addr(n3, 1)
    t3 = wl.task(n3, pre=True)
    t3.bind(a3).recv_from(a3, 9)
    t4 = wl.task(n4, init=True)
    t4.flag_add(2, 1).sleep(ms=500)
    m = wl.main()
    m.mark().sleep_until(ms=30).assert_flag(0, 2).assert_flag(1, 2)
    m.pause(n1).sleep_until(ms=50).assert_flag(0, 2).resume(n1).sleep_until(ms=55).assert_flag(0, 4)
    m.kill(n2).assert_exit(n2, True).restart(n2).assert_exit(n2, False).sleep_until(ms=70).assert_flag(1, 0).sleep_until(ms=80).assert_flag(1, 2)
    m.abort(t3).join(t3, expect_err=True)
    m.assert_flag(2, 0).build_node(n4).sleep(ms=5).assert_flag(2, 1).assert_exit(n4, False)
    return wl.build(), None, None


def signal_ops():
    """The three signal ops: a select that a datagram wins, one that the signal wins, a plain ctrl_c() that the next signal completes; a
    signal nobody waits for is lost; a node without a handler is killed by it."""
    wl = W.WorkloadBuilder()
    n1, n2, n3 = (wl.create_node() for _ in range(3))
    a1, a3 = wl.addr(n1, 1), wl.addr(n3, 1)
    h = wl.task(n1)
    h.bind(a1).recv_or_ctrl_c(a1, 1).assert_val(5).recv_or_ctrl_c(a1, 1, recv_first=True).assert_val(A.VAL_TIMEOUT).trace(1).ctrl_c().trace(2)
    victim = wl.task(n2)
    victim.sleep(secs=1).trace(3)
    tx = wl.task(n3)
    tx.bind(a3).sleep(ms=10).send_to(a3, a1, 1, 5)
    m = wl.main()
    m.spawn(h).spawn(victim).spawn(tx).sleep(ms=50).send_ctrl_c(n1).sleep(ms=10).send_ctrl_c(n1).sleep(ms=10).send_ctrl_c(n1)
    m.assert_exit(n2, False).send_ctrl_c(n2).assert_exit(n2, True).assert_exit(n1, False).join(h).join(victim, expect_err=True)
    return wl.build(), None, None


def tier_ops():
    """Every timer-tier op in one task: ticks that park and a tick that is due, a reset, a scope around a tick that expires, a select the
    datagram wins and one the tick wins (polled first, its instant folded), timeout_at met and missed."""
    wl = W.WorkloadBuilder()
    n1, n2 = wl.create_node(), wl.create_node()
    a1, a2 = wl.addr(n1, 1), wl.addr(n2, 1)
    t = wl.task(n1)
    t.mark().bind(a1).interval("skip", ms=10).tick(trace=True).tick(trace=True).sleep(ms=25).tick(trace=True).interval_reset()
    with t.timeout(ms=3):
        t.tick()
    t.trace_val().recv_or_tick(a1, 1).trace_val().recv_or_tick(a1, 1, tick_first=True, trace=True).trace_val()
    t.recv_from_timeout_at(a1, 1, ms=200).trace_val().recv_from_timeout_at(a1, 1, ms=210).trace_val().trace_instant()
    tx = wl.task(n2)
    tx.bind(a2).sleep(ms=52).send_to(a2, a1, 1, 7).sleep(ms=60).send_to(a2, a1, 1, 8)
    m = wl.main()
    m.spawn(t).spawn(tx).join(t).join(tx)
    return wl.build(), None, _lim(mbox_regs=8, mbox_msgs=4)         # (a select the tick wins leaves its registration behind)


def graceful_shutdown():
    return W.graceful_shutdown(n_servers=2, n_clients=1, requests=3), None, W.graceful_shutdown_limits()


def _lw(name):
    return lambda: (LW.ALL[name](), LW.config(name), LW.limits(name))


WORKLOADS = dict(base_ops=base_ops, base_panic=base_panic, time_ops=time_ops, chan_ops=chan_ops, guard_ops=guard_ops, node_ops=node_ops, scope_around_channel=scope_around_channel,
                 tier_ops=tier_ops, signal_ops=signal_ops, graceful_shutdown=graceful_shutdown)
WORKLOADS.update({name: _lw(name) for name in LW.ALL})
_BUILT = {}


def built(name, carriers=()):
    """(workload, config, the limits it needs beyond the defaults) of a named workload under its carriers, built once."""
    key = (name, tuple(carriers))
    if key not in _BUILT:
        w, cfg, lim = WORKLOADS[name]() if not carriers else built(name, carriers[:-1])
        _BUILT[key] = (carrier(w, carriers[-1]), cfg, lim) if carriers else (w, cfg, lim)
    return _BUILT[key]


def case_limits(row, need, n_carriers):
    """A row's limits on top of what the workload needs (mailbox, connection and task capacities); a carrier is one task more."""
    lim = A.Limits()
    if need is not None:
        for f, _ in A.Limits._fields_:
            setattr(lim, f, getattr(need, f))
    if lim.max_tasks:
        lim.max_tasks += n_carriers
    for k, v in ROWS[row].limits.items():
        setattr(lim, k, max(v, lim.max_tasks) if k == "max_tasks" else v)
    return lim


# ---- cases ------------------------------------------------------------------------------------------------------------------------------------
# The workloads every row draws from, in this order, each with the MADSIM_FEAT_* word geometry.h computes for it (held against the library):
# the directed ones above, and four of tests/lifecycle_workloads.py for what those leave out — typed RPC with both hooks, a latency switch
# under a channel, IPVS (general addresses).
CORE = dict(
    base_ops=0, base_panic=0, time_ops=TIME, chan_ops=CHAN, guard_ops=CHAN, node_ops=TIME | NODE, rpc_hooks=TIME | RPC,
    update_config_latency_channel=TIME | CHAN, ipvs_round_robin_unit_test=ALL & ~(CHAN | NODE | RPC), scope_around_channel=TIME | CHAN | SCOPE,
    tier_ops=TIME | TIERS, signal_ops=TIME | NODE | SIGNAL, graceful_shutdown=TIME | NODE | SIGNAL,
)


def feature_tier(feat):
    """sim_kernel.h feature_tier."""
    if feat & SIGNAL:
        return SIGNAL
    return TIERS if feat & SELECT else SCOPE | TICK if feat & TICK else feat & SCOPE


def carriers_for(row, feat):
    """The carriers under which a workload with features `feat` selects `row` (select_variant's rule, restated), or None when none do."""
    r, rt, cls = ROWS[row], feature_tier(ROWS[row].feat), feat & ALL
    rc = r.feat & ALL
    if feature_tier(feat) & ~rt or (rt == SIGNAL) != bool(feat & SIGNAL) and feat & (TIERS | SIGNAL):
        return None
    if rc == 0:
        return () if feat == 0 else None
    out = []
    if rc in (TIME, CHAN):
        if cls & ~rc:
            return None
        if not cls:
            out.append("time" if rc == TIME else "chan")
    else:
        if not rt and (cls & ~TIME == 0 or cls & ~CHAN == 0):
            out.append("all")
        if r.addr is False and cls & ADDR:
            return None
        if r.addr and not cls & ADDR:
            out.append("addr")
    if rt and feature_tier(feat) != rt:
        out.append(r.lift[-1])
    return tuple(out)


def cases(row):
    """(name, carriers, workload, config, limits) of a row: every CORE workload that some carriers bring onto it."""
    for name, feat in CORE.items():
        cs = carriers_for(row, feat)
        if cs is None:
            continue
        w, cfg, need = built(name, cs)
        yield name, cs, w, cfg, case_limits(row, need, len(cs))


_TRUTH, _POLLED = {}, {}


def truth(row, name, cs):
    """What the build must answer for the SEEDS seeds of a case (parity.expected: the oracle with the model's ceilings off), computed once
    and left unchanged."""
    key = (row, name, cs)
    if key not in _TRUTH:
        w, cfg, need = built(name, cs)
        want = parity.expected(w, SEED0, SEEDS, cfg, case_limits(row, need, len(cs)))
        want.setflags(write=False)
        _TRUTH[key] = want
    return _TRUTH[key]


def polled(row, name, cs, seeds=SEEDS):
    """The opcodes the oracle polls in the first `seeds` seeds of a case."""
    key = (row, name, cs, seeds)
    if key not in _POLLED:
        w, cfg, need = built(name, cs)
        st = oracle.run_batch(w, SEED0, seeds, cfg, case_limits(row, need, len(cs)), want_stats=True)[2]
        _POLLED[key] = frozenset(OP_NAME[i] for i in OP_NAME if st.op_polls[i])
    return _POLLED[key]


def polled_by_row(row):
    """... over the cases of a row; a trace row: over the TRACE_SEEDS seeds of each case of the row it borrows them from."""
    src, seeds = (TRACE_ROWS[row][1], TRACE_SEEDS) if row in TRACE_ROWS else (row, SEEDS)
    out = set()
    for name, cs, *_ in cases(src):
        out |= polled(src, name, cs, seeds)
    return out


def check_variant(row, w, lim, emu=None):
    """The case runs on exactly the build its row names: the host library's selection, which is the device run's; the host-compiled kernel
    selects with the same select_variant over the same make_geometry and is held to the row's lane stride, spill region, state placement and
    entry width (the row it really runs on is asserted where it runs: run_row)."""
    from madsim_amd import runtime
    r = ROWS[row]
    g = runtime.geometry(w, lim)
    assert runtime.variant_name(g) == r.variant, (row, runtime.variant_name(g), r.variant)
    if emu is not None:
        e, p = emu.geometry(w, lim), emu.geometry_params(w, lim)
        assert e.lanes_per_wave == g.lanes_per_wave and (p["heap_spill"] > 0) == (g.heap_spill_slots > 0) == bool(r.sel[1]), (row, e.lanes_per_wave, p)
        assert bool(p["gstate_mode"]) == bool(r.sel[5]) and bool(p["narrow"]) == bool(r.feat & NARROW), (row, p)
        assert p["features"] & ALL & ~r.feat == 0 and feature_tier(p["features"]) == feature_tier(r.feat), (row, p["features"])
    return g


def run_row(row, run, check=None, ran_on=None):
    """Every case of a row: `run(w, seed0, count, cfg, lim)` -> results, compared with the truth on all 48 bytes; no seed of the pass may be
    a runner verdict.  `check(row, w, lim)` asserts the selection before the run, `ran_on()` names the build the run really used after it.
    -> the number of cases."""
    n = 0
    for name, cs, w, cfg, lim in cases(row):
        what = (row, name, cs)
        if check is not None:
            check(row, w, lim)
        want = truth(row, name, cs)
        got = run(w, SEED0, SEEDS, cfg, lim)
        if ran_on is not None:
            assert ran_on() == ROWS[row].sel, (what, ran_on(), ROWS[row].sel)
        assert not (got["verdict"] >= A.OVERFLOW).any(), (what, "runner verdicts in the first pass", np.unique(got["verdict"], return_counts=True))
        bad = got != want
        assert not bad.any(), (what, f"{int(bad.sum())} of {SEEDS} seeds differ", int(np.nonzero(bad)[0][0]) + SEED0, got[bad][0], want[bad][0])
        n += 1
    return n


def count_differing(row, run):
    """(name, carriers, seeds that differ from the truth) per case of a row, nothing asserted: what tools/build_mutants.py tabulates."""
    for name, cs, w, cfg, lim in cases(row):
        yield name, cs, int((run(w, SEED0, SEEDS, cfg, lim) != truth(row, name, cs)).sum())


# ---- the trace rows: raw determinism and observation logs, byte for byte ---------------------------------------------------------------------
_TRACE_TRUTH = {}


def trace_truth(row):
    """[(name, carriers, workload, config, limits, [(seed, log bytes, observations, result tuple)])] of a trace row — the cases of the
    LDS-resident row of its tier, TRACE_SEEDS seeds each —, from the oracle."""
    if row not in _TRACE_TRUTH:
        out = []
        for name, cs, w, cfg, lim in cases(TRACE_ROWS[row][1]):
            seeds = []
            for s in range(SEED0, SEED0 + TRACE_SEEDS):
                log, res = oracle.trace_seed(w, s, cfg, lim)
                obs, res2 = oracle.observe_seed(w, s, cfg, lim)
                assert res.astuple() == res2.astuple() and res.verdict < A.OVERFLOW, (row, name, s)
                seeds.append((s, log, obs, res.astuple()))
            out.append((name, cs, w, cfg, lim, seeds))
        _TRACE_TRUTH[row] = out
    return _TRACE_TRUTH[row]
