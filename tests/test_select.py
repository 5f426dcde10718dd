"""select_biased! over a receive and a tick (MS_OP_RECV_OR_TICK) and timeout_at (MS_OP_RECV_TIMEOUT_AT), ABI v7 — CPU side.

* the DSL encoding and validate()'s refusals, one per rule;
* the CPU reference (tests/select_sim.py) on directed programs: each rule it restates;
* two yardsticks through the unchanged C oracle, on the host-compiled kernel (tests/emu): MARK; RECV_TIMEOUT_AT d equals MARK;
  RECV_TIMEOUT d, and INTERVAL p; RECV_OR_TICK (recv first, no fold) equals MARK; RECV_TIMEOUT 1 ms;
* the host-compiled kernel against SelectSim on directed workloads, the select fuzzer and trace_seed logs, in both layouts;
* geometry: either op, and only they, route the workload to a select build (the ticker builds stay as they were).
"""
import random

import pytest

from madsim_amd import _abi as A
from madsim_amd import runtime
from madsim_amd import workload as W
from tests import fuzz_select, parity
from tests import select_sim as S
from tests.test_timeout_scope import FIELDS, resolved_emu

MS = 1_000_000
T = 5


def _pair(build_rx, build_tx=None, cfg=None):
    """A receiver on its own node (body `build_rx(t, a_rx)`) and an optional sender (`build_tx(s, a_tx, a_rx)`), joined by main.
    Both bodies start at pc 1 of their program (pc 0 is the bind): their jump targets count from there."""
    wl = W.WorkloadBuilder()
    nr, nt = wl.create_node(), wl.create_node()
    a_rx, a_tx = wl.addr(nr, 1), wl.addr(nt, 1)
    r = wl.task(nr)
    r.bind(a_rx)
    build_rx(r, a_rx)
    r.done()
    m = wl.main()
    m.spawn(r)
    if build_tx:
        s = wl.task(nt)
        s.bind(a_tx)
        build_tx(s, a_tx, a_rx)
        s.done()
        m.spawn(s); m.join(s)
    m.join(r); m.done()
    return wl.build(), cfg or A.Config.default()


def _sim(w, cfg, seed=0):
    s = S.SelectSim(w, cfg, seed)
    s.result = s.run()
    return s


def directed():
    out = {}
    # tick first, due at the select's first poll (a 10 ms body on a 2 ms ticker): wins without registering, drawing or yielding
    out["tick_first_due"] = _pair(lambda t, a: (t.interval(ms=2), t.set(0, 4), t.sleep(ms=10), t.recv_or_tick(a, T, tick_first=True, trace=True),
                                                t.trace_instant(), t.trace_val(), t.djnz(0, 3)))
    # recv first, tick due, a message queued: taken, its rand_delay drawn, lost to the tick
    out["lost"] = (W.lossy_select(), A.Config.default())
    # recv first on a 20 ms ticker, messages every ~3 ms: the recv arm wins and the pending tick's timers go stale
    out["stale_wake"] = _pair(lambda t, a: (t.interval(ms=20), t.set(0, 8), t.recv_or_tick(a, T), t.trace_val(), t.trace_instant(), t.djnz(0, 3)),
                              lambda s, a, d: (s.set(0, 6), s.sleep(ms=3), s.send_to(a, d, T, 0x33), s.djnz(0, 2)))
    # tick first, nothing due, a sender: both arms win sometimes
    out["tick_first_mixed"] = _pair(lambda t, a: (t.interval(ms=4, behavior="delay"), t.set(0, 10), t.recv_or_tick(a, T, tick_first=True, trace=True),
                                                  t.trace_val(), t.djnz(0, 3)),
                                    lambda s, a, d: (s.set(0, 8), s.sleep_rand(lo_ms=0, ms=9), s.send_to(a, d, T, 0x44), s.djnz(0, 2)))
    # timeout_at: the deadline from the mark, 1 ms floor when it has passed; a message does not move it
    out["timeout_at_floor"] = _pair(lambda t, a: (t.mark(), t.sleep(ms=5), t.recv_from_timeout_at(a, T, ms=2), t.trace_val(), t.trace_instant()))
    out["timeout_at_fixed"] = _pair(lambda t, a: (t.mark(), t.set(0, 6), t.recv_from_timeout_at(a, T, ms=12), t.trace_val(), t.trace_instant(),
                                                  t.djnz(0, 3)),
                                    lambda s, a, d: (s.set(0, 4), s.sleep(ms=2), s.send_to(a, d, T, 0x55), s.djnz(0, 2)))
    out["raft_select"] = (W.raft_select(), A.Config.default())
    out["raft_select_skip"] = (W.raft_select(behavior="skip", pauses=2), A.Config.default())
    return out


DIRECTED = directed()
LIMITS = {"lost": W.lossy_select_limits, "raft_select": W.raft_select_limits, "raft_select_skip": W.raft_select_limits}


def limits_for(name, state_mem):
    lim = LIMITS[name]() if name in LIMITS else fuzz_select.select_limits()
    lim.state_mem = state_mem
    return lim


# ---- DSL and validate() -----------------------------------------------------------------------------------------------------------
def test_dsl_encodes_the_two_ops():
    wl = W.WorkloadBuilder()
    n = wl.create_node()
    a = wl.addr(n, 1)
    t = wl.task(n)
    t.mark(); t.interval(ms=5); t.recv_or_tick(a, 0x23); t.recv_or_tick(a, 0x81, tick_first=True, trace=True)
    t.recv_from_timeout_at(a, 7, secs=2, ms=250); t.done()
    w = wl.build()
    e = w.progs[1].entry
    ins = [(w.insns[i].op, w.insns[i].a, w.insns[i].b, w.insns[i].imm) for i in range(e + 2, e + 5)]
    assert ins == [(A.OP["RECV_OR_TICK"], a, 0x2300, 0), (A.OP["RECV_OR_TICK"], a, 0x8103, 0), (A.OP["RECV_TIMEOUT_AT"], a, 0x0702, 250 * MS)]
    assert A.OP["RECV_OR_TICK"] == 65 and A.OP["RECV_TIMEOUT_AT"] == 66 and A.ABI_VERSION == 7
    g = runtime.geometry(w)
    assert g.variant & A.VARIANT_TICK
    with pytest.raises(ValueError):
        t.recv_from_timeout_at(a, 7, secs=256)


@pytest.mark.parametrize("state_mem", [A.STATE_LDS, A.STATE_GLOBAL])
def test_either_op_and_only_they_select_a_select_build(state_mem):
    w, _ = DIRECTED["timeout_at_fixed"]                  # timeout_at without a ticker: a select build without the tick unit
    assert A.OP["INTERVAL"] not in [w.insns[i].op for i in range(w.struct.n_insns)]
    sel = A.VARIANT_TICK | A.VARIANT_SELECT
    for name in ("timeout_at_fixed", "raft_select", "lost", "tick_first_due"):
        g = runtime.geometry(DIRECTED[name][0], limits_for(name, state_mem))
        assert g.variant & sel == sel and int(runtime.variant_name(g).split(", ")[3]) & 1024, name
    # the ticker workloads stay on the ticker builds, the others on theirs
    g = runtime.geometry(W.raft_ticker(), W.raft_ticker_limits())
    assert g.variant & A.VARIANT_TICK and not g.variant & A.VARIANT_SELECT
    g = runtime.geometry(W.lease_keeper(), W.lease_keeper_limits())
    assert g.variant & A.VARIANT_TICK and not g.variant & A.VARIANT_SELECT
    for w2 in (W.pingpong(), W.raft_election(), W.tonic_unary()):
        assert not runtime.geometry(w2, A.Limits()).variant & sel


def _refused(build, match):
    wl = W.WorkloadBuilder()
    n = wl.create_node()
    a = wl.addr(n, 1)
    t = wl.task(n)
    build(wl, t, a)
    t.done()
    with pytest.raises(runtime.MadsimHipError, match=match):
        runtime.geometry(wl.build())


def test_validate_refuses_every_rule_violation():
    # inside a timeout scope, as RECV_TIMEOUT is refused there
    def scoped_select(wl, t, a):
        t.interval(ms=5)
        with t.timeout(ms=5):
            t.recv_or_tick(a, T)
    _refused(scoped_select, "op not allowed inside a timeout scope")

    def scoped_at(wl, t, a):
        t.mark()
        with t.timeout(ms=5):
            t.recv_from_timeout_at(a, T, ms=1)
    _refused(scoped_at, "op not allowed inside a timeout scope")
    # RECV_OR_TICK on a path that passes no interval
    _refused(lambda wl, t, a: t.recv_or_tick(a, T), "passes no interval")

    def branch_around(wl, t, a):
        t.jeq(0, t.label() + 2); t.interval(ms=5); t.recv_or_tick(a, T)
    _refused(branch_around, "passes no interval")

    def child(wl, t, a):
        c = wl.task(t.node); c.recv_or_tick(a, T); c.done()
        t.interval(ms=5); t.spawn(c)
    _refused(child, "passes no interval")
    # RECV_TIMEOUT_AT without a MARK at a lower pc
    _refused(lambda wl, t, a: (t.recv_from_timeout_at(a, T, ms=3), t.mark()), "recv_from_timeout_at before the program's first mark")
    # unknown flag bits, ns >= 10^9
    _refused(lambda wl, t, a: (t.interval(ms=5), t._emit("RECV_OR_TICK", a=a, b=(T << 8) | 4)), "b bits 0-1 are the flags")
    _refused(lambda wl, t, a: (t.mark(), t._emit("RECV_TIMEOUT_AT", a=a, b=T << 8, imm=10**9)), "nanoseconds below one second")
    # RECV_TIMEOUT's tag and socket rules
    _refused(lambda wl, t, a: (t.interval(ms=5), t.recv_or_tick(a, 0xFE)), "reserved")
    _refused(lambda wl, t, a: (t.mark(), t.recv_from_timeout_at(a, 0xFF, ms=1)), "reserved")
    _refused(lambda wl, t, a: (t.interval(ms=5), t._emit("RECV_OR_TICK", a=9, b=T << 8)), "socket operand out of range")

    def ok(wl, t, a):                 # a loop back over the select, a replaced ticker, timeout_at after the mark
        t.mark(); t.interval(ms=5); t.set(0, 3)
        top = t.label()
        t.recv_or_tick(a, T, tick_first=True); t.recv_from_timeout_at(a, T, ms=4); t.interval(ms=2); t.djnz(0, top)
    wl = W.WorkloadBuilder(); n = wl.create_node(); a = wl.addr(n, 1); t = wl.task(n); ok(wl, t, a); t.done()
    runtime.geometry(wl.build())


# ---- reference facts on SelectSim ---------------------------------------------------------------------------------------------------
def test_a_due_tick_first_wins_at_once_without_registration_draw_or_yield():
    w, cfg = DIRECTED["tick_first_due"]
    s = _sim(w, cfg)
    assert s.won == {"recv": 0, "tick": 4, "deadline": 0} and s.tick_immediate == 4
    assert all(not sock["regs"] for sock in s.bound.values() if sock)                      # never polled: no registration
    # the instant traced right behind the select is the one the body's sleep ended at: no yield, and no rand_delay draw
    w2, _ = _pair(lambda t, a: (t.interval(ms=2), t.sleep(ms=10), t.trace_instant(), t.recv_or_tick(a, T, tick_first=True), t.trace_instant()))
    s2 = _sim(w2, cfg)
    w3, _ = _pair(lambda t, a: (t.interval(ms=2), t.sleep(ms=10), t.trace_instant(), t.trace_instant()))
    s3 = _sim(w3, cfg)
    assert s2.obs_list[0] == s2.obs_list[1] and s2.result["rng_calls"] == s3.result["rng_calls"]
    assert A.VAL_TIMEOUT in s.obs_list


def test_a_recv_first_select_loses_the_message_it_took():
    w, cfg = DIRECTED["lost"]
    s = _sim(w, cfg)
    assert s.lost > 0 and s.won["tick"] == 16 and s.won["recv"] == 0
    assert s.result["verdict"] == A.PASS and 0x51 not in s.obs_list                          # every message sent, none received
    # the draw happened: the recv arms drew (their rand_delay, at least one GlobalRng call per message taken) — and with the tick arm first,
    # the same sends on the same ticker, nothing is taken and the recv arms draw nothing
    assert s.recv_arm_draws >= s.lost
    t = _sim(W.lossy_select(tick_first=True), cfg)
    assert t.lost == 0 and t.recv_arm_draws == 0 and t.won["tick"] == 16


def test_a_dropped_pending_tick_leaves_timers_that_wake_the_task_for_nothing():
    w, cfg = DIRECTED["stale_wake"]
    s = _sim(w, cfg)
    assert s.won["recv"] > 0 and s.stale_wakes > 0


def test_timeout_at_takes_its_deadline_from_the_mark_with_the_1_ms_floor():
    w, cfg = DIRECTED["timeout_at_floor"]
    s = _sim(w, cfg)
    assert s.won["deadline"] == 1 and s.obs_list[0] == A.VAL_TIMEOUT
    w2, _ = _pair(lambda t, a: (t.mark(), t.sleep(ms=5), t.trace_instant()))
    woke = _sim(w2, cfg).obs_list[0]                                                          # the instant the sleep ended
    assert 1 * MS <= s.obs_list[1] - woke <= 1 * MS + 100                                     # max(t0 + 2 ms, now + 1 ms) = now + 1 ms
    f = _sim(*DIRECTED["timeout_at_fixed"])
    assert f.won["recv"] > 0 and f.won["deadline"] > 0                                        # messages do not move the deadline


def test_directed_workloads_reach_what_they_are_named_for():
    s = _sim(*DIRECTED["tick_first_mixed"])
    assert s.won["recv"] > 0 and s.won["tick"] > 0
    r = [_sim(*DIRECTED["raft_select"], seed=k) for k in range(4)]
    assert all(x.result["verdict"] == A.PASS for x in r) and sum(x.won["tick"] for x in r) > 0 and sum(x.won["deadline"] for x in r) > 0


# ---- the oracle yardsticks -----------------------------------------------------------------------------------------------------------
def _echo_programs(rng, body):
    """Clients that loop `send to the echo server; body(client, a)` against a server that answers after a random service time."""
    wl = W.WorkloadBuilder()
    ns = wl.create_node()
    srv = wl.addr(ns, 9)
    r = wl.task(ns, init=True, pre=True)
    r.bind(srv)
    top = r.label()
    r.recv_from(srv, 1); r.sleep_rand(lo_ms=0, us=rng.choice([800, 3000, 9000])); r.reply(srv, T, 0x77); r.jmp(top)
    cs = []
    for i in range(rng.randint(1, 3)):
        nc = wl.create_node()
        a = wl.addr(nc, 1)
        c = wl.task(nc)
        c.bind(a); c.set(0, rng.randint(2, 6))
        top = c.label()
        c.send_to(a, srv, 1, i)
        body(rng, c, a)
        c.trace_val(); c.djnz(0, top)
        cs.append(c)
    m = wl.main()
    for c in cs:
        m.spawn(c)
    for c in cs:
        m.join(c)
    m.done()
    return wl.build(), A.Config.default(packet_loss_rate=rng.choice([0.0, 0.2]))


def timeout_at_programs(n, base):
    def body(rng, c, a):
        c.mark(); c.recv_from_timeout_at(a, T, us=rng.choice([500, 1500, 4000, 12000]))
    return [(base + k,) + _echo_programs(random.Random(base + k), body) for k in range(n)]


def fresh_select_programs(n, base):
    def body(rng, c, a):
        c.interval(ms=rng.choice([1, 5, 50]), behavior=rng.choice(["burst", "delay", "skip"])); c.recv_or_tick(a, T)
    return [(base + k,) + _echo_programs(random.Random(base + k), body) for k in range(n)]


YARDSTICKS = [("timeout_at", timeout_at_programs, S.rewrite_timeout_at_as_timeout),
              ("fresh_select", fresh_select_programs, S.rewrite_fresh_select_as_timeout)]


@pytest.mark.parametrize("name,progs,rewrite", YARDSTICKS, ids=[y[0] for y in YARDSTICKS])
def test_reference_equals_the_oracle_on_the_rewrite(name, progs, rewrite):
    for k, w, cfg in progs(12, 7300):
        w2 = rewrite(w)
        want = parity.expected(w2, 0, 4, cfg, A.Limits())
        for s in range(4):
            got = S.SelectSim(w, cfg, s).run()
            assert {f: got[f] for f in FIELDS} == {f: int(want[s][f]) for f in FIELDS}, (name, k, s)


@pytest.mark.parametrize("state_mem", [A.STATE_LDS, A.STATE_GLOBAL])
@pytest.mark.parametrize("name,progs,rewrite", YARDSTICKS, ids=[y[0] for y in YARDSTICKS])
def test_emu_equals_the_parity_expectation_of_the_rewrite(name, progs, rewrite, state_mem):
    from tests import emu
    for k, w, cfg in progs(8, 7600):
        lim = fuzz_select.select_limits(state_mem)
        assert emu.geometry_params(w, lim)["features"] & 512
        w2 = rewrite(w)
        got = emu.run_batch(w, 0, 6, cfg, lim)
        want = parity.expected(w2, 0, 6, cfg, lim)
        parity.compare(got, want, lambda: parity.resolve_seed_by_seed(emu.run_batch, w, 0, got, cfg, lim), f"{name}/{k}", None, k,
                       lambda i: parity.beyond_ceiling(w2, i, cfg, lim))


# ---- emulator parity --------------------------------------------------------------------------------------------------------------
def assert_equals_select_sim(got, w, cfg, seed0, label):
    for i in range(len(got)):
        want = S.SelectSim(w, cfg, seed0 + i).run()
        assert {f: int(got[i][f]) for f in FIELDS} == {f: want[f] for f in FIELDS}, (label, seed0 + i)


@pytest.mark.parametrize("name", sorted(DIRECTED))
def test_emu_directed_select_workloads_equal_select_sim(name):
    w, cfg = DIRECTED[name]
    for sm in (A.STATE_LDS, A.STATE_GLOBAL):
        got = resolved_emu(w, 0, 4, cfg, limits_for(name, sm))
        assert_equals_select_sim(got, w, cfg, 0, (name, sm))


@pytest.mark.parametrize("block", ["fixed", "clock"])
def test_emu_select_fuzz_equals_select_sim(block):
    import time
    base = 500 if block == "fixed" else int(time.time()) % 1_000_000 * 100
    for k in range(16):
        w, cfg, _ = fuzz_select.random_select_workload(random.Random(base + k))
        got = resolved_emu(w, 0, 4, cfg, fuzz_select.select_limits(A.STATE_GLOBAL if k % 2 else A.STATE_LDS))
        assert_equals_select_sim(got, w, cfg, 0, f"random_select_workload(Random({base + k}))")


def test_select_fuzz_reaches_every_rule():
    tot = dict(recv=0, tick=0, deadline=0, lost=0, immediate=0, stale=0)
    for k in range(24):
        w, cfg, _ = fuzz_select.random_select_workload(random.Random(500 + k))
        s = _sim(w, cfg)
        tot["recv"] += s.won["recv"]; tot["tick"] += s.won["tick"]; tot["deadline"] += s.won["deadline"]
        tot["lost"] += s.lost; tot["immediate"] += s.tick_immediate; tot["stale"] += s.stale_wakes
    assert all(v > 0 for v in tot.values()), tot


def test_emu_trace_seed_log_equals_select_sim():
    from tests import emu
    for name in ("raft_select", "lost", "stale_wake", "tick_first_mixed"):
        w, cfg = DIRECTED[name]
        lim = limits_for(name, 0)
        log, res = emu.trace_seed(w, 3, cfg, lim)
        while res["verdict"] == A.OVERFLOW:
            lim = parity.grow(lim, w.struct.n_progs)
            log, res = emu.trace_seed(w, 3, cfg, lim)
        want = S.SelectSim(w, cfg, 3).run()
        assert log.hex() == want["log"] and {f: int(res[f]) for f in FIELDS} == {f: want[f] for f in FIELDS}, name
