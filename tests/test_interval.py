"""Interval tickers (MS_OP_INTERVAL / MS_OP_TICK / MS_OP_INTERVAL_RESET): time::interval — CPU side.

* the DSL and validate()'s static rules;
* the CPU reference (tests/interval_sim.py) on directed programs: each rule of madsim's Interval it restates;
* an independent yardstick: straight-line ticker programs equal, through the unchanged C oracle, their MARK + SLEEP_UNTIL rewrite;
* the host-compiled kernel (tests/emu) against IntervalSim on directed workloads, the ticker fuzzer and trace_seed logs;
* geometry: ticker workloads, and only they, select a ticker build.
"""
import random

import pytest

from madsim_amd import _abi as A
from madsim_amd import runtime
from madsim_amd import workload as W
from tests import fuzz_interval, parity
from tests import interval_sim as I
from tests.test_timeout_scope import FIELDS, resolved_emu

MS = 1_000_000


def _one_task(build, cfg=None):
    """One ticking task on its own node (body `build(t)`), spawned and joined by main."""
    wl = W.WorkloadBuilder()
    n = wl.create_node()
    t = wl.task(n)
    build(t)
    t.done()
    m = wl.main()
    m.spawn(t); m.join(t); m.done()
    return wl.build(), cfg or A.Config.default()


def _paused(behavior, pause_us, period_ms=10, ticks=8, fold=True):
    """A ticker whose node is paused for pause_us after its second tick: the overdue ticks come due together on resume."""
    wl = W.WorkloadBuilder()
    n = wl.create_node()
    t = wl.task(n)
    t.interval(ms=period_ms, behavior=behavior)
    t.set(0, ticks)
    top = t.label()
    t.tick(trace=fold); t.trace_instant(); t.djnz(0, top); t.done()
    m = wl.main()
    m.spawn(t); m.sleep(us=period_ms * 1000 + 1500); m.pause(n); m.sleep(us=pause_us); m.resume(n); m.join(t); m.done()
    return wl.build(), A.Config.default()


def _sim(w, cfg, seed=0):
    s = I.IntervalSim(w, cfg, seed)
    s.result = s.run()
    return s


def directed():
    out = {}
    out["first_tick"] = _one_task(lambda t: (t.interval(ms=10), t.tick(trace=True), t.trace_instant(), t.tick(trace=True), t.trace_instant()))
    out["under_floor"] = _one_task(lambda t: (t.interval(us=300), t.set(0, 6), t.tick(trace=True), t.trace_instant(), t.sleep(us=500), t.djnz(0, 2)))
    out["overrun"] = _one_task(lambda t: (t.interval(ms=4), t.set(0, 5), t.tick(trace=True), t.sleep(ms=13), t.trace_instant(), t.djnz(0, 2)))
    out["overrun_delay"] = _one_task(lambda t: (t.interval(ms=4, behavior="delay"), t.set(0, 5), t.tick(trace=True), t.sleep(ms=13), t.djnz(0, 2)))
    out["overrun_skip"] = _one_task(lambda t: (t.interval(ms=4, behavior="skip"), t.set(0, 5), t.tick(trace=True), t.sleep(ms=13), t.djnz(0, 2)))
    out["reset"] = _one_task(lambda t: (t.interval(ms=10), t.tick(trace=True), t.sleep(ms=3), t.interval_reset(), t.tick(trace=True), t.trace_instant()))
    out["interval_at"] = _one_task(lambda t: (t.mark(), t.sleep(ms=7), t.interval(ms=5, at_mark=True), t.set(0, 4), t.tick(trace=True),
                                              t.trace_instant(), t.djnz(0, 4)))
    out["secs_period"] = _one_task(lambda t: (t.interval(secs=2, ms=5, behavior="skip"), t.set(0, 3), t.tick(trace=True), t.sleep(secs=3), t.djnz(0, 2)))

    def scoped(t):      # timeout(2 ms, ticker.tick()) on a 10 ms ticker: expiries leave stale timers, which wake the task spuriously
        t.interval(ms=10); t.set(0, 6)
        top = t.label()
        with t.timeout(ms=2):
            t.tick(trace=True)
        t.trace_val(); t.sleep(ms=1); t.djnz(0, top)
    out["scoped_tick"] = _one_task(scoped)
    for b in ("burst", "delay", "skip"):
        out["paused_" + b] = _paused(b, 47000)
    out["raft_ticker"] = (W.raft_ticker(), A.Config.default())
    out["raft_ticker_skip"] = (W.raft_ticker(behavior="skip", pauses=2), A.Config.default())
    out["lease_keeper"] = (W.lease_keeper(), A.Config.default())
    return out


DIRECTED = directed()


# ---- DSL and validate() -----------------------------------------------------------------------------------------------------------
def test_dsl_encodes_the_three_ops():
    wl = W.WorkloadBuilder()
    n = wl.create_node()
    t = wl.task(n)
    t.mark(); t.interval(secs=3, ms=250, behavior="skip", at_mark=True); t.tick(trace=True); t.tick(); t.interval_reset(); t.done()
    w = wl.build()
    e = w.progs[1].entry
    ins = [(w.insns[i].op, w.insns[i].a, w.insns[i].b, w.insns[i].imm) for i in range(e, e + 5)]
    assert ins[1:] == [(A.OP["INTERVAL"], 2 | 4, 3, 250 * MS), (A.OP["TICK"], 1, 0, 0), (A.OP["TICK"], 0, 0, 0), (A.OP["INTERVAL_RESET"], 0, 0, 0)]
    g = runtime.geometry(w)
    assert g.variant & A.VARIANT_TICK and int(runtime.variant_name(g).split(", ")[3]) & 512
    with pytest.raises(ValueError):
        t.interval(ms=0)
    with pytest.raises(ValueError):
        t.interval(ms=1, behavior="catch-up")


def _refused(build, match):
    wl = W.WorkloadBuilder()
    n = wl.create_node()
    t = wl.task(n)
    build(wl, t)
    t.done()
    with pytest.raises(runtime.MadsimHipError, match=match):
        runtime.geometry(wl.build())


def test_validate_refuses_every_static_rule_violation():
    _refused(lambda wl, t: (t._emit("INTERVAL", a=0, b=0, imm=0), t.tick()), "period must be non-zero")
    _refused(lambda wl, t: (t._emit("INTERVAL", a=3, b=0, imm=MS), t.tick()), "missed-tick behaviour")
    _refused(lambda wl, t: (t._emit("INTERVAL", a=0, b=1, imm=10**9), t.tick()), "nanoseconds below one second")
    _refused(lambda wl, t: (t.interval(ms=5, at_mark=True), t.tick()), "interval_at before the program's first mark")
    _refused(lambda wl, t: t.tick(), "passes no interval")
    _refused(lambda wl, t: t.interval_reset(), "passes no interval")

    def branch_around(wl, t):       # one path reaches the tick without the interval
        t.jeq(0, t.label() + 2); t.interval(ms=5); t.tick()
    _refused(branch_around, "passes no interval")

    def loop_back(wl, t):           # the loop's back edge is fine, the entry path is not
        top = t.label(); t.set(0, 2); t.tick(); t.interval(ms=5); t.djnz(0, top)
    _refused(loop_back, "passes no interval")

    def child(wl, t):               # a spawned program does not inherit its parent's ticker
        c = wl.task(t.node); c.tick(); c.done()
        t.interval(ms=5); t.spawn(c); t.tick()
    _refused(child, "passes no interval")

    def in_scope(wl, t):
        with t.timeout(ms=5):
            t.interval(ms=1)
        t.tick()
    _refused(in_scope, "interval inside a timeout scope")

    def ok(wl, t):                  # loops, jumps, a scope around the tick, a replaced ticker, reset
        t.mark(); t.interval(ms=5, at_mark=True); t.set(0, 3)
        top = t.label()
        with t.timeout(ms=2) as s:
            t.tick(); t.interval_reset(); t.jmp(s.end)
        t.jeq(A.VAL_TIMEOUT, top); t.interval(us=700, behavior="delay"); t.djnz(0, top)
    wl = W.WorkloadBuilder(); n = wl.create_node(); t = wl.task(n); ok(wl, t); t.done()
    runtime.geometry(wl.build())


# ---- reference facts on IntervalSim -------------------------------------------------------------------------------------------------
def test_first_tick_lands_one_ms_after_creation_and_returns_its_deadline():
    w, cfg = DIRECTED["first_tick"]
    s = _sim(w, cfg)
    created = s.tick_instants[0] - MS
    assert s.tick_instants == [created + MS, created + MS + 10 * MS]
    assert s.obs_list[0] == s.tick_instants[0] and s.obs_list[1] > s.tick_instants[0]      # the instant folded is the scheduled one, not `now`
    assert s.obs_list[2] == s.tick_instants[1] and s.obs_list[3] - s.tick_instants[1] >= 50
    assert s.ticks_immediate == 0 and s.tick_spurious == 0


def test_a_passed_deadline_completes_without_yielding():
    w, cfg = DIRECTED["overrun"]                  # a 13 ms body on a 4 ms ticker: every later tick is already due
    s = _sim(w, cfg)
    assert s.ticks_done == 5 and s.ticks_immediate == 4
    # no yield: the instant traced right behind an immediate tick is the instant the body's sleep ended at (no ready-queue draw between)
    w2, _ = _one_task(lambda t: (t.interval(ms=4), t.tick(), t.sleep(ms=13), t.trace_instant(), t.tick(), t.trace_instant()))
    s2 = _sim(w2, cfg)
    assert s2.ticks_immediate == 1 and s2.obs_list[0] == s2.obs_list[1]
    w3, _ = _one_task(lambda t: (t.interval(ms=4), t.tick(), t.sleep(ms=13), t.trace_instant(), t.yield_now(), t.trace_instant()))
    s3 = _sim(w3, cfg)
    assert s3.obs_list[1] > s3.obs_list[0] and s3.result["rng_calls"] > s2.result["rng_calls"]   # a yield: a ready-queue draw, time moves


@pytest.mark.parametrize("k", [2, 3, 4, 6])
def test_burst_gives_k_immediate_ticks_after_a_pause_of_k_periods(k):
    # paused at 11.5 ms, parked on the tick due at 21 ms; resumed at 12 ms + k periods: the deadlines 21 .. 11 + 10 k ms are overdue —
    # the parked tick completes on its wake, the k - 1 behind it at once, without a timer
    w, cfg = _paused("burst", 10_000 * k + 500, ticks=3 + k + 2)
    s = _sim(w, cfg)
    assert s.ticks_immediate == k - 1 and s.ticks_late["burst"] >= k - 1
    d = s.tick_instants
    assert all(d[i + 1] - d[i] == 10 * MS for i in range(len(d) - 1))       # Burst keeps every deadline of the schedule
    for b in ("delay", "skip"):                                              # the other two pick a deadline ahead of now
        s2 = _sim(*_paused(b, 10_000 * k + 500, ticks=3 + k + 2))
        assert s2.ticks_immediate == 0 and s2.ticks_late[b] == 1


def test_lateness_of_exactly_5_ms_is_not_late_and_5_ms_1_ns_is():
    # advance() right behind the first tick, in the same poll: the second tick is polled exactly (first tick's lag) + adv - period late
    def run(adv):
        w, cfg = _one_task(lambda t: (t.interval(ms=10, behavior="delay"), t.tick(), t.advance(ns=adv), t.tick(), t.tick(trace=True)))
        return _sim(w, cfg)
    due1, now1 = run(MS).tick_log[0]
    on_time, late = run(15 * MS - (now1 - due1)), run(15 * MS - (now1 - due1) + 1)
    (d_on, n_on), (d_late, n_late) = on_time.tick_log[1], late.tick_log[1]
    assert n_on - d_on == 5 * MS and n_late - d_late == 5 * MS + 1
    assert on_time.ticks_late["delay"] == 0 and late.ticks_late["delay"] == 1
    assert on_time.tick_instants[2] == d_on + 10 * MS                      # not late: deadline + period
    assert late.tick_instants[2] == n_late + 10 * MS                        # late, Delay: now + period


def test_the_skip_formula():
    w, cfg = DIRECTED["overrun_skip"]
    s = _sim(w, cfg)
    assert s.ticks_late["skip"] >= 3
    d = s.tick_instants
    t0 = d[0]
    assert all((x - t0) % (4 * MS) == 0 for x in d)                         # Skip stays on the grid of the start
    assert all(d[i + 1] > d[i] + 4 * MS for i in range(1, len(d) - 1))      # ... and skips the missed ones
    wd, _ = DIRECTED["overrun_delay"]
    sd = _sim(wd, cfg)
    assert sd.ticks_late["delay"] >= 3 and any((x - sd.tick_instants[0]) % (4 * MS) for x in sd.tick_instants)


def test_reset_restarts_the_period_from_now():
    w, cfg = DIRECTED["reset"]
    s = _sim(w, cfg)
    assert s.tick_instants[1] - s.tick_instants[0] > 13 * MS                # 3 ms of sleep (+ floor and 50 ns) + a full period


def test_scoped_ticks_leave_stale_timers_that_wake_the_task():
    w, cfg = DIRECTED["scoped_tick"]
    s = _sim(w, cfg)
    assert A.VAL_TIMEOUT in s.obs_list and s.tick_spurious > 0 and s.ticks_done > 0


def test_directed_workloads_reach_what_they_are_named_for():
    s = {n: _sim(*DIRECTED[n]) for n in ("under_floor", "interval_at", "secs_period", "raft_ticker", "lease_keeper")}
    assert s["under_floor"].ticks_immediate > 0                             # a 300 us period under the 1 ms floor of the body's polls
    ia = s["interval_at"]                                                   # start 7 ms in the past: the 1 ms floor still applies
    assert ia.ticks_done == 4 and ia.ticks_immediate == 0 and ia.tick_log[0][0] - ia.obs_list[0] < 2 * MS
    assert s["secs_period"].ticks_late["skip"] >= 1
    assert sum(_sim(*DIRECTED["raft_ticker"], seed=k).ticks_late["burst"] for k in range(4)) > 0
    assert s["lease_keeper"].ticks_late["skip"] > 0 and A.VAL_TIMEOUT in s["lease_keeper"].obs_list


# ---- the oracle yardstick ---------------------------------------------------------------------------------------------------------
def straight_line(rng):
    """Straight-line ticker programs whose bodies end at least 1 ms before the next deadline (the first tick 1 ms after the
    interval; a body of sleeps, sends, traces and yields well inside period - 2 ms)."""
    wl = W.WorkloadBuilder()
    ns = wl.create_node()
    srv = wl.addr(ns, 9)
    r = wl.task(ns, init=True, pre=True)
    r.bind(srv)
    top = r.label()
    r.recv_from(srv, 1); r.trace_val(); r.jmp(top)
    ts = []
    for i in range(rng.randint(1, 3)):
        nc = wl.create_node()
        a = wl.addr(nc, 1)
        t = wl.task(nc)
        t.bind(a); t.sleep(us=rng.randint(1, 4000))
        period_ms = rng.choice([8, 10, 25, 1000, 2100])
        t.interval(ms=period_ms, behavior=rng.choice(["burst", "delay", "skip"]))
        for k in range(rng.randint(2, 6)):
            t.tick()
            budget = (period_ms - 3) * 1000            # us; each await below costs at most its duration (>= 1 ms floor) + a few us
            for _ in range(rng.randint(0, 3)):
                op = rng.choice(["sleep", "send", "trace", "yield", "instant"])
                if op == "sleep" and budget > 2100:
                    d = rng.randint(1, min(budget - 1100, 6000)); t.sleep(us=d); budget -= max(d, 1000) + 100
                elif op == "send" and budget > 1200:
                    t.send_to(a, srv, 1, k); budget -= 1100
                elif op == "trace":
                    t.trace(k)
                elif op == "yield":
                    t.yield_now(); budget -= 10
                else:
                    t.trace_instant()
        ts.append(t)
    m = wl.main()
    for t in ts:
        m.spawn(t)
    for t in ts:
        m.join(t)
    m.done()
    return wl.build(), A.Config.default(packet_loss_rate=rng.choice([0.0, 0.2]))


def straight_line_programs(n, base=4200):
    return [(base + k,) + straight_line(random.Random(base + k)) for k in range(n)]


def test_reference_on_straight_line_programs_equals_the_oracle_on_their_rewrite():
    for k, w, cfg in straight_line_programs(24):
        w2 = I.rewrite_ticks_as_sleep_until(w)
        lim = A.Limits()
        want = parity.expected(w2, 0, 4, cfg, lim)
        for s in range(4):
            sim = I.IntervalSim(w, cfg, s)
            got = sim.run()
            assert sim.ticks_immediate == 0 and sum(sim.ticks_late.values()) == 0 and sim.ticks_done > 0, (k, s)
            assert {f: got[f] for f in FIELDS} == {f: int(want[s][f]) for f in FIELDS}, (k, s)


@pytest.mark.parametrize("state_mem", [A.STATE_LDS, A.STATE_GLOBAL])
def test_emu_straight_line_programs_equal_the_parity_expectation_of_the_rewrite(state_mem):
    from tests import emu
    for k, w, cfg in straight_line_programs(10, base=5100):
        lim = fuzz_interval.interval_limits(state_mem)
        assert emu.geometry_params(w, lim)["features"] & 512
        w2 = I.rewrite_ticks_as_sleep_until(w)
        got = emu.run_batch(w, 0, 6, cfg, lim)
        want = parity.expected(w2, 0, 6, cfg, lim)
        parity.compare(got, want, lambda: parity.resolve_seed_by_seed(emu.run_batch, w, 0, got, cfg, lim), f"straight/{k}", None, k,
                       lambda i: parity.beyond_ceiling(w2, i, cfg, lim))


# ---- emulator parity --------------------------------------------------------------------------------------------------------------
def assert_equals_interval_sim(got, w, cfg, seed0, label):
    for i in range(len(got)):
        want = I.IntervalSim(w, cfg, seed0 + i).run()
        assert {f: int(got[i][f]) for f in FIELDS} == {f: want[f] for f in FIELDS}, (label, seed0 + i)


@pytest.mark.parametrize("name", sorted(DIRECTED))
def test_emu_directed_interval_workloads_equal_interval_sim(name):
    w, cfg = DIRECTED[name]
    for sm in (A.STATE_LDS, A.STATE_GLOBAL):
        got = resolved_emu(w, 0, 4, cfg, fuzz_interval.interval_limits(sm))
        assert_equals_interval_sim(got, w, cfg, 0, (name, sm))


@pytest.mark.parametrize("block", ["fixed", "clock"])
def test_emu_interval_fuzz_equals_interval_sim(block):
    import time
    base = 300 if block == "fixed" else int(time.time()) % 1_000_000 * 100
    for k in range(16):
        w, cfg, _ = fuzz_interval.random_interval_workload(random.Random(base + k))
        got = resolved_emu(w, 0, 4, cfg, fuzz_interval.interval_limits(A.STATE_GLOBAL if k % 2 else A.STATE_LDS))
        assert_equals_interval_sim(got, w, cfg, 0, f"random_interval_workload(Random({base + k}))")


def test_emu_trace_seed_log_equals_interval_sim():
    from tests import emu
    for name in ("raft_ticker", "lease_keeper", "scoped_tick", "paused_skip"):
        w, cfg = DIRECTED[name]
        lim = fuzz_interval.interval_limits()
        log, res = emu.trace_seed(w, 3, cfg, lim)
        while res["verdict"] == A.OVERFLOW:
            lim = parity.grow(lim, w.struct.n_progs)
            log, res = emu.trace_seed(w, 3, cfg, lim)
        want = I.IntervalSim(w, cfg, 3).run()
        assert log.hex() == want["log"] and {f: int(res[f]) for f in FIELDS} == {f: want[f] for f in FIELDS}, name


# ---- geometry ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("state_mem", [0, A.STATE_LDS, A.STATE_GLOBAL, A.STATE_GLOBAL | A.STATE_NARROW_HEAP | A.STATE_DEDUP_TIMERS])
def test_ticker_workloads_and_only_they_select_a_ticker_build(state_mem):
    cases = [W.raft_ticker(), W.lease_keeper()] + [fuzz_interval.random_interval_workload(random.Random(60 + k))[0] for k in range(6)]
    for w in cases:
        lim = fuzz_interval.interval_limits(state_mem)
        g = runtime.geometry(w, lim)
        assert g.variant & A.VARIANT_TICK and g.variant & A.VARIANT_SCOPE and "799" in runtime.variant_name(g) or "783" in runtime.variant_name(g)
    for w in (W.raft_election(), W.tonic_unary(), W.kv_rpc(), W.streaming_topology(), W.pingpong()):
        assert not runtime.geometry(w, A.Limits()).variant & A.VARIANT_TICK
