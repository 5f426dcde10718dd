"""Ctrl-c signals (MS_OP_CTRL_C / MS_OP_SEND_CTRL_C / MS_OP_RECV_OR_CTRL_C) — CPU side.

* the DSL encoding and validate()'s refusals;
* the reference's own two tests, `ctrl_c_kill` and `ctrl_c_catch` (signal.rs:23-69), restated as workloads;
* the CPU reference (tests/signal_sim.py) on directed programs, one per rule it restates;
* an oracle yardstick: lifecycle workloads whose nodes install no handler, every KILL rewritten to SEND_CTRL_C, equal the parity
  expectation of the original (the unchanged C oracle) on all 48 bytes;
* the host-compiled kernel (tests/emu) against SignalSim on the directed workloads, the signal fuzzer and trace_seed logs, in both layouts;
* geometry: the three ops, and only they, route a workload to a signal build; the bench cases' layouts are what they were.
"""
import random

import pytest

from madsim_amd import _abi as A
from madsim_amd import runtime
from madsim_amd import workload as W
from tests import fuzz_signal, lifecycle_workloads as LW, parity
from tests import signal_sim as S
from tests.test_timeout_scope import FIELDS, resolved_emu

MS = 1_000_000
T = 5
FUZZ_UNSUPPORTED_CAP = 0.10        # at most this share of the fuzzer's seeds may end in rule 6's verdict


def _sim(w, cfg, seed=0):
    s = S.SignalSim(w, cfg, seed)
    s.result = s.run()
    return s


# ---- the reference's own tests (signal.rs:23-69) -------------------------------------------------------------------------------------
def ctrl_c_kill():
    wl = W.WorkloadBuilder()
    m = wl.main()
    n = wl.create_node()
    h = wl.task(n)
    h.sleep(secs=1000); h.done()                 # pending::<()>()
    m.spawn(h); m.assert_exit(n, False)
    m.send_ctrl_c(n)                              # ctrl-c will kill the node
    m.sleep(secs=1)
    m.join(h, expect_err=True); m.assert_exit(n, True)
    m.done()
    return wl.build()


def ctrl_c_catch():
    wl = W.WorkloadBuilder()
    m = wl.main()
    n = wl.create_node()
    h = wl.task(n)
    h.ctrl_c(); h.flag_store(0, 1); h.sleep(secs=1000); h.done()
    for _ in range(2):
        m.flag_store(0, 0)
        m.spawn(h)
        m.sleep(secs=1); m.assert_flag(0, 0)
        m.send_ctrl_c(n)                          # ctrl-c will be caught and not kill the node
        m.sleep(secs=1); m.assert_flag(0, 1); m.assert_exit(n, False)
    m.done()
    return wl.build()


# ---- directed workloads, one per rule ---------------------------------------------------------------------------------------------------
def _handler_node(wl, init=True):
    """A node whose (init) task awaits ctrl_c() in a loop and counts what it catches in flag 0."""
    n = wl.create_node()
    t = wl.task(n, init=init, pre=init)
    top = t.label()
    t.ctrl_c(); t.flag_add(0, 1); t.trace_instant(); t.jmp(top)
    return n, t


def install_then_restart():
    wl = W.WorkloadBuilder(); m = wl.main()
    n, _ = _handler_node(wl)
    m.sleep(ms=2); m.send_ctrl_c(n); m.sleep(ms=2); m.assert_flag(0, 1); m.assert_exit(n, False)     # installed: caught
    m.restart(n); m.send_ctrl_c(n); m.assert_exit(n, True)                                          # new NodeInfo, no handler yet: killed
    m.restart(n); m.sleep(ms=2); m.send_ctrl_c(n); m.sleep(ms=2); m.assert_flag(0, 2); m.assert_exit(n, False)
    m.done()
    return wl.build()


def handler_outlives_its_task():
    wl = W.WorkloadBuilder(); m = wl.main()
    n = wl.create_node()
    t = wl.task(n)
    t.ctrl_c(); t.flag_add(0, 1); t.done()         # the installing task ends; the handler stays
    m.spawn(t); m.sleep(ms=2); m.send_ctrl_c(n); m.join(t)
    m.send_ctrl_c(n); m.send_ctrl_c(n); m.assert_exit(n, False); m.assert_flag(0, 1)                # nobody waits: lost, and nothing is killed
    m.done()
    return wl.build()


def signal_to_killed_node():
    wl = W.WorkloadBuilder(); m = wl.main()
    n, _ = _handler_node(wl)
    m.sleep(ms=2); m.kill(n); m.send_ctrl_c(n); m.sleep(ms=2); m.send_ctrl_c(n)
    m.assert_exit(n, True); m.assert_flag(0, 0)
    m.done()
    return wl.build()


def signal_to_paused_node():
    wl = W.WorkloadBuilder(); m = wl.main()
    n, _ = _handler_node(wl)
    m.sleep(ms=2); m.pause(n); m.send_ctrl_c(n); m.sleep(ms=5); m.assert_flag(0, 0)                # the woken runnable is parked
    m.resume(n); m.sleep(ms=2); m.assert_flag(0, 1)
    m.done()
    return wl.build()


def signal_to_own_node():
    wl = W.WorkloadBuilder(); m = wl.main()
    n, _ = _handler_node(wl)
    s = wl.task(n)
    s.sleep(ms=2); s.send_ctrl_c(n); s.sleep(ms=2); s.assert_flag(0, 1); s.done()                  # a sibling catches it
    n2 = wl.create_node()
    k = wl.task(n2)
    k.sleep(ms=1); k.send_ctrl_c(n2); k.trace(0x99); k.sleep(ms=1); k.trace(0x9A); k.done()        # no handler: kills its own node, runs on to its next await
    m.spawn(s); m.spawn(k); m.join(s); m.join(k, expect_err=True); m.assert_exit(n2, True)
    m.done()
    return wl.build()


def select_pair(recv_first, gap_us, sends=6, signals=4):
    """A select loop, a client that sends at random intervals, and a supervisor that signals every `gap_us`."""
    wl = W.WorkloadBuilder(); m = wl.main()
    ns, nc = wl.create_node(), wl.create_node()
    a_s, a_c = wl.addr(ns, 1), wl.addr(nc, 1)
    srv = wl.task(ns)
    srv.bind(a_s)
    top = srv.label()
    srv.recv_or_ctrl_c(a_s, T, recv_first=recv_first); srv.trace_val(); srv.trace_instant(); srv.jmp(top)
    cl = wl.task(nc)
    cl.bind(a_c); cl.set(0, sends)
    top = cl.label()
    cl.sleep_rand(lo_ms=0, ms=4); cl.send_to(a_c, a_s, T, 0x51); cl.djnz(0, top); cl.done()
    m.spawn(srv); m.spawn(cl); m.sleep(ms=2)
    for _ in range(signals):
        m.send_ctrl_c(ns); m.sleep(us=gap_us)
    m.join(cl); m.done()
    return wl.build()


def paused_select(recv_first):
    """A select whose recv arm has taken a queued message (its rand_delay runs, 1 ms) on a node that is then paused: the delay's timer and a
    ctrl-c both reach the parked task, and the poll after the resume finds the message ready AND the signal.  Recv first: the message
    wins and the signal is lost.  Ctrl-c first: the signal wins and the message is lost."""
    wl = W.WorkloadBuilder(); m = wl.main()
    ns, nc = wl.create_node(), wl.create_node()
    a_s, a_c = wl.addr(ns, 1), wl.addr(nc, 1)
    srv = wl.task(ns)
    srv.bind(a_s); srv.sleep(ms=15)                                     # the message (sent at 2 ms, at most 10 ms on the wire) is queued by now
    srv.recv_or_ctrl_c(a_s, T, recv_first=recv_first); srv.trace_val(); srv.trace_instant(); srv.sleep(secs=1); srv.done()
    cl = wl.task(nc)
    cl.bind(a_c); cl.send_to(a_c, a_s, T, 0x51); cl.done()
    m.spawn(srv); m.spawn(cl)
    m.sleep(us=16500); m.pause(ns)                                      # the select began at 16 ms: its rand_delay ends at 17 ms
    m.sleep(ms=2); m.send_ctrl_c(ns); m.sleep(ms=1); m.resume(ns); m.sleep(ms=5)
    m.done()
    return wl.build()


def two_waiters():
    wl = W.WorkloadBuilder(); m = wl.main()
    n = wl.create_node()
    a, b = wl.task(n), wl.task(n)
    for t in (a, b):
        t.ctrl_c(); t.flag_add(0, 1); t.done()
    m.spawn(a); m.spawn(b); m.sleep(ms=2); m.send_ctrl_c(n); m.join(a); m.join(b)
    m.done()
    return wl.build()


def two_waiters_in_turn():
    """Two tasks of one node that wait one after the other — the second signals the first before it subscribes itself: never two
    parked at a send, exact."""
    wl = W.WorkloadBuilder(); m = wl.main()
    n = wl.create_node()
    a = wl.task(n)
    a.ctrl_c(); a.flag_add(0, 1); a.done()
    b = wl.task(n)
    b.sleep(ms=3); b.send_ctrl_c(n); b.ctrl_c(); b.flag_add(0, 1); b.done()    # b signals a, then waits itself
    m.spawn(a); m.spawn(b); m.join(a); m.sleep(ms=2); m.send_ctrl_c(n); m.join(b); m.assert_flag(0, 2)
    m.done()
    return wl.build()


def directed():
    d = A.Config.default()
    out = dict(ctrl_c_kill=ctrl_c_kill(), ctrl_c_catch=ctrl_c_catch(), install_then_restart=install_then_restart(),
               handler_outlives_its_task=handler_outlives_its_task(), signal_to_killed_node=signal_to_killed_node(),
               signal_to_paused_node=signal_to_paused_node(), signal_to_own_node=signal_to_own_node(),
               recv_first_loses_signal=paused_select(True), ctrl_c_first_loses_message=paused_select(False),
               select_loop_recv_first=select_pair(True, 1500, sends=10, signals=8),
               select_loop_ctrl_c_first=select_pair(False, 2500, sends=10, signals=6),
               two_waiters=two_waiters(), two_waiters_in_turn=two_waiters_in_turn(),
               graceful_shutdown=W.graceful_shutdown(), graceful_shutdown_recv_first=W.graceful_shutdown(recv_first=True, n_servers=2),
               shutdown_race=W.shutdown_race())
    return {k: (w, d) for k, w in out.items()}


DIRECTED = directed()
LIMITS = {"graceful_shutdown": W.graceful_shutdown_limits, "graceful_shutdown_recv_first": W.graceful_shutdown_limits,
          "shutdown_race": W.shutdown_race_limits}


def limits_for(name, state_mem):
    lim = LIMITS[name]() if name in LIMITS else fuzz_signal.signal_limits()
    lim.state_mem = state_mem
    return lim


# ---- DSL, ABI and validate() -------------------------------------------------------------------------------------------------------------
def test_dsl_encodes_the_three_ops_and_the_abi_stays_7():
    wl = W.WorkloadBuilder()
    n = wl.create_node()
    a = wl.addr(n, 1)
    t = wl.task(n)
    t.ctrl_c(); t.send_ctrl_c(n); t.recv_or_ctrl_c(a, 0x23); t.recv_or_ctrl_c(a, 0x81, recv_first=True); t.done()
    w = wl.build()
    e = w.progs[1].entry
    ins = [(w.insns[i].op, w.insns[i].a, w.insns[i].b, w.insns[i].imm) for i in range(e, e + 4)]
    assert ins == [(67, 0, 0, 0), (68, n, 0, 0), (69, a, 0x2300, 0), (69, a, 0x8101, 0)]
    assert (A.OP["CTRL_C"], A.OP["SEND_CTRL_C"], A.OP["RECV_OR_CTRL_C"]) == (67, 68, 69) and A.ABI_VERSION == 7
    assert A.VARIANT_SIGNAL == 1 << 23
    assert " kernels=43 " in runtime.lib().madsim_hip_build_info().decode()


@pytest.mark.parametrize("state_mem", [A.STATE_LDS, A.STATE_GLOBAL])
def test_the_three_ops_and_only_they_select_a_signal_build(state_mem):
    for name in ("ctrl_c_kill", "ctrl_c_catch", "graceful_shutdown", "shutdown_race", "recv_first_loses_signal"):
        g = runtime.geometry(DIRECTED[name][0], limits_for(name, state_mem))
        assert g.variant & A.VARIANT_SIGNAL and not g.variant & (A.VARIANT_SCOPE | A.VARIANT_TICK | A.VARIANT_SELECT), name
        assert int(runtime.variant_name(g).split(", ")[3]) & ~16 == 15 | 2048, name                  # every class (ADDR or not) + the signal class
        assert bool(g.variant & 16) == (state_mem == A.STATE_GLOBAL)
    for w2, lim in ((W.pingpong(), A.Limits()), (W.raft_election(), A.Limits()), (W.tonic_unary(), A.Limits()),
                    (W.raft_select(), W.raft_select_limits()), (LW.ALL["kill_many_tasks"](), LW.limits("kill_many_tasks"))):
        assert not runtime.geometry(w2, lim).variant & A.VARIANT_SIGNAL


def _refused(build, match):
    wl = W.WorkloadBuilder()
    n = wl.create_node()
    a = wl.addr(n, 1)
    t = wl.task(n)
    build(wl, t, a, n)
    t.done()
    with pytest.raises(runtime.MadsimHipError, match=match):
        runtime.geometry(wl.build())


def test_validate_refuses_every_rule_violation():
    _refused(lambda wl, t, a, n: t._emit("SEND_CTRL_C", a=n + 1), "node operand out of range")
    _refused(lambda wl, t, a, n: t._emit("RECV_OR_CTRL_C", a=a, b=(T << 8) | 2), "b bit 0 is the only flag")
    _refused(lambda wl, t, a, n: t._emit("RECV_OR_CTRL_C", a=a, b=(T << 8) | 0x80), "b bit 0 is the only flag")
    _refused(lambda wl, t, a, n: t.recv_or_ctrl_c(a, 0xFE), "reserved")
    _refused(lambda wl, t, a, n: t._emit("RECV_OR_CTRL_C", a=9, b=T << 8), "socket operand out of range")
    _refused(lambda wl, t, a, n: t.recv_or_ctrl_c(wl.virtual_addr(1, 80), T), "virtual address")
    mix = "cannot be combined with timeout scopes, interval tickers"

    def scoped(wl, t, a, n):
        with t.timeout(ms=5):
            t.sleep(ms=1)
        t.ctrl_c()
    _refused(scoped, mix)
    _refused(lambda wl, t, a, n: (t.interval(ms=5), t.tick(), t.send_ctrl_c(n)), mix)
    _refused(lambda wl, t, a, n: (t.interval(ms=5), t.interval_reset(), t.recv_or_ctrl_c(a, T)), mix)
    _refused(lambda wl, t, a, n: (t.interval(ms=5), t.recv_or_tick(a, T), t.ctrl_c()), mix)
    _refused(lambda wl, t, a, n: (t.mark(), t.recv_from_timeout_at(a, T, ms=1), t.send_ctrl_c(n)), mix)

    def other_task(wl, t, a, n):                    # the rule is per workload, not per program
        c = wl.task(n); c.interval(ms=5); c.tick(); c.done()
        t.ctrl_c()
    _refused(other_task, mix)
    # what stays allowed beside the three ops: timeouts of one receive, marks, every other class
    wl = W.WorkloadBuilder(); n = wl.create_node(); a = wl.addr(n, 1); t = wl.task(n)
    t.bind(a); t.mark(); t.recv_from_timeout(a, T, ms=2); t.recv_or_ctrl_c(a, T, recv_first=True); t.send_ctrl_c(0); t.ctrl_c(); t.done()
    assert runtime.geometry(wl.build()).variant & A.VARIANT_SIGNAL


def test_a_signal_can_reset_a_node_so_two_listeners_are_refused():
    """SEND_CTRL_C without a handler is kill_id: the node counts as resettable for reset_node's unmodelled socket order."""
    wl = W.WorkloadBuilder(); m = wl.main()
    n = wl.create_node()
    a, b = wl.addr(n, 1), wl.addr(n, 2)
    t = wl.task(n)
    t.bind(a); t.bind(b); t.accept1(a); t.accept1(b); t.done()
    m.spawn(t); m.send_ctrl_c(n); m.done()
    with pytest.raises(runtime.MadsimHipError, match="two listening"):
        runtime.geometry(wl.build())


# ---- reference facts on SignalSim ----------------------------------------------------------------------------------------------------------
def test_the_references_own_two_tests_pass():
    for name in ("ctrl_c_kill", "ctrl_c_catch"):
        s = _sim(*DIRECTED[name])
        assert s.result["verdict"] == A.PASS, name
    assert _sim(*DIRECTED["ctrl_c_kill"]).killed_by_signal == 1
    c = _sim(*DIRECTED["ctrl_c_catch"])
    assert c.caught == 2 and c.killed_by_signal == 0


def test_directed_workloads_reach_what_they_are_named_for():
    r = _sim(*DIRECTED["install_then_restart"])
    assert r.result["verdict"] == A.PASS and r.caught == 2 and r.killed_by_signal == 1
    h = _sim(*DIRECTED["handler_outlives_its_task"])
    assert h.result["verdict"] == A.PASS and h.caught == 1 and h.lost_signals == 2 and h.killed_by_signal == 0
    k = _sim(*DIRECTED["signal_to_killed_node"])
    assert k.result["verdict"] == A.PASS and k.caught == 0 and k.killed_by_signal == 0
    p = _sim(*DIRECTED["signal_to_paused_node"])
    assert p.result["verdict"] == A.PASS and p.caught == 1
    o = _sim(*DIRECTED["signal_to_own_node"])
    assert o.result["verdict"] == A.PASS and o.caught == 1 and o.killed_by_signal == 1 and 0x99 in o.obs_list and 0x9A not in o.obs_list
    for seed in range(8):
        ls = _sim(*DIRECTED["recv_first_loses_signal"], seed=seed)
        assert ls.result["verdict"] == A.PASS and ls.lost_signals == 1 and ls.caught == 0 and ls.obs_list[0] == 0x51, seed
        lm = _sim(*DIRECTED["ctrl_c_first_loses_message"], seed=seed)
        assert lm.result["verdict"] == A.PASS and lm.lost_messages == 1 and lm.caught == 1 and lm.obs_list[0] == A.VAL_TIMEOUT, seed
    loops = [_sim(*DIRECTED[n], seed=s) for s in range(8) for n in ("select_loop_recv_first", "select_loop_ctrl_c_first")]
    assert sum(x.caught for x in loops) > 0 and sum(x.lost_messages for x in loops) > 0
    u = _sim(*DIRECTED["two_waiters"])
    assert u.result == dict(verdict=A.UNSUPPORTED, steps=0, clock_ns=0, msg_count=0, rng_calls=0, trace_hash=0, obs_hash=0, log="")
    t = _sim(*DIRECTED["two_waiters_in_turn"])
    assert t.result["verdict"] == A.PASS and t.caught == 2 and t.unsupported == 0
    g = _sim(*DIRECTED["graceful_shutdown"])
    assert g.result["verdict"] == A.PASS and g.caught == 4 and g.killed_by_signal == 1


def test_a_signal_wakes_without_a_draw_a_timer_or_a_message():
    """ctrl_c().await parks with no timer, and the send draws nothing: the run with the signal equals the run with a plain flag
    store in its place, but for the steps of the woken task."""
    def prog(send):
        wl = W.WorkloadBuilder(); m = wl.main()
        n, _ = _handler_node(wl)
        m.sleep(ms=2)
        if send:
            m.send_ctrl_c(n)
        else:
            m.trace(0)
        m.sleep(ms=2); m.done()
        return wl.build()
    a, b = _sim(prog(True), A.Config.default()), _sim(prog(False), A.Config.default())
    assert a.caught == 1 and a.result["msg_count"] == b.result["msg_count"] == 0
    assert a.result["steps"] == b.result["steps"] + 1                      # one more poll: the woken task's
    assert len(a.heap) == len(b.heap)                                      # no timer was made for the wait or the wake


def test_shutdown_race_fails_on_some_seeds_and_only_by_lost_signals():
    w, cfg = DIRECTED["shutdown_race"]
    runs = [_sim(w, cfg, s) for s in range(64)]
    failed = [s for s, r in enumerate(runs) if r.result["verdict"] == A.PANIC]
    assert 0 < len(failed) < 64 and all(r.result["verdict"] in (A.PASS, A.PANIC) for r in runs)
    assert all((runs[s].lost_signals > 0) == (s in failed) for s in range(64))


# ---- the fuzzer --------------------------------------------------------------------------------------------------------------------------
def test_signal_fuzz_reaches_every_rule_and_keeps_the_unsupported_share_low():
    tot = dict(killed_by_signal=0, caught=0, lost_signals=0, lost_messages=0, unsupported=0)
    n = 0
    for k in range(48):
        w, cfg, _ = fuzz_signal.random_signal_workload(random.Random(500 + k))
        for seed in range(4):
            s = _sim(w, cfg, seed)
            n += 1
            for f in tot:
                tot[f] += getattr(s, f)
    print("signal fuzz:", tot, "of", n, "seeds")
    assert all(v > 0 for v in tot.values()), tot
    assert tot["unsupported"] <= FUZZ_UNSUPPORTED_CAP * n, (tot["unsupported"], n)


# ---- the oracle yardstick --------------------------------------------------------------------------------------------------------------------
def _kill_workloads():
    out = []
    for name in sorted(LW.ALL):
        w = LW.ALL[name]()
        ops = {w.insns[i].op for i in range(w.struct.n_insns)}
        tiers = {A.OP[o] for o in ("TIMEOUT_BEGIN", "TIMEOUT_END", "INTERVAL", "TICK", "INTERVAL_RESET", "RECV_OR_TICK", "RECV_TIMEOUT_AT")}
        if A.OP["KILL"] in ops and not ops & tiers:
            out.append(name)
    return out


KILL_WORKLOADS = _kill_workloads()


def test_the_yardstick_has_workloads():
    assert len(KILL_WORKLOADS) >= 4 and "kill_many_tasks" in KILL_WORKLOADS


@pytest.mark.parametrize("name", KILL_WORKLOADS)
def test_reference_equals_the_oracle_on_the_kill_rewrite(name):
    w = LW.ALL[name]()
    w2 = S.rewrite_kill_as_send_ctrl_c(w)
    cfg = A.Config.default()
    want = parity.expected(w, 0, 4, cfg, LW.limits(name))
    for s in range(4):
        if int(want[s]["verdict"]) == A.UNSUPPORTED:
            continue
        try:
            got = S.SignalSim(w2, cfg, s).run()
        except NotImplementedError:               # (an op the generator restatement does not model: the emulator test below still holds)
            return
        assert {f: got[f] for f in FIELDS} == {f: int(want[s][f]) for f in FIELDS}, (name, s)


@pytest.mark.parametrize("state_mem", [A.STATE_LDS, A.STATE_GLOBAL])
@pytest.mark.parametrize("name", KILL_WORKLOADS)
def test_emu_send_ctrl_c_without_handlers_equals_the_oracle_on_kill(name, state_mem):
    """All 48 bytes: the SEND_CTRL_C form on the signal build against the parity expectation of the KILL form."""
    from tests import emu
    w = LW.ALL[name]()
    w2 = S.rewrite_kill_as_send_ctrl_c(w)
    cfg = A.Config.default()
    lim = LW.limits(name) or A.Limits()
    lim.state_mem = (lim.state_mem & ~0xff & ~(A.STATE_NARROW_HEAP | A.STATE_DEDUP_TIMERS)) | state_mem
    assert emu.geometry_params(w2, lim)["features"] & 2048
    got = emu.run_batch(w2, 0, 6, cfg, lim)
    want = parity.expected(w, 0, 6, cfg, lim)
    parity.compare(got, want, lambda: parity.resolve_seed_by_seed(emu.run_batch, w2, 0, got, cfg, lim), name, None, (name, state_mem),
                   lambda i: parity.beyond_ceiling(w, i, cfg, lim))


# ---- emulator parity ---------------------------------------------------------------------------------------------------------------------
def assert_equals_signal_sim(got, w, cfg, seed0, label):
    for i in range(len(got)):
        want = S.SignalSim(w, cfg, seed0 + i).run()
        assert {f: int(got[i][f]) for f in FIELDS} == {f: want[f] for f in FIELDS}, (label, seed0 + i)


@pytest.mark.parametrize("name", sorted(DIRECTED))
def test_emu_directed_signal_workloads_equal_signal_sim(name):
    w, cfg = DIRECTED[name]
    for sm in (A.STATE_LDS, A.STATE_GLOBAL):
        got = resolved_emu(w, 0, 6, cfg, limits_for(name, sm))
        assert_equals_signal_sim(got, w, cfg, 0, (name, sm))


@pytest.mark.parametrize("block", ["fixed", "clock"])
def test_emu_signal_fuzz_equals_signal_sim(block):
    import time
    base = 500 if block == "fixed" else int(time.time()) % 1_000_000 * 100
    for k in range(24):
        w, cfg, _ = fuzz_signal.random_signal_workload(random.Random(base + k))
        got = resolved_emu(w, 0, 4, cfg, fuzz_signal.signal_limits(A.STATE_GLOBAL if k % 2 else A.STATE_LDS))
        assert_equals_signal_sim(got, w, cfg, 0, f"random_signal_workload(Random({base + k}))")


def test_emu_trace_seed_log_equals_signal_sim():
    from tests import emu
    for name in ("graceful_shutdown", "shutdown_race", "ctrl_c_catch", "ctrl_c_first_loses_message", "install_then_restart"):
        w, cfg = DIRECTED[name]
        lim = limits_for(name, 0)
        log, res = emu.trace_seed(w, 3, cfg, lim)
        while res["verdict"] == A.OVERFLOW:
            lim = parity.grow(lim, w.struct.n_progs)
            log, res = emu.trace_seed(w, 3, cfg, lim)
        want = S.SignalSim(w, cfg, 3).run()
        assert log.hex() == want["log"] and {f: int(res[f]) for f in FIELDS} == {f: want[f] for f in FIELDS}, name


# ---- no layout of an existing build moved ------------------------------------------------------------------------------------------------
# emu.geometry_params of the five bench cases on the parent commit (the signal class adds a node word and a `sub` bit only where it is compiled in)
BENCH_GEOMETRY = {
    'kv': {'dedup_n': 0,
     'dedup_off': 768,
     'features': 2,
     'gs_plane_words': 80,
     'gs_planes': 768,
     'gs_stride': 1088,
     'gstate_mode': 1,
     'heap_lds': 8,
     'heap_spill': 0,
     'lds_per_seed': 152,
     'max_tasks': 12,
     'mbox_msgs': 0,
     'mbox_regs': 0,
     'n_progs': 8,
     'n_socks': 5,
     'narrow': 0,
     'off_clog': 40,
     'off_conn': 44,
     'off_greg': 40,
     'off_handles': 25,
     'off_nodes': 33,
     'off_pause': 40,
     'off_socks': 0,
     'pool_n': 0,
     'sock_words': 5,
     'task_units': 3},
    'pingpong': {'dedup_n': 0,
     'dedup_off': 0,
     'features': 0,
     'gs_plane_words': 0,
     'gs_planes': 0,
     'gs_stride': 24,
     'gstate_mode': 0,
     'heap_lds': 4,
     'heap_spill': 0,
     'lds_per_seed': 152,
     'max_tasks': 5,
     'mbox_msgs': 0,
     'mbox_regs': 1,
     'n_progs': 5,
     'n_socks': 4,
     'narrow': 0,
     'off_clog': 8,
     'off_conn': 8,
     'off_greg': 8,
     'off_handles': 8,
     'off_nodes': 8,
     'off_pause': 8,
     'off_socks': 0,
     'pool_n': 0,
     'sock_words': 2,
     'task_units': 2},
    'raft': {'dedup_n': 64,
     'dedup_off': 704,
     'features': 1,
     'gs_plane_words': 534,
     'gs_planes': 1728,
     'gs_stride': 4416,
     'gstate_mode': 1,
     'heap_lds': 20,
     'heap_spill': 236,
     'lds_per_seed': 192,
     'max_tasks': 11,
     'mbox_msgs': 10,
     'mbox_regs': 80,
     'n_progs': 11,
     'n_socks': 5,
     'narrow': 1,
     'off_clog': 528,
     'off_conn': 534,
     'off_greg': 530,
     'off_handles': 510,
     'off_nodes': 521,
     'off_pause': 530,
     'off_socks': 0,
     'pool_n': 64,
     'sock_words': 102,
     'task_units': 3},
    'timers': {'dedup_n': 0,
     'dedup_off': 0,
     'features': 0,
     'gs_plane_words': 0,
     'gs_planes': 0,
     'gs_stride': 0,
     'gstate_mode': 0,
     'heap_lds': 4,
     'heap_spill': 64,
     'lds_per_seed': 748,
     'max_tasks': 25,
     'mbox_msgs': 2,
     'mbox_regs': 2,
     'n_progs': 25,
     'n_socks': 0,
     'narrow': 0,
     'off_clog': 25,
     'off_conn': 25,
     'off_greg': 25,
     'off_handles': 25,
     'off_nodes': 25,
     'off_pause': 25,
     'off_socks': 25,
     'pool_n': 0,
     'sock_words': 7,
     'task_units': 2},
    'topo': {'dedup_n': 0,
     'dedup_off': 1792,
     'features': 15,
     'gs_plane_words': 410,
     'gs_planes': 1792,
     'gs_stride': 3968,
     'gstate_mode': 1,
     'heap_lds': 31,
     'heap_spill': 161,
     'lds_per_seed': 296,
     'max_tasks': 28,
     'mbox_msgs': 5,
     'mbox_regs': 6,
     'n_progs': 22,
     'n_socks': 16,
     'narrow': 1,
     'off_clog': 368,
     'off_conn': 374,
     'off_greg': 370,
     'off_handles': 336,
     'off_nodes': 358,
     'off_pause': 370,
     'off_socks': 0,
     'pool_n': 64,
     'sock_words': 21,
     'task_units': 4},
}


def test_bench_case_geometries_are_what_they_were():
    from tests import emu
    assert sorted(BENCH_GEOMETRY) == ["kv", "pingpong", "raft", "timers", "topo"]
    for name, want in BENCH_GEOMETRY.items():
        w, lim, _ = W.bench_case(name)
        assert emu.geometry_params(w, lim) == want, name


def test_the_node_word_exists_only_for_signal_workloads():
    from tests import emu
    w = LW.ALL["kill_many_tasks"]()
    lim = LW.limits("kill_many_tasks")
    a, b = emu.geometry_params(w, lim), emu.geometry_params(S.rewrite_kill_as_send_ctrl_c(w), lim)
    assert b["off_clog"] - b["off_nodes"] == a["off_clog"] - a["off_nodes"] + 1 and b["features"] == a["features"] | 2048
