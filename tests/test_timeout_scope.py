"""Timeout scopes (MS_OP_TIMEOUT_BEGIN / MS_OP_TIMEOUT_END): time::timeout over a block of awaits — CPU side.

* the CPU reference (tests/scope_sim.py) against itself: timeout(d, f) == timeout(d, async { f.await }) on every fuzz program
  with a single-await timeout, rewritten into a scope — every result field and the raw determinism log;
* the host-compiled kernel (tests/emu) on the rewritten programs against the parity expectation of the ORIGINAL programs
  (derived from the unchanged C oracle), and on directed scope workloads and the scope fuzz generator against ScopeSim;
* validate()'s static rules.
"""
import random

import numpy as np
import pytest

import oracle
from madsim_amd import _abi as A
from madsim_amd import runtime
from madsim_amd import workload as W
from tests import fuzz, fuzz_scope, parity
from tests import scope_sim as S

FIELDS = ["verdict", "steps", "clock_ns", "msg_count", "rng_calls", "trace_hash", "obs_hash"]
TIMED_GENS = [(fuzz.random_workload, 1000), (fuzz.random_timeout_workload, 92000), (fuzz.random_mixed_workload, 9900),
              (fuzz.random_rpc_workload, 31000), (fuzz.random_unstructured_wide_workload, 77000)]


def _timed_programs(per_gen):
    for gen, base in TIMED_GENS:
        n = 0
        for k in range(400):
            w, cfg, _ = gen(random.Random(base + k))
            if S.has_timed_ops(w):
                yield gen.__name__, base + k, w, cfg
                n += 1
                if n == per_gen:
                    break


def _sim(cls, w, cfg, seed):
    try:
        return cls(w, cfg, seed).run()
    except Exception as e:          # (a program the generator restatement itself does not model: both sides must agree on that too)
        return type(e).__name__


# ---- directed workloads ---------------------------------------------------------------------------------------------------------
def _client_server(scope_body, server="none", svc_ms=50, cfg=None, kill_at_ms=0, clog_ms=0):
    """One server node (datagram echo / connection handler / rpc handler, or nothing listening) and one client that runs
    `scope_body(c, acl, addrs, s)` inside `timeout(..)`, then traces val."""
    wl = W.WorkloadBuilder()
    ns = wl.create_node()
    a_dg, a_ch, a_rpc = wl.addr(ns, 100), wl.addr(ns, 200), wl.addr(ns, 300)
    if server != "none":
        fuzz_scope._servers(wl, ns, a_dg, a_ch, a_rpc, svc_ms)
    nc = wl.create_node()
    acl = wl.addr(nc, 7)
    c = wl.task(nc)
    c.bind(acl); c.set(0, 3)
    top = c.label()
    scope_body(c, acl, (a_dg, a_ch, a_rpc))
    c.trace_val(); c.trace_instant(); c.djnz(0, top); c.done()
    m = wl.main()
    m.spawn(c)
    if clog_ms:
        m.clog_link(ns, nc); m.sleep(ms=clog_ms); m.unclog_link(ns, nc)
    if kill_at_ms:
        m.sleep(ms=kill_at_ms); m.kill(ns)
    m.join(c)
    m.done()
    return wl.build(), cfg or A.Config.default()


def _scoped(ms=0, us=0, **_):
    def wrap(fn):
        def body(c, acl, addrs):
            with c.timeout(ms=ms, us=us) as s:
                fn(c, acl, addrs, s)
        return body
    return wrap


def directed():
    out = {}
    # expiry inside a send's rand_delay (buggify: rand_delay up to 4 s) and inside connect1's
    out["send_rand_delay"] = _client_server(_scoped(ms=2)(lambda c, acl, a, s: (c.send_to(acl, a[0], 1, 5), c.recv_from(acl, 2))),
                                            "all", cfg=A.Config.default(buggify=True))
    out["connect_rand_delay"] = _client_server(_scoped(ms=3)(lambda c, acl, a, s: (c.connect1(acl, a[1]), c.jeq(A.VAL_REFUSED, s.end),
                                                                                 c.chan_send(1), c.chan_recv())), "all", cfg=A.Config.default(buggify=True))
    # the connection made, crecv parked on a slow handler
    out["crecv_parked"] = _client_server(_scoped(ms=20)(lambda c, acl, a, s: (c.connect1(acl, a[1]), c.jeq(A.VAL_REFUSED, s.end),
                                                                             c.chan_send(1), c.chan_recv())), "all", svc_ms=200)
    # the receiver's backoff on a clogged link
    out["crecv_backoff"] = _client_server(_scoped(ms=30)(lambda c, acl, a, s: (c.connect1(acl, a[1]), c.jeq(A.VAL_REFUSED, s.end),
                                                                              c.chan_send(1), c.chan_recv())), "all", svc_ms=1, clog_ms=60)
    # inside an untimed rpc_call (the send's rand_delay, the response wait, the response's rand_delay)
    out["rpc_call"] = _client_server(_scoped(ms=6)(lambda c, acl, a, s: c.rpc_call(acl, a[2], 1, 9)), "all", svc_ms=8)
    # completion exactly at the deadline: the block is polled first and wins
    out["at_deadline"] = _client_server(_scoped(ms=5)(lambda c, acl, a, s: (c.sleep(ms=5), c.trace(1))))
    out["under_floor"] = _client_server(_scoped(us=300)(lambda c, acl, a, s: (c.sleep(us=999), c.yield_now(), c.sleep_rand(lo_ms=0, ms=1))))
    # early exit on VAL_REFUSED: nobody listens
    out["refused"] = _client_server(_scoped(ms=50)(lambda c, acl, a, s: (c.connect1(acl, a[1]), c.jeq(A.VAL_REFUSED, s.end),
                                                                        c.chan_send(1), c.chan_recv())))
    # the server node killed mid-call
    out["kill_mid_scope"] = _client_server(_scoped(ms=40)(lambda c, acl, a, s: (c.connect1(acl, a[1]), c.jeq(A.VAL_REFUSED, s.end),
                                                                               c.chan_send(1), c.chan_recv(), c.trace_val(),
                                                                               c.send_to(acl, a[0], 1, 5), c.recv_from(acl, 2))),
                                           "all", svc_ms=30, kill_at_ms=15)
    out["tonic_unary"] = (W.tonic_unary(), A.Config.default())
    out["tonic_unary_loss"] = (W.tonic_unary(n_clients=3, timeout_ms=25), A.Config.default(packet_loss_rate=0.1))
    return out


DIRECTED = directed()


def scope_limits(state_mem=0):
    lim = fuzz_scope.scope_limits()
    lim.state_mem = state_mem
    return lim


def resolved_emu(w, seed0, count, cfg, lim):
    """The host-compiled kernel, seeds that came back with a capacity verdict re-run with grown capacities (parity.py)."""
    from tests import emu
    got = emu.run_batch(w, seed0, count, cfg, lim)
    for i in np.nonzero(got["verdict"] == A.OVERFLOW)[0]:
        g = lim
        for _ in range(8):
            g = parity.grow(g, w.struct.n_progs)
            r = emu.run_batch(w, seed0 + int(i), 1, cfg, g)
            if r[0]["verdict"] != A.OVERFLOW:
                break
        got[i] = r[0]
    return got


def assert_equals_scope_sim(got, w, cfg, seed0, label):
    for i in range(len(got)):
        want = S.ScopeSim(w, cfg, seed0 + i).run()
        assert {f: int(got[i][f]) for f in FIELDS} == {f: want[f] for f in FIELDS}, (label, seed0 + i)


# ---- tests ------------------------------------------------------------------------------------------------------------------------
def test_dsl_builds_scopes_with_forward_end_targets():
    wl = W.WorkloadBuilder()
    n = wl.create_node()
    a = wl.addr(n, 1)
    t = wl.task(n)
    t.bind(a)
    with t.timeout(ms=1500) as s:
        t.connect1(a, a); t.jeq(A.VAL_REFUSED, s.end); t.chan_send(3); t.chan_recv()
    t.done()
    w = wl.build()
    ins = [(w.insns[i].op, w.insns[i].a, w.insns[i].b, w.insns[i].imm) for i in range(w.struct.n_insns)]
    base = w.progs[1].entry
    begin = next(i for i, x in enumerate(ins) if x[0] == A.OP["TIMEOUT_BEGIN"])
    end = next(i for i, x in enumerate(ins) if x[0] == A.OP["TIMEOUT_END"])
    assert ins[begin] == (A.OP["TIMEOUT_BEGIN"], 1, end, 500_000_000) and begin == base + 1
    assert ins[begin + 2] == (A.OP["JEQ"], 0, end, A.VAL_REFUSED)
    g = runtime.geometry(w)
    assert g.variant & A.VARIANT_SCOPE and int(runtime.variant_name(g).split(", ")[3]) & 256
    # a workload without scopes selects what it always did
    assert not runtime.geometry(W.kv_rpc()).variant & A.VARIANT_SCOPE


def _refused(build, match):
    wl = W.WorkloadBuilder()
    n = wl.create_node()
    a, b = wl.addr(n, 1), wl.addr(n, 2)
    t = wl.task(n)
    t.bind(a)
    build(wl, t, a, b)
    t.done()
    with pytest.raises(runtime.MadsimHipError, match=match):
        runtime.geometry(wl.build())


def test_validate_refuses_every_static_rule_violation():
    def nested(wl, t, a, b):
        h = t.timeout_begin(ms=5); h2 = t.timeout_begin(ms=1); t.sleep(ms=1); t.timeout_end(h2); t.timeout_end(h)
    _refused(nested, "do not nest")

    def recv_timeout_inside(wl, t, a, b):
        with t.timeout(ms=5):
            t.recv_from_timeout(a, 1, ms=1)
    _refused(recv_timeout_inside, "not allowed inside")

    def timed_rpc(wl, t, a, b):
        with t.timeout(ms=5):
            t.rpc_call(a, b, 1, 3, timeout_ms=2)
    _refused(timed_rpc, "not allowed inside")
    for op in ("spawn", "done", "bind", "close", "accept1", "chan_close", "kill", "advance", "set_latency"):
        def bad(wl, t, a, b, op=op):
            with t.timeout(ms=5):
                {"spawn": lambda: t.spawn(t), "done": lambda: t.done(), "bind": lambda: t.bind(b), "close": lambda: t.close(a),
                 "accept1": lambda: t.accept1(a), "chan_close": lambda: t.chan_close(), "kill": lambda: t.kill(1),
                 "advance": lambda: t.advance(ms=1), "set_latency": lambda: t.set_latency(0)}[op]()
        _refused(bad, "not allowed inside")

    def chan_without_connect(wl, t, a, b):
        t.connect1(a, b)
        with t.timeout(ms=5):
            t.chan_send(1)
    _refused(chan_without_connect, "need a connect")

    def jump_in(wl, t, a, b):
        t.jmp(t.label() + 3)
        with t.timeout(ms=5):
            t.sleep(ms=1); t.sleep(ms=1)
    _refused(jump_in, "into a timeout scope")

    def jump_out(wl, t, a, b):
        with t.timeout(ms=5):
            t.jeq(1, t.label() + 3); t.sleep(ms=1)
        t.sleep(ms=1)
    _refused(jump_out, "out of a timeout scope")

    def orphan_end(wl, t, a, b):
        t._emit("TIMEOUT_END")
    _refused(orphan_end, "without its timeout_begin")

    def ok(wl, t, a, b):
        with t.timeout(ms=5) as s:
            t.connect1(a, b); t.jeq(A.VAL_REFUSED, s.end); t.chan_send(1); t.chan_recv(); t.jmp(s.end)
    wl = W.WorkloadBuilder(); n = wl.create_node(); a, b = wl.addr(n, 1), wl.addr(n, 2)
    t = wl.task(n); t.bind(a); ok(wl, t, a, b); t.done()
    runtime.geometry(wl.build())                 # a jump to its own END is the one way out of a scope
    # the C oracle restates the ops (tests/test_oracle_tiers.py holds it against ScopeSim at length); an op it lacks fails the call
    got, _ = oracle.run_batch(W.tonic_unary(), 0, 2)
    assert_equals_scope_sim(got, W.tonic_unary(), A.Config.default(), 0, "tonic_unary")


def test_reference_rewritten_into_scopes_equals_the_timed_ops():
    """timeout(d, f) == timeout(d, async { f.await }): ScopeSim on the rewritten program equals Sim on the original, every
    field and the raw log, under the generator's config."""
    n = 0
    for name, k, w, cfg in _timed_programs(12):
        w2 = S.rewrite_into_scopes(w)
        for s in range(3):
            a, b = _sim(S.Sim, w, cfg, s), _sim(S.ScopeSim, w2, cfg, s)
            assert a == b, (name, k, s)
            n += not isinstance(a, str) and a["steps"] > 0
    assert n > 100


@pytest.mark.parametrize("state_mem", [A.STATE_LDS, A.STATE_GLOBAL])
def test_emu_rewritten_programs_equal_the_parity_expectation_of_the_originals(state_mem):
    from tests import emu
    n = 0
    for name, k, w, cfg in _timed_programs(5):
        lim = fuzz.generous_limits()
        lim.state_mem = state_mem
        if state_mem == A.STATE_GLOBAL:
            lim.lanes_per_wave = 0               # (global state: full waves)
        w2 = S.rewrite_into_scopes(w)
        assert emu.geometry_params(w2, lim)["features"] & 256          # (MADSIM_FEAT_SCOPE: the scope builds run it)
        got = emu.run_batch(w2, 0, 6, cfg, lim)
        want = parity.expected(w, 0, 6, cfg, lim)
        parity.compare(got, want, lambda: parity.resolve_seed_by_seed(emu.run_batch, w2, 0, got, cfg, lim),
                       f"{name}/{k}", None, (name, k), lambda i: parity.beyond_ceiling(w, i, cfg, lim))
        n += 6
    assert n >= 120


@pytest.mark.parametrize("name", sorted(DIRECTED))
def test_emu_directed_scope_workloads_equal_scope_sim(name):
    w, cfg = DIRECTED[name]
    for sm in (A.STATE_LDS, A.STATE_GLOBAL):
        got = resolved_emu(w, 0, 6, cfg, scope_limits(sm))
        assert_equals_scope_sim(got, w, cfg, 0, (name, sm))


def test_directed_workloads_reach_what_they_are_named_for():
    """The directed workloads are not vacuous: some expire, some complete, the refused one returns early."""
    def vals(name, seed=0):
        w, cfg = DIRECTED[name]
        sim = S.ScopeSim(w, cfg, seed)
        sim.run()
        return sim.obs_list
    assert A.VAL_TIMEOUT in vals("crecv_parked") and A.VAL_TIMEOUT in vals("rpc_call")
    assert A.VAL_REFUSED in vals("refused") and A.VAL_TIMEOUT not in vals("refused")
    assert A.VAL_TIMEOUT not in vals("at_deadline") and A.VAL_TIMEOUT in vals("under_floor")
    assert any(A.VAL_TIMEOUT in vals("send_rand_delay", s) for s in range(8))


def test_emu_scope_fuzz_equals_scope_sim():
    for k in range(24):
        w, cfg, _ = fuzz_scope.random_scope_workload(random.Random(5000 + k))
        got = resolved_emu(w, 0, 4, cfg, scope_limits(A.STATE_GLOBAL if k % 2 else A.STATE_LDS))
        assert_equals_scope_sim(got, w, cfg, 0, ("fuzz_scope", 5000 + k))


def test_emu_trace_seed_log_equals_scope_sim():
    from tests import emu
    for name in ("tonic_unary", "kill_mid_scope", "rpc_call"):
        w, cfg = DIRECTED[name]
        lim = scope_limits()
        log, res = emu.trace_seed(w, 3, cfg, lim)
        while res["verdict"] == A.OVERFLOW:            # (a capacity verdict: the trace is run again with grown capacities)
            lim = parity.grow(lim, w.struct.n_progs)
            log, res = emu.trace_seed(w, 3, cfg, lim)
        want = S.ScopeSim(w, cfg, 3).run()
        assert log.hex() == want["log"] and {f: int(res[f]) for f in FIELDS} == {f: want[f] for f in FIELDS}, name
