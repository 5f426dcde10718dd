"""Timeout scopes on the MI355X: the scope builds against the CPU reference (tests/scope_sim.py) and against the parity expectation of
the single-await timeouts they restate.  Seeds are printed on failure."""
import random
import time

import numpy as np
import pytest

from madsim_amd import _abi as A
from madsim_amd import workload as W
from tests import fuzz, fuzz_scope, parity
from tests import scope_sim as S
from tests.test_timeout_scope import DIRECTED, FIELDS, _timed_programs, assert_equals_scope_sim, scope_limits

pytestmark = pytest.mark.gpu


def _same_limits(lim):
    g = A.Limits()
    for f, _ in A.Limits._fields_:
        setattr(g, f, getattr(lim, f))
    return g


def test_gpu_directed_scope_workloads_equal_scope_sim(hip):
    for name, (w, cfg) in sorted(DIRECTED.items()):
        for sm in (A.STATE_LDS, A.STATE_GLOBAL):
            got, _ = hip.run_batch_auto(w, 100, 24, cfg, scope_limits(sm))
            assert_equals_scope_sim(got, w, cfg, 100, (name, sm))


@pytest.mark.parametrize("block", ["fixed", "clock"])
def test_gpu_scope_fuzz_equals_scope_sim(hip, block):
    base = 7000 if block == "fixed" else int(time.time()) % 1_000_000 * 100
    for k in range(12):
        w, cfg, _ = fuzz_scope.random_scope_workload(random.Random(base + k))
        seed0 = 1000 * k
        got, _ = hip.run_batch_auto(w, seed0, 12, cfg, scope_limits(A.STATE_GLOBAL if k % 2 else A.STATE_LDS))
        assert_equals_scope_sim(got, w, cfg, seed0, f"random_scope_workload(Random({base + k})) seeds {seed0}..")


@pytest.mark.parametrize("state_mem", [A.STATE_LDS, A.STATE_GLOBAL])
def test_gpu_rewritten_programs_equal_the_parity_expectation_of_the_originals(hip, state_mem):
    for name, k, w, cfg in _timed_programs(6):
        lim = fuzz.generous_limits()
        lim.state_mem = state_mem
        if state_mem == A.STATE_GLOBAL:
            lim.lanes_per_wave = 0
        w2 = S.rewrite_into_scopes(w)
        assert hip.geometry(w2, lim).variant & A.VARIANT_SCOPE
        got, _ = hip.run_batch(w2, 0, 96, cfg, lim)
        want = parity.expected(w, 0, 96, cfg, lim)
        parity.compare(got, want, lambda: parity.resolve_with_auto(hip.run_batch_auto, w2, 0, 96, cfg, lim),
                       f"{name}/{k}", None, (name, k, state_mem), lambda i: parity.beyond_ceiling(w, i, cfg, lim))


@pytest.mark.parametrize("case", ["raft_election", "streaming_topology"])
def test_gpu_bench_workloads_rewritten_into_scopes_are_bit_identical(hip, case):
    w, lim, n = {"raft_election": (W.raft_election(), W.raft_election_limits(), 262144),
                 "streaming_topology": (W.streaming_topology(), W.streaming_topology_limits(), 524288)}[case]
    w2 = S.rewrite_into_scopes(w)
    assert hip.geometry(w2, lim).variant & A.VARIANT_SCOPE and not hip.geometry(w, lim).variant & A.VARIANT_SCOPE
    a, _ = hip.run_batch_auto(w, 0, n, None, lim)
    b, _ = hip.run_batch_auto(w2, 0, n, None, lim)
    bad = np.nonzero(a != b)[0]
    assert len(bad) == 0, (case, f"{len(bad)} seeds differ, first {int(bad[0]) if len(bad) else None}")


def test_gpu_trace_seed_log_equals_scope_sim(hip):
    for name in ("tonic_unary", "kill_mid_scope", "crecv_backoff"):
        w, cfg = DIRECTED[name]
        lim = W.tonic_unary_limits()
        for seed in (3, 11):
            log, res = hip.trace_seed(w, seed, cfg, lim)
            want = S.ScopeSim(w, cfg, seed).run()
            assert log.hex() == want["log"] and {f: int(getattr(res, f)) for f in FIELDS} == {f: want[f] for f in FIELDS}, (name, seed)


def test_gpu_campaign_stops_at_the_first_failing_seed_scope_sim_finds(hip):
    # a 68 ms deadline over ~50 ms of service time plus latencies: now and then a call times out, and the test asserts that none does
    w = W.tonic_unary(n_clients=2, n_calls=3, timeout_ms=68, svc_ms=50, clog=False, kill=False, min_ok=6)
    cfg = A.Config.default()
    first = next(s for s in range(4096) if S.ScopeSim(w, cfg, s).run()["verdict"] != A.PASS)
    assert first > 64
    rep = hip.run_campaign(w, 0, 1 << 16, batch=64, in_flight=3, stop_at_failure=True, config=cfg, limits=W.tonic_unary_limits())
    assert rep.first_failing_seed == first, (rep.first_failing_seed, first)
    assert rep.n_failed >= 1 and rep.n_runner == 0
