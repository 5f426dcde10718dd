"""Interval tickers on the MI355X: the ticker builds against the CPU reference (tests/interval_sim.py) and against the parity
expectation of the straight-line programs' MARK + SLEEP_UNTIL rewrite.  Seeds are printed on failure."""
import random
import time

import numpy as np
import pytest

from madsim_amd import _abi as A
from madsim_amd import workload as W
from tests import fuzz_interval, parity
from tests import interval_sim as I
from tests.test_interval import DIRECTED, FIELDS, assert_equals_interval_sim, straight_line_programs

pytestmark = pytest.mark.gpu


def test_gpu_directed_interval_workloads_equal_interval_sim(hip):
    for name, (w, cfg) in sorted(DIRECTED.items()):
        for sm in (A.STATE_LDS, A.STATE_GLOBAL):
            got, _ = hip.run_batch_auto(w, 100, 16, cfg, fuzz_interval.interval_limits(sm))
            assert_equals_interval_sim(got, w, cfg, 100, (name, sm))


@pytest.mark.parametrize("block", ["fixed", "clock"])
def test_gpu_interval_fuzz_equals_interval_sim(hip, block):
    base = 8000 if block == "fixed" else int(time.time()) % 1_000_000 * 100
    for k in range(12):
        w, cfg, _ = fuzz_interval.random_interval_workload(random.Random(base + k))
        seed0 = 1000 * k
        got, _ = hip.run_batch_auto(w, seed0, 12, cfg, fuzz_interval.interval_limits(A.STATE_GLOBAL if k % 2 else A.STATE_LDS))
        assert_equals_interval_sim(got, w, cfg, seed0, f"random_interval_workload(Random({base + k})) seeds {seed0}..")


@pytest.mark.parametrize("state_mem", [A.STATE_LDS, A.STATE_GLOBAL])
def test_gpu_straight_line_programs_equal_the_parity_expectation_of_the_rewrite(hip, state_mem):
    for k, w, cfg in straight_line_programs(8, base=6100):
        lim = fuzz_interval.interval_limits(state_mem)
        assert hip.geometry(w, lim).variant & A.VARIANT_TICK
        w2 = I.rewrite_ticks_as_sleep_until(w)
        got, _ = hip.run_batch(w, 0, 96, cfg, lim)
        want = parity.expected(w2, 0, 96, cfg, lim)
        parity.compare(got, want, lambda: parity.resolve_with_auto(hip.run_batch_auto, w, 0, 96, cfg, lim),
                       f"straight/{k}", None, (k, state_mem), lambda i: parity.beyond_ceiling(w2, i, cfg, lim))


def test_gpu_trace_seed_log_equals_interval_sim(hip):
    for name in ("raft_ticker", "lease_keeper", "scoped_tick", "paused_burst"):
        w, cfg = DIRECTED[name]
        for seed in (3, 11):
            lim = fuzz_interval.interval_limits()
            log, res = hip.trace_seed(w, seed, cfg, lim)
            while int(res.verdict) == A.OVERFLOW:          # (a capacity verdict: the trace is run again with grown capacities)
                lim = parity.grow(lim, w.struct.n_progs)
                log, res = hip.trace_seed(w, seed, cfg, lim)
            want = I.IntervalSim(w, cfg, seed).run()
            assert log.hex() == want["log"] and {f: int(getattr(res, f)) for f in FIELDS} == {f: want[f] for f in FIELDS}, (name, seed)


def test_gpu_campaign_stops_at_the_first_failing_seed_interval_sim_finds(hip):
    w = W.raft_ticker(min_ticks=34)             # a few seeds in a hundred: the leaders ticked fewer than 34 times in all
    cfg = A.Config.default()
    first = next(s for s in range(4096) if I.IntervalSim(w, cfg, s).run()["verdict"] != A.PASS)
    rep = hip.run_campaign(w, 0, 1 << 16, batch=64, in_flight=3, stop_at_failure=True, config=cfg, limits=W.raft_ticker_limits())
    assert rep.first_failing_seed == first, (rep.first_failing_seed, first)
    assert rep.n_failed >= 1 and rep.n_runner == 0


def test_gpu_raft_ticker_full_batch_is_identical_in_both_layouts(hip):
    w, n = W.raft_ticker(), 262144
    lds, glb = W.raft_ticker_limits(), W.raft_ticker_limits()
    lds.state_mem, lds.lanes_per_wave = A.STATE_LDS, 0
    assert hip.geometry(w, glb).variant & A.VARIANT_TICK and hip.geometry(w, lds).variant & A.VARIANT_TICK
    a, _ = hip.run_batch_auto(w, 0, n, None, glb)
    b, _ = hip.run_batch_auto(w, 0, n, None, lds)
    bad = np.nonzero(a != b)[0]
    assert len(bad) == 0, f"{len(bad)} seeds differ, first {int(bad[0]) if len(bad) else None}"
    cfg = A.Config.default()
    for s in random.Random(7).sample(range(n), 24):
        want = I.IntervalSim(w, cfg, s).run()
        assert {f: int(a[s][f]) for f in FIELDS} == {f: want[f] for f in FIELDS}, s
