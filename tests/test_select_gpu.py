"""select_biased! over a receive and a tick (MS_OP_RECV_OR_TICK) and timeout_at (MS_OP_RECV_TIMEOUT_AT) on the MI355X: the ticker builds
against the CPU reference (tests/select_sim.py) and against the parity expectation of the two oracle yardsticks' rewrites.  Seeds are
printed on failure."""
import random
import time

import numpy as np
import pytest

from madsim_amd import _abi as A
from madsim_amd import workload as W
from tests import fuzz_select, parity
from tests import select_sim as S
from tests.test_select import DIRECTED, FIELDS, YARDSTICKS, assert_equals_select_sim, limits_for

pytestmark = pytest.mark.gpu

RAFT_SELECT_MIN_TICKS = 42


def test_gpu_directed_select_workloads_equal_select_sim(hip):
    for name, (w, cfg) in sorted(DIRECTED.items()):
        for sm in (A.STATE_LDS, A.STATE_GLOBAL):
            got, _ = hip.run_batch_auto(w, 100, 16, cfg, limits_for(name, sm))
            assert_equals_select_sim(got, w, cfg, 100, (name, sm))


@pytest.mark.parametrize("block", ["fixed", "clock"])
def test_gpu_select_fuzz_equals_select_sim(hip, block):
    base = 9000 if block == "fixed" else int(time.time()) % 1_000_000 * 100
    for k in range(12):
        w, cfg, _ = fuzz_select.random_select_workload(random.Random(base + k))
        seed0 = 1000 * k
        got, _ = hip.run_batch_auto(w, seed0, 12, cfg, fuzz_select.select_limits(A.STATE_GLOBAL if k % 2 else A.STATE_LDS))
        assert_equals_select_sim(got, w, cfg, seed0, f"random_select_workload(Random({base + k})) seeds {seed0}..")


@pytest.mark.parametrize("state_mem", [A.STATE_LDS, A.STATE_GLOBAL])
@pytest.mark.parametrize("name,progs,rewrite", YARDSTICKS, ids=[y[0] for y in YARDSTICKS])
def test_gpu_yardsticks_equal_the_parity_expectation_of_the_rewrite(hip, name, progs, rewrite, state_mem):
    for k, w, cfg in progs(6, 8100):
        lim = fuzz_select.select_limits(state_mem)
        assert hip.geometry(w, lim).variant & A.VARIANT_SELECT
        w2 = rewrite(w)
        got, _ = hip.run_batch(w, 0, 96, cfg, lim)
        want = parity.expected(w2, 0, 96, cfg, lim)
        parity.compare(got, want, lambda: parity.resolve_with_auto(hip.run_batch_auto, w, 0, 96, cfg, lim),
                       f"{name}/{k}", None, (k, state_mem), lambda i: parity.beyond_ceiling(w2, i, cfg, lim))


def test_gpu_trace_seed_log_equals_select_sim(hip):
    for name in ("raft_select", "lost", "stale_wake", "tick_first_due", "timeout_at_fixed"):
        w, cfg = DIRECTED[name]
        for seed in (3, 11):
            lim = limits_for(name, 0)
            log, res = hip.trace_seed(w, seed, cfg, lim)
            while int(res.verdict) == A.OVERFLOW:          # (a capacity verdict: the trace is run again with grown capacities)
                lim = parity.grow(lim, w.struct.n_progs)
                log, res = hip.trace_seed(w, seed, cfg, lim)
            want = S.SelectSim(w, cfg, seed).run()
            assert log.hex() == want["log"] and {f: int(getattr(res, f)) for f in FIELDS} == {f: want[f] for f in FIELDS}, (name, seed)


def test_gpu_campaign_stops_at_the_first_failing_seed_select_sim_finds(hip):
    w = W.raft_select(min_ticks=RAFT_SELECT_MIN_TICKS)    # some seeds fail: the leaders ticked fewer times in all
    cfg = A.Config.default()
    first = next(s for s in range(4096) if S.SelectSim(w, cfg, s).run()["verdict"] != A.PASS)
    rep = hip.run_campaign(w, 0, 1 << 16, batch=64, in_flight=3, stop_at_failure=True, config=cfg, limits=W.raft_select_limits())
    assert rep.first_failing_seed == first, (rep.first_failing_seed, first)
    assert rep.n_failed >= 1 and rep.n_runner == 0


def test_gpu_raft_select_full_batch_is_identical_in_both_layouts(hip):
    w, n = W.raft_select(), 262144
    lds, glb = W.raft_select_limits(), W.raft_select_limits()
    lds.state_mem, lds.lanes_per_wave = A.STATE_LDS, 0
    assert hip.geometry(w, glb).variant & A.VARIANT_SELECT and hip.geometry(w, lds).variant & A.VARIANT_SELECT
    a, _ = hip.run_batch_auto(w, 0, n, None, glb)
    b, _ = hip.run_batch_auto(w, 0, n, None, lds)
    bad = np.nonzero(a != b)[0]
    assert len(bad) == 0, f"{len(bad)} seeds differ, first {int(bad[0]) if len(bad) else None}"
    cfg = A.Config.default()
    for s in random.Random(7).sample(range(n), 24):
        want = S.SelectSim(w, cfg, s).run()
        assert {f: int(a[s][f]) for f in FIELDS} == {f: want[f] for f in FIELDS}, s
