"""Ctrl-c signals (MS_OP_CTRL_C / MS_OP_SEND_CTRL_C / MS_OP_RECV_OR_CTRL_C) on the MI355X: the signal builds against the CPU reference
(tests/signal_sim.py) and, for nodes without a handler, against the parity expectation of the KILL form (the unchanged oracle).
Seeds are printed on failure."""
import random
import time

import numpy as np
import pytest

from madsim_amd import _abi as A
from madsim_amd import workload as W
from tests import fuzz_signal, lifecycle_workloads as LW, parity
from tests import signal_sim as S
from tests.test_signal import DIRECTED, FIELDS, KILL_WORKLOADS, assert_equals_signal_sim, limits_for

pytestmark = pytest.mark.gpu


def test_gpu_directed_signal_workloads_equal_signal_sim(hip):
    for name, (w, cfg) in sorted(DIRECTED.items()):
        for sm in (A.STATE_LDS, A.STATE_GLOBAL):
            lim = limits_for(name, sm)
            assert hip.geometry(w, lim).variant & A.VARIANT_SIGNAL
            got, _ = hip.run_batch_auto(w, 100, 16, cfg, lim)
            assert_equals_signal_sim(got, w, cfg, 100, (name, sm))


@pytest.mark.parametrize("block", ["fixed", "clock"])
def test_gpu_signal_fuzz_equals_signal_sim(hip, block):
    base = 9000 if block == "fixed" else int(time.time()) % 1_000_000 * 100
    print("signal fuzz base", base)
    for k in range(12):
        w, cfg, _ = fuzz_signal.random_signal_workload(random.Random(base + k))
        seed0 = 1000 * k
        got, _ = hip.run_batch_auto(w, seed0, 12, cfg, fuzz_signal.signal_limits(A.STATE_GLOBAL if k % 2 else A.STATE_LDS))
        assert_equals_signal_sim(got, w, cfg, seed0, f"random_signal_workload(Random({base + k})) seeds {seed0}..")


@pytest.mark.parametrize("state_mem", [A.STATE_LDS, A.STATE_GLOBAL])
def test_gpu_send_ctrl_c_without_handlers_equals_the_oracle_on_kill(hip, state_mem):
    for name in KILL_WORKLOADS:
        w = LW.ALL[name]()
        w2 = S.rewrite_kill_as_send_ctrl_c(w)
        cfg = A.Config.default()
        lim = LW.limits(name) or A.Limits()
        lim.state_mem = (lim.state_mem & ~0xff & ~(A.STATE_NARROW_HEAP | A.STATE_DEDUP_TIMERS)) | state_mem
        assert hip.geometry(w2, lim).variant & A.VARIANT_SIGNAL and not hip.geometry(w, lim).variant & A.VARIANT_SIGNAL
        got, _ = hip.run_batch(w2, 0, 96, cfg, lim)
        want = parity.expected(w, 0, 96, cfg, lim)
        parity.compare(got, want, lambda: parity.resolve_with_auto(hip.run_batch_auto, w2, 0, 96, cfg, lim),
                       name, None, (name, state_mem), lambda i: parity.beyond_ceiling(w, i, cfg, lim))


def test_gpu_trace_seed_log_equals_signal_sim(hip):
    for name in ("graceful_shutdown", "shutdown_race", "ctrl_c_catch", "ctrl_c_first_loses_message", "recv_first_loses_signal", "install_then_restart"):
        w, cfg = DIRECTED[name]
        for seed in (3, 11):
            lim = limits_for(name, 0)
            log, res = hip.trace_seed(w, seed, cfg, lim)
            while int(res.verdict) == A.OVERFLOW:          # (a capacity verdict: the trace is run again with grown capacities)
                lim = parity.grow(lim, w.struct.n_progs)
                log, res = hip.trace_seed(w, seed, cfg, lim)
            want = S.SignalSim(w, cfg, seed).run()
            assert log.hex() == want["log"] and {f: int(getattr(res, f)) for f in FIELDS} == {f: want[f] for f in FIELDS}, (name, seed)


def test_gpu_campaign_stops_at_the_first_failing_seed_signal_sim_finds(hip):
    w = W.shutdown_race()                               # some seeds lose a signal between two selects and fail the supervisor's assertion
    cfg = A.Config.default()
    first = next(s for s in range(4096) if S.SignalSim(w, cfg, s).run()["verdict"] != A.PASS)
    rep = hip.run_campaign(w, 0, 1 << 16, batch=64, in_flight=3, stop_at_failure=True, config=cfg, limits=W.shutdown_race_limits())
    assert rep.first_failing_seed == first, (rep.first_failing_seed, first)
    assert rep.n_failed >= 1 and rep.n_runner == 0


def test_gpu_graceful_shutdown_full_batch_is_identical_in_both_layouts(hip):
    w, n = W.graceful_shutdown(), 262144
    lds, glb = W.graceful_shutdown_limits(), W.graceful_shutdown_limits()
    lds.state_mem, glb.state_mem = A.STATE_LDS, A.STATE_GLOBAL
    assert hip.geometry(w, glb).variant & A.VARIANT_SIGNAL and hip.geometry(w, lds).variant & A.VARIANT_SIGNAL
    assert hip.geometry(w, glb).variant & 16 and not hip.geometry(w, lds).variant & 16
    a, _ = hip.run_batch_auto(w, 0, n, None, glb)
    b, _ = hip.run_batch_auto(w, 0, n, None, lds)
    bad = np.nonzero(a != b)[0]
    assert len(bad) == 0, f"{len(bad)} seeds differ, first {int(bad[0]) if len(bad) else None}"
    cfg = A.Config.default()
    for s in random.Random(7).sample(range(n), 24):
        want = S.SignalSim(w, cfg, s).run()
        assert {f: int(a[s][f]) for f in FIELDS} == {f: want[f] for f in FIELDS}, s
