"""Collecting campaigns on the MI355X: the list of failing seeds and the verdict histogram of madsim_hip_run_campaign_collect (and its
context / several-contexts forms) against a host filter over the CPU oracle's results of the same range (or, where the verdict is the
runner's own, over madsim_hip_run_batch's) — never against a second call of the code under test."""
import functools

import numpy as np
import pytest

import oracle
from madsim_amd import _abi as A
from madsim_amd import workload as W

pytestmark = pytest.mark.gpu

NONE = (1 << 64) - 1
SEED0, TOTAL, BATCH = 5_000_000, 40_000, 4096          # the lossy ping-pong range: 4 670 deadlocks, ragged last batch of 3 136
REPORT_FIELDS = ("seeds_run", "batches_run", "batches_launched", "first_failing_seed", "n_failed", "n_runner", "total_steps", "total_clock_ns")


def report(rep):
    return {f: int(getattr(rep, f)) for f in REPORT_FIELDS}


def listed(results, seed0, cap=None, list_runner=False):
    """The truth: the records a collecting campaign owes for per-seed `results` of [seed0, seed0 + len) — a filter on the host."""
    v = results["verdict"]
    idx = np.nonzero((v != A.PASS) & ((v < A.OVERFLOW) | list_runner))[0][:cap]
    rec = np.zeros(len(idx), dtype=A.FAILURE_DTYPE)
    rec["seed"] = seed0 + idx.astype(np.uint64)
    for f in results.dtype.names:
        rec[f] = results[f][idx]
    return rec


def check(got, results, seed0, cap, list_runner=False, plain=None, what=None):
    """(campaign, failures, by_verdict) of a collecting campaign over exactly the seeds of `results`."""
    rep, fails, hist = got
    want = listed(results, seed0, cap, list_runner)
    assert fails.dtype == np.dtype(A.FAILURE_DTYPE) and len(fails) == len(want), (what, len(fails), len(want))
    assert (fails["seed"] == want["seed"]).all(), (what, "seeds", fails["seed"][:8], want["seed"][:8])
    assert fails.tobytes() == want.tobytes(), (what, "result bytes")
    assert hist.dtype == np.uint64 and (hist == np.bincount(results["verdict"], minlength=8)).all(), (what, hist)
    assert int(hist.sum()) == rep.seeds_run == len(results) and int(hist[1:4].sum()) == rep.n_failed and int(hist[4:].sum()) == rep.n_runner, what
    if plain is not None:
        assert report(rep) == report(plain), what


@functools.lru_cache(maxsize=None)
def lossy_pingpong():
    w, cfg = W.pingpong(4, 16), A.Config.default(packet_loss_rate=0.002)
    want, _ = oracle.run_batch(w, SEED0, TOTAL, cfg)
    want.setflags(write=False)
    assert int((want["verdict"] == A.DEADLOCK).sum()) == 4670 == int((want["verdict"] != A.PASS).sum()) and want["verdict"][4] != A.PASS
    return w, cfg, want


@pytest.mark.parametrize("cap", [0, 1, 100, 1000, 8192])
def test_the_list_is_the_oracles(hip, cap):
    """Histogram only, one record, less than one batch's failures, a list spanning three batches, room for more than all."""
    w, cfg, want = lossy_pingpong()
    plain = hip.run_campaign(w, SEED0, TOTAL, BATCH, 3, False, cfg)
    got = hip.run_campaign(w, SEED0, TOTAL, BATCH, 3, False, cfg, collect=cap)
    check(got, want, SEED0, cap, plain=plain, what=cap)
    assert len(got[1]) == min(cap, 4670) and (got[0].batches_run, got[0].batches_launched) == (10, 10)


def test_the_list_does_not_depend_on_the_cut(hip):
    """batch (100: partial waves, count % 64 != 0; one batch for everything), batches in flight, one context or two: the same bytes."""
    w, cfg, want = lossy_pingpong()
    truth = listed(want, SEED0, 1000).tobytes()
    for batch, in_flight in ((100, 1), (100, 8), (4096, 1), (4096, 3), (4096, 8), (40_000, 3)):
        got = hip.run_campaign(w, SEED0, TOTAL, batch, in_flight, False, cfg, collect=1000)
        check(got, want, SEED0, 1000, what=(batch, in_flight))
        assert got[1].tobytes() == truth, (batch, in_flight)
    with hip.Context(0) as c0, hip.Context(0) as c1:
        for batch, in_flight in ((100, 3), (4096, 2)):
            many = hip.run_campaign_multi([c0, c1], w, SEED0, TOTAL, batch, in_flight, False, cfg, collect=1000)
            check(many, want, SEED0, 1000, plain=hip.run_campaign_multi([c0, c1], w, SEED0, TOTAL, batch, in_flight, False, cfg), what=("two contexts", batch))
            assert many[1].tobytes() == truth
        one = c0.run_campaign(w, SEED0, TOTAL, BATCH, 3, False, cfg, collect=1000)
        check(one, want, SEED0, 1000, plain=c0.run_campaign(w, SEED0, TOTAL, BATCH, 3, False, cfg), what="context form")
    # the smallest campaigns: one seed (a failing one, a passing one), one batch of a wave and one lane
    for seed0, total in ((SEED0 + 4, 1), (SEED0, 1), (SEED0, 65)):
        check(hip.run_campaign(w, seed0, total, 0, 0, False, cfg, collect=1000), want[seed0 - SEED0:seed0 - SEED0 + total], seed0, 1000,
              plain=hip.run_campaign(w, seed0, total, 0, 0, False, cfg), what=(seed0, total))


def test_truncation_inside_a_batch_is_by_seed_order(hip):
    """One batch of 40 000 holds 4 670 failing seeds spread over the pieces of 160 waves; room for 7: the 7 smallest, the same on every call."""
    w, cfg, want = lossy_pingpong()
    truth = listed(want, SEED0, 7)
    assert len(truth) == 7 and truth["seed"][0] == SEED0 + 4
    for _ in range(3):
        got = hip.run_campaign(w, SEED0, TOTAL, TOTAL, 1, False, cfg, collect=7)
        check(got, want, SEED0, 7, what="one batch, cap 7")
        assert got[1].tobytes() == truth.tobytes() and got[0].batches_run == 1


def test_stop_at_cap_stops_at_the_batch_that_fills_the_list(hip):
    w, cfg, want = lossy_pingpong()
    per_batch = [int((want["verdict"][k * BATCH:(k + 1) * BATCH] != A.PASS).sum()) for k in range(10)]
    j = int(np.nonzero(np.cumsum(per_batch) >= 600)[0][0])
    assert j == 1 and per_batch[:2] == [448, 465]
    rep, fails, hist = got = hip.run_campaign(w, SEED0, TOTAL, BATCH, 3, False, cfg, collect=600, stop_at_cap=True)
    assert rep.batches_run == j + 1 and rep.seeds_run == (j + 1) * BATCH and j + 1 <= rep.batches_launched <= j + 3
    check(got, want[:rep.seeds_run], SEED0, 600, what="stop at cap")
    assert len(fails) == 600
    # a cap the range never reaches: the whole range runs
    rep, fails, _ = got = hip.run_campaign(w, SEED0, TOTAL, BATCH, 3, False, cfg, collect=5000, stop_at_cap=True)
    assert (rep.batches_run, rep.batches_launched, len(fails)) == (10, 10, 4670)
    check(got, want, SEED0, 5000, what="cap beyond all")
    with pytest.raises(hip.MadsimHipError, match="STOP_AT_CAP"):
        hip.run_campaign(w, SEED0, TOTAL, BATCH, 3, False, cfg, collect=0, stop_at_cap=True)


def test_stop_at_failure_lists_the_stopping_batch(hip):
    """The rare-failure setting of the campaign test: the prefix ends with the batch that holds the first genuine failure."""
    w, cfg = W.pingpong(4, 16), A.Config.default(packet_loss_rate=0.000002)
    plain = hip.run_campaign(w, 9_000_000, 64 * BATCH, BATCH, 3, True, cfg)
    rep, fails, hist = got = hip.run_campaign(w, 9_000_000, 64 * BATCH, BATCH, 3, True, cfg, collect=64)
    assert rep.first_failing_seed != NONE and rep.seeds_run == rep.batches_run * BATCH < 64 * BATCH
    want, _ = oracle.run_batch(w, 9_000_000, int(rep.seeds_run), cfg)
    check(got, want, 9_000_000, 64, what="stop at failure")
    assert len(fails) >= 1 and fails["seed"][0] == rep.first_failing_seed and (fails["seed"] >= 9_000_000 + rep.seeds_run - BATCH).all()
    assert report(rep) == report(plain) and rep.batches_run <= rep.batches_launched <= rep.batches_run + 2


def test_runner_verdicts_are_counted_and_listed_only_on_request(hip):
    w = W.pingpong(4, 16)
    lim = A.Limits(); lim.heap_lds_slots, lim.heap_spill_slots = 2, 0          # a capacity nobody fits
    first, _ = hip.run_batch(w, 0, 3 * BATCH, None, lim)
    assert (first["verdict"] == A.OVERFLOW).all()
    plain = hip.run_campaign(w, 0, 3 * BATCH, BATCH, 2, True, None, lim)
    rep, fails, hist = got = hip.run_campaign(w, 0, 3 * BATCH, BATCH, 2, True, None, lim, collect=50)
    check(got, first, 0, 50, plain=plain, what="runner verdicts, not listed")
    assert len(fails) == 0 and hist[A.OVERFLOW] == 3 * BATCH == rep.n_runner and rep.first_failing_seed == NONE
    rep, fails, hist = got = hip.run_campaign(w, 0, 3 * BATCH, BATCH, 2, True, None, lim, collect=50, list_runner=True)
    check(got, first, 0, 50, list_runner=True, plain=plain, what="runner verdicts, listed")
    assert (fails["seed"] == np.arange(50)).all() and (fails["verdict"] == A.OVERFLOW).all()


def mixed_verdicts():
    """Two nodes: a client that sends a request, draws a bool and panics on `true` (5 %), then waits for the answer; a server that
    answers once.  On a 3 % lossy network either datagram can be lost: both tasks then wait forever."""
    wl = W.WorkloadBuilder()
    n1, n2 = wl.create_node(), wl.create_node()
    a1, a2 = wl.addr(n1, 1), wl.addr(n2, 1)
    t1 = wl.task(n1)
    t1.bind(a1).sleep(secs=1).send_to(a1, a2, 1, 7).rand_bool(0)
    skip = len(t1.code); t1.jeq(0, 0)
    t1.panic(3)
    t1.code[skip][2] = t1.label()
    t1.recv_from(a1, 1).assert_val(9).done()
    t2 = wl.task(n2)
    t2.bind(a2).recv_from(a2, 1).assert_val(7).reply(a2, 1, 9).done()
    wl.main().spawn(t1).spawn(t2).join(t1).join(t2).done()
    return wl.build(), A.Config.default(packet_loss_rate=0.03, loss_table=(0.05,))


def test_mixed_verdicts_are_told_apart(hip):
    w, cfg = mixed_verdicts()
    want, _ = oracle.run_batch(w, 0, 8192, cfg)
    kinds = np.bincount(want["verdict"], minlength=8)
    assert all(kinds[v] >= 82 for v in (A.PASS, A.PANIC, A.DEADLOCK)) and kinds.sum() == 8192, kinds        # each at least 1 % of the seeds
    for cap, batch in ((0, 1000), (300, 1000), (8192, 1000), (8192, 8192)):
        check(hip.run_campaign(w, 0, 8192, batch, 3, False, cfg, collect=cap), want, 0, cap,
              plain=hip.run_campaign(w, 0, 8192, batch, 3, False, cfg), what=("mixed", cap, batch))


@pytest.mark.parametrize("state", ["global", "lds"])
def test_an_extended_op_build(hip, state):
    """streaming_topology on a lossy network, per-seed state in global memory (the workload's own limits) and in LDS: the result array
    either build writes is read the same way.  Seeds the first pass answers with a runner verdict are counted, not listed."""
    w, cfg, lim = W.streaming_topology(), A.Config.default(packet_loss_rate=0.05), W.streaming_topology_limits()
    if state == "lds":
        lim.state_mem, lim.heap_lds_slots, lim.heap_spill_slots = A.STATE_LDS, 8, 184
    assert bool(hip.geometry(w, lim).variant & 16) == (state == "global")
    want, _ = oracle.run_batch(w, 1000, 4096, cfg, lim)
    assert int((want["verdict"] == A.PANIC).sum()) == 1884
    first, _ = hip.run_batch(w, 1000, 4096, cfg, lim)
    settled = first["verdict"] < A.OVERFLOW
    assert settled.sum() > 4000 and (first[settled] == want[settled]).all()
    check(hip.run_campaign(w, 1000, 4096, 1500, 2, False, cfg, lim, collect=2000), first, 1000, 2000,
          plain=hip.run_campaign(w, 1000, 4096, 1500, 2, False, cfg, lim), what=("streaming_topology", state))
