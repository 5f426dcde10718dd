"""Campaign statistics on the MI355X: madsim_hip_run_campaign_stats (and its context / several-contexts forms) against
tests/stats_ref.py's stats_truth over the CPU oracle's per-seed results of the same range — never against a second call of the code under
test.  All tests but the edge-value and extended-op ones use the lossy ping-pong range of tests/test_collect_gpu.py: among its 35 330
passing seeds clock_ns has 35 315 distinct values (no tie in the top 16), steps is 402 or 403 (17 722 seeds tie at the maximum: the top 16
are the 16 smallest seeds of those, and more than a thousand tie at the 16th place of every 4 096-seed batch), msg_count is 64 everywhere
(a total tie) and rng_calls has 183 values over two octaves; with the deadlocked seeds counted too, rng_calls spans bit lengths 7-11 and
msg_count 2-7."""
import numpy as np
import pytest

import oracle
from madsim_amd import _abi as A
from madsim_amd import workload as W
from tests import stats_ref as R

pytestmark = pytest.mark.gpu

NONE = (1 << 64) - 1
SEED0, TOTAL, BATCH = R.SEED0, R.TOTAL, 4096
PASS, DEADLOCK = R.mask(A.PASS), R.mask(A.DEADLOCK)
ALL = R.mask(A.PASS, A.PANIC, A.DEADLOCK, A.TIME_LIMIT)
REPORT_FIELDS = ("seeds_run", "batches_run", "batches_launched", "first_failing_seed", "n_failed", "n_runner", "total_steps", "total_clock_ns")


def report(rep):
    return {f: int(getattr(rep, f)) for f in REPORT_FIELDS}


def verdicts(include):
    return tuple(v for v in range(4) if include >> v & 1)


def check(stats, results, seed0, include, top_k, what=None):
    """Every field of a CampaignStats against the truth over `results`; returns the bytes that must not depend on the cut."""
    want, got = R.stats_truth(results, seed0, include, top_k), R.of_stats(stats)
    assert (got["n"], got["n_top"]) == (want["n"], want["n_top"]), (what, got["n"], want["n"], got["n_top"])
    assert (stats.include, stats.top_k) == (include, top_k)
    for name in R.METRICS:
        g, w = got[name], want[name]
        print(what, name, "n", got["n"], "min/max/sum", g["min"], g["max"], g["sum"], "want", w["min"], w["max"], w["sum"], "top", g["top"][:3], w["top"][:3])
        assert (g["min"], g["max"], g["sum"]) == (w["min"], w["max"], w["sum"]), (what, name)
        assert g["hist"].dtype == np.uint64 and (g["hist"] == w["hist"]).all(), (what, name, np.nonzero(g["hist"] != w["hist"])[0][:8])
        assert g["top"] == w["top"], (what, name, g["top"], w["top"])
        assert stats.top(name).dtype == np.dtype(A.EXTREME_DTYPE) and len(stats.top(name)) == want["n_top"]
        if want["n"]:
            assert stats.mean[name] == w["sum"] / want["n"] and stats.quantile(name, 0.5) == R.quantile_bounds(want, name, 0.5)
    return as_bytes(stats)


def as_bytes(stats):
    return b"".join([np.array([stats.n, stats.n_top], dtype=np.uint64).tobytes()] + [
        np.array([stats.min[m], stats.max[m], stats.sum[m] & NONE, stats.sum[m] >> 64], dtype=np.uint64).tobytes() + stats.hist[m].tobytes()
        + stats.top(m).tobytes() for m in R.METRICS])


@pytest.mark.parametrize("top_k", [0, 1, 16])
@pytest.mark.parametrize("include", [PASS, DEADLOCK, ALL])
def test_statistics_are_the_oracles(hip, include, top_k):
    w, cfg, want = R.lossy_pingpong()
    plain = hip.run_campaign(w, SEED0, TOTAL, BATCH, 3, False, cfg)
    rep, stats = hip.run_campaign_stats(w, SEED0, TOTAL, BATCH, 3, False, cfg, include=verdicts(include), top_k=top_k)
    check(stats, want, SEED0, include, top_k, what=(include, top_k))
    assert stats.n == {PASS: 35_330, DEADLOCK: 4_670, ALL: 40_000}[include]
    assert report(rep) == report(plain) and (rep.batches_run, rep.batches_launched) == (10, 10)


def test_the_cut_does_not_matter(hip):
    """batch (100: partial waves; one batch for everything: four 64-seed rounds per wave), batches in flight, one context or two, run to
    run: the same bytes."""
    w, cfg, want = R.lossy_pingpong()
    first = None
    for batch, in_flight in ((100, 1), (100, 8), (4096, 3), (40_000, 1), (40_000, 1), (40_000, 1)):
        rep, stats = hip.run_campaign_stats(w, SEED0, TOTAL, batch, in_flight, False, cfg, top_k=16)
        b = check(stats, want, SEED0, PASS, 16, what=(batch, in_flight))
        first = first or b
        assert b == first and report(rep) == report(hip.run_campaign(w, SEED0, TOTAL, batch, in_flight, False, cfg)), (batch, in_flight)
    with hip.Context(0) as c0, hip.Context(0) as c1:
        for batch, in_flight in ((100, 3), (4096, 2)):
            rep, stats = hip.run_campaign_stats_multi([c0, c1], w, SEED0, TOTAL, batch, in_flight, False, cfg, top_k=16)
            assert check(stats, want, SEED0, PASS, 16, what=("two contexts", batch)) == first
            assert report(rep) == report(hip.run_campaign_multi([c0, c1], w, SEED0, TOTAL, batch, in_flight, False, cfg))
        rep, stats = c0.run_campaign_stats(w, SEED0, TOTAL, BATCH, 3, False, cfg, top_k=16)
        assert check(stats, want, SEED0, PASS, 16, what="context form") == first
    # the smallest campaigns: one seed (a failing one: nothing counted; a passing one), one batch of a wave and one lane
    assert want["verdict"][4] != A.PASS and want["verdict"][0] == A.PASS
    for seed0, total in ((SEED0 + 4, 1), (SEED0, 1), (SEED0, 65)):
        rep, stats = hip.run_campaign_stats(w, seed0, total, 0, 0, False, cfg, top_k=16)
        check(stats, want[seed0 - SEED0:seed0 - SEED0 + total], seed0, PASS, 16, what=(seed0, total))
        assert report(rep) == report(hip.run_campaign(w, seed0, total, 0, 0, False, cfg))
        if total == 1:
            assert stats.n == stats.n_top == (0 if seed0 == SEED0 + 4 else 1)
            assert seed0 == SEED0 or all(stats.min[m] == NONE and stats.max[m] == 0 and stats.sum[m] == 0 for m in R.METRICS)


def test_with_a_collect_list(hip):
    w, cfg, want = R.lossy_pingpong()
    crep, cfails, chist = hip.run_campaign(w, SEED0, TOTAL, BATCH, 3, False, cfg, collect=1000)
    rep, fails, hist, stats = hip.run_campaign_stats(w, SEED0, TOTAL, BATCH, 3, False, cfg, top_k=16, collect=1000)
    b = check(stats, want, SEED0, PASS, 16, what="with collect")
    assert report(rep) == report(crep) and fails.tobytes() == cfails.tobytes() and len(fails) == 1000 and (hist == chist).all()
    assert (hist == np.bincount(want["verdict"], minlength=8)).all()
    assert b == as_bytes(hip.run_campaign_stats(w, SEED0, TOTAL, BATCH, 3, False, cfg, top_k=16)[1])
    # STOP_AT_CAP stops the statistics where it stops the list
    rep, fails, hist, stats = hip.run_campaign_stats(w, SEED0, TOTAL, BATCH, 3, False, cfg, top_k=16, collect=600, stop_at_cap=True)
    assert rep.seeds_run == 2 * BATCH and len(fails) == 600
    check(stats, want[:rep.seeds_run], SEED0, PASS, 16, what="stop at cap")


def test_early_stop_counts_the_prefix(hip):
    """The rare-failure setting of the campaign tests: the statistics are those of exactly rep.seeds_run seeds."""
    w, cfg = W.pingpong(4, 16), A.Config.default(packet_loss_rate=0.000002)
    plain = hip.run_campaign(w, 9_000_000, 64 * BATCH, BATCH, 3, True, cfg)
    rep, stats = hip.run_campaign_stats(w, 9_000_000, 64 * BATCH, BATCH, 3, True, cfg, include=(A.PASS, A.DEADLOCK), top_k=16)
    assert rep.first_failing_seed != NONE and rep.seeds_run == rep.batches_run * BATCH < 64 * BATCH
    assert report(rep) == report(plain) and rep.batches_run <= rep.batches_launched <= rep.batches_run + 2
    want, _ = oracle.run_batch(w, 9_000_000, int(rep.seeds_run), cfg)
    check(stats, want, 9_000_000, PASS | DEADLOCK, 16, what="stop at failure")
    assert stats.n == rep.seeds_run


def test_runner_verdicts_are_never_counted(hip):
    w = W.pingpong(4, 16)
    lim = A.Limits(); lim.heap_lds_slots, lim.heap_spill_slots = 2, 0          # a capacity nobody fits: every seed MADSIM_OVERFLOW
    first, _ = hip.run_batch(w, 0, 2 * BATCH, None, lim)
    assert (first["verdict"] == A.OVERFLOW).all()
    for include in range(1, 16):
        rep, stats = hip.run_campaign_stats(w, 0, 2 * BATCH, BATCH, 2, False, None, lim, include=verdicts(include), top_k=16)
        assert stats.n == stats.n_top == 0 and rep.n_runner == 2 * BATCH, include
        check(stats, first, 0, include, 16, what=("overflow", include))
    for bad in ((A.OVERFLOW,), (A.PASS, A.STEP_LIMIT), ()):
        with pytest.raises(hip.MadsimHipError):
            hip.run_campaign_stats(w, 0, BATCH, include=bad)


def test_edge_values(hip):
    """One task: a randomised sleep, then 5 s.  clock_ns >= 2^32 (the high half-sum, buckets above 128), msg_count = 0 (bucket 0)."""
    wl = W.WorkloadBuilder()
    wl.main().sleep_rand(0, secs=10).sleep(secs=5).done()          # 5 s .. 15 s: past 2^33 ns, bucket 128
    w = wl.build()
    want, _ = oracle.run_batch(w, 77, 4096)
    assert (want["verdict"] == A.PASS).all() and want["clock_ns"].min() >= 1 << 32 and (want["msg_count"] == 0).all()
    assert len(set(want["clock_ns"].tolist())) > 4000 and R.bucket(int(want["clock_ns"].max())) > 128
    for batch in (4096, 1000):
        rep, stats = hip.run_campaign_stats(w, 77, 4096, batch, 2, top_k=16)
        check(stats, want, 77, PASS, 16, what=("edge", batch))
        assert stats.sum["clock_ns"] > 4096 << 32 and stats.hist["msg_count"][0] == 4096 and stats.max["msg_count"] == 0
        assert report(rep) == report(hip.run_campaign(w, 77, 4096, batch, 2))


def test_an_extended_op_build(hip):
    """streaming_topology with its state in global memory: the reduction reads the result array whichever kernel build filled it.  Truth:
    the oracle, for the seeds the first pass settles; seeds it answers with a runner verdict are not counted (run_batch's verdicts)."""
    w, cfg, lim = W.streaming_topology(), A.Config.default(packet_loss_rate=0.05), W.streaming_topology_limits()
    assert hip.geometry(w, lim).variant & 16
    want, _ = oracle.run_batch(w, 1000, 4096, cfg, lim)
    first, _ = hip.run_batch(w, 1000, 4096, cfg, lim)
    settled = first["verdict"] < A.OVERFLOW
    assert settled.sum() > 4000 and (first[settled] == want[settled]).all()
    truth = want.copy()
    truth[~settled] = first[~settled]
    rep, stats = hip.run_campaign_stats(w, 1000, 4096, 1500, 2, False, cfg, lim, include=(A.PASS, A.PANIC), top_k=16)
    check(stats, truth, 1000, R.mask(A.PASS, A.PANIC), 16, what="streaming_topology")
    assert stats.n > 3000 and report(rep) == report(hip.run_campaign(w, 1000, 4096, 1500, 2, False, cfg, lim))
