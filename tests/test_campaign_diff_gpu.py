"""Differential campaigns on the MI355X: madsim_hip_run_campaign_diff (and its context / several-contexts forms) against
tests/diff_ref.py's diff_truth over the CPU oracle's per-seed results of each side — never against a second call of the code under test.
The two-config range is the four-node ping-pong at loss 0 against loss 0.002 over 10 000 seeds: the oracle says 1 149 of them deadlock on
the lossy side (asserted below), and every one of those differs in every field but obs_hash."""
import copy

import numpy as np
import pytest

import oracle
from madsim_amd import _abi as A
from madsim_amd import workload as W
from tests import diff_ref as R
from tests import lifecycle_workloads as LW

pytestmark = pytest.mark.gpu

NONE = (1 << 64) - 1
SEED0, TOTAL, DEADLOCKS = R.SEED0, R.TOTAL, R.DEADLOCKS
REPORT_FIELDS = ("seeds_run", "batches_run", "batches_launched", "first_failing_seed", "n_failed", "n_runner", "total_steps", "total_clock_ns")


def report(rep, skip=()):
    return {f: int(getattr(rep, f)) for f in REPORT_FIELDS if f not in skip}


@pytest.fixture(scope="module")
def truth():
    """The precondition the file rests on, asserted on the oracle's results: side A passes everywhere, side B deadlocks DEADLOCKS times."""
    w, cfg_a, cfg_b, a, b = R.two_configs()
    assert (a["verdict"] == A.PASS).all() and int((b["verdict"] == A.DEADLOCK).sum()) == DEADLOCKS and set(b["verdict"].tolist()) == {A.PASS, A.DEADLOCK}
    t = R.diff_truth(a, b, SEED0, A.DIFF_ALL, 0)
    assert t["n_differ"] >= DEADLOCKS and t["n_by_field"][0] == DEADLOCKS and t["transitions"][A.PASS][A.DEADLOCK] == DEADLOCKS
    return w, cfg_a, cfg_b, a, b


def check(got, a, b, seed0, fields, cap, what):
    rep_a, rep_b, d = got
    want, have = R.diff_truth(a, b, seed0, fields, cap), R.of_report(d)
    print(what, "differ", have["n_differ"], want["n_differ"], "listed", have["n_listed"], want["n_listed"], "by field", have["n_by_field"], want["n_by_field"])
    assert have == want, what
    assert (d.fields, d.max_listed) == (fields, cap)
    t = d.transitions.astype(np.int64)
    assert int(t.sum()) == int(rep_a.seeds_run) == int(rep_b.seeds_run) == len(a)
    for rep, sums in ((rep_a, t.sum(axis=1)), (rep_b, t.sum(axis=0))):                      # the plain report of each side, seen in the matrix
        assert int(sums[1:4].sum()) == int(rep.n_failed) and int(sums[4:].sum()) == int(rep.n_runner)
    return d.records.tobytes()


def test_identity(hip, truth):
    """One workload on both sides, ALL: nothing differs, the matrix is diagonal and is collect's histogram, both reports are the plain one's."""
    w, _, cfg_b, _, b = truth
    for batch, in_flight in ((1000, 3), (4096, 1)):
        got = hip.run_campaign_diff(w, SEED0, TOTAL, config=cfg_b, max_listed=8, batch=batch, in_flight=in_flight)
        check(got, b, b, SEED0, A.DIFF_ALL, 8, ("identity", batch, in_flight))
        rep_a, rep_b, d = got
        assert d.n_differ == 0 and len(d) == 0 and d.n_compared == TOTAL
        _, _, hist = hip.run_campaign(w, SEED0, TOTAL, batch, in_flight, False, cfg_b, collect=0)
        assert (np.diag(d.transitions) == hist).all() and int(d.transitions.sum()) == int(np.trace(d.transitions)) == TOTAL
        plain = hip.run_campaign(w, SEED0, TOTAL, batch, in_flight, False, cfg_b)
        assert report(rep_a) == report(rep_b) == report(plain)
        assert rep_a.kernel_ms > 0 and rep_b.kernel_ms > 0


@pytest.mark.parametrize("name", ["kill_restart_with_traffic", "timeout_repeats_and_ties"])
def test_build_against_build(hip, name):
    """One workload under two state layouts, and with and without the 8-byte heap entries: the same 48 bytes for every seed."""
    w, cfg = getattr(LW, name)(), LW.config(name)
    total = 3000
    want, _ = oracle.run_batch(w, 1000, total, cfg or A.Config.default())

    def lim(state_mem):
        x = copy.copy(LW.limits(name) or A.Limits())
        x.state_mem, x.lanes_per_wave = state_mem, 0
        return x
    builds = {"lds": lim(A.STATE_LDS), "global": lim(A.STATE_GLOBAL), "narrow": lim(A.STATE_GLOBAL | A.STATE_NARROW_HEAP)}
    geo = {k: hip.geometry(w, v).variant for k, v in builds.items()}
    assert not geo["lds"] & 16 and geo["global"] & 16 and geo["narrow"] & 16 and geo["narrow"] & 0x8000 and not geo["global"] & 0x8000, geo
    for one, other in (("lds", "global"), ("global", "narrow")):
        rep_a, rep_b, d = hip.run_campaign_diff(w, 1000, total, config=cfg, limits=builds[one], other_limits=builds[other], max_listed=4, batch=1024)
        print(name, one, other, "differ", d.n_differ, "incomparable", d.n_incomparable, d.records)
        assert d.n_differ == 0 and len(d) == 0 and d.n_compared + d.n_incomparable == total
        assert report(rep_a) == report(rep_b)
        if d.n_incomparable == 0:                                                          # (no capacity verdict on either side: the oracle's matrix)
            check((rep_a, rep_b, d), want, want, 1000, A.DIFF_ALL, 4, (name, one, other))


def test_no_trace_hash(hip, truth):
    """no_trace_hash on one side: trace_hash comes back 0 there, and nothing else changes."""
    w, _, cfg_b, _, b = truth
    off = A.Limits()
    off.no_trace_hash = 1
    total = 5000
    rep_a, rep_b, d = hip.run_campaign_diff(w, SEED0, total, config=cfg_b, other_limits=off, fields=A.DIFF_ALL & ~A.DIFF_TRACE, max_listed=4, batch=2048)
    assert d.n_differ == 0 and d.n_compared == total and report(rep_a) == report(rep_b)
    zeroed = b[:total].copy()
    zeroed["trace_hash"] = 0
    got = hip.run_campaign_diff(w, SEED0, total, config=cfg_b, other_limits=off, max_listed=4, batch=2048)
    check(got, b[:total], zeroed, SEED0, A.DIFF_ALL, 4, "no trace hash")
    d = got[2]
    assert d.n_by_field[5] == d.n_compared == d.n_differ == total and int(d.n_by_field.sum()) == total


def test_two_configs_whatever_the_cut(hip, truth):
    """batch, batches in flight, one and two contexts: the whole struct is the truth, and the same bytes."""
    w, cfg_a, cfg_b, a, b = truth
    kw = dict(config=cfg_a, other_config=cfg_b)
    for fields, cap in ((A.DIFF_ALL, 64), (A.DIFF_VERDICT, DEADLOCKS + 10), (A.DIFF_OBS | A.DIFF_STEPS, 0)):
        first = None
        for batch in (1000, 4096):
            for in_flight in (1, 3):
                got = hip.run_campaign_diff(w, SEED0, TOTAL, fields=fields, max_listed=cap, batch=batch, in_flight=in_flight, **kw)
                recs = check(got, a, b, SEED0, fields, cap, (fields, cap, batch, in_flight))
                first = recs if first is None else first
                assert recs == first
                assert report(got[0]) == report(hip.run_campaign(w, SEED0, TOTAL, batch, in_flight, False, cfg_a))
                assert report(got[1]) == report(hip.run_campaign(w, SEED0, TOTAL, batch, in_flight, False, cfg_b))
        with hip.Context(0) as c0, hip.Context(0) as c1:
            got = c0.run_campaign_diff(w, SEED0, TOTAL, fields=fields, max_listed=cap, batch=1000, in_flight=3, **kw)
            assert check(got, a, b, SEED0, fields, cap, "context form") == first
            for ctxs in ([c0], [c0, c1]):
                for batch, in_flight in ((1000, 3), (4096, 1)):
                    got = hip.run_campaign_diff_multi(ctxs, w, SEED0, TOTAL, fields=fields, max_listed=cap, batch=batch, in_flight=in_flight, **kw)
                    assert check(got, a, b, SEED0, fields, cap, (len(ctxs), batch, in_flight)) == first
                    assert report(got[1]) == report(hip.run_campaign_multi(ctxs, w, SEED0, TOTAL, batch, in_flight, False, cfg_b))


@pytest.mark.parametrize("cap", [1, 3, 150])
def test_stop_at_diffs(hip, truth, cap):
    """"Show me `cap` seeds that changed": the campaign stops within the batches in flight, and everything it reports is the prefix's."""
    w, cfg_a, cfg_b, a, b = truth
    batch, in_flight = 1000, 3
    differs = np.nonzero(R.masks(a, b, A.DIFF_ALL))[0]
    stop_batch = int(differs[cap - 1]) // batch                                             # the batch that holds the cap-th differing seed
    assert stop_batch + 1 < TOTAL // batch
    with hip.Context(0) as c0, hip.Context(0) as c1:
        for ctxs in ([c0], [c0, c1]):
            got = hip.run_campaign_diff_multi(ctxs, w, SEED0, TOTAL, config=cfg_a, other_config=cfg_b, max_listed=cap, stop_at_diffs=True, batch=batch,
                                              in_flight=in_flight)
            rep_a, rep_b, d = got
            assert rep_a.seeds_run == rep_b.seeds_run == (stop_batch + 1) * batch and rep_a.batches_run == stop_batch + 1
            assert rep_a.batches_run <= rep_a.batches_launched <= rep_a.batches_run + len(ctxs) * (in_flight - 1) + (len(ctxs) - 1)
            n = int(rep_a.seeds_run)
            check(got, a[:n], b[:n], SEED0, A.DIFF_ALL, cap, ("stop at diffs", cap, len(ctxs)))
            assert len(d) == cap
            plain = hip.run_campaign_multi(ctxs, w, SEED0, n, batch, in_flight, False, cfg_b)     # the plain campaign over the same prefix
            assert report(rep_b, ("batches_launched",)) == report(plain, ("batches_launched",))
    # without the flag the same call runs to the end; the other stop flags mean nothing to this form
    rep_a, rep_b, d = hip.run_campaign_diff(w, SEED0, TOTAL, config=cfg_a, other_config=cfg_b, max_listed=cap, batch=batch, in_flight=in_flight)
    assert rep_a.seeds_run == TOTAL and len(d) == cap and d.n_differ == len(differs)


def test_small_ranges_and_argument_errors(hip, truth):
    w, cfg_a, cfg_b, a, b = truth
    kw = dict(config=cfg_a, other_config=cfg_b)
    first = int(np.nonzero(b["verdict"] == A.DEADLOCK)[0][0])
    for at, total in ((first, 1), (0, 1), (0, 65), (max(first - 3, 0), 700)):
        got = hip.run_campaign_diff(w, SEED0 + at, total, max_listed=4, **kw)                   # total < batch (the default batch)
        check(got, a[at:at + total], b[at:at + total], SEED0 + at, A.DIFF_ALL, 4, (at, total))
        assert report(got[1]) == report(hip.run_campaign(w, SEED0 + at, total, 0, 0, False, cfg_b))
    got = hip.run_campaign_diff(w, SEED0, 2500, max_listed=0, batch=1000, **kw)                  # cap = 0: the matrix and the counts only
    check(got, a[:2500], b[:2500], SEED0, A.DIFF_ALL, 0, "matrix only")
    rep_a, rep_b, d = hip.run_campaign_diff(w, SEED0, 0, max_listed=4, **kw)                      # no seeds: nothing
    assert (rep_a.seeds_run, rep_b.seeds_run, len(d), d.n_compared, int(d.transitions.sum())) == (0, 0, 0, 0, 0)
    # two different workloads: the sides need not share anything but the seeds
    other = W.pingpong(4, 15)
    wb, _ = oracle.run_batch(other, SEED0, 500, cfg_b)
    got = hip.run_campaign_diff(w, SEED0, 500, other=other, max_listed=500, batch=128, **kw)
    check(got, a[:500], wb, SEED0, A.DIFF_ALL, 500, "two workloads")
    # the errors that need a context to be reached by the mirror's own forms
    for bad in (dict(fields=0), dict(fields=128), dict(max_listed=0, stop_at_diffs=True), dict(in_flight=9)):
        with pytest.raises(hip.MadsimHipError):
            hip.run_campaign_diff(w, SEED0, 1000, **bad)
    with hip.Context(0) as c0:
        with pytest.raises(hip.MadsimHipError):
            hip.run_campaign_diff_multi([c0, c0], w, SEED0, 1000)                               # the same context twice
        with pytest.raises(hip.MadsimHipError):
            c0.run_campaign_diff(w, NONE - 5, 1000)                                             # seed0 + total wraps
