"""Failure-mode grouping on the MI355X: madsim_hip_run_campaign_groups (and its context / several-contexts forms) against
tests/groups_ref.py's groups_truth over the CPU oracle's per-seed results of the same range — never against a second call of the code under
test.  The range is the traced lossy two-pair ping-pong of examples/failure_modes_test.cpp (tests/groups_ref.py traced_pingpong): 20 000
seeds whose deadlocks come in three modes — pair 0 stuck, pair 1 stuck, both stuck — and whose passes in two (which pair finished first)."""
import numpy as np
import pytest

from madsim_amd import _abi as A
from tests import groups_ref as G
from tests import stats_ref as R

pytestmark = pytest.mark.gpu

NONE = (1 << 64) - 1
SEED0, TOTAL = G.SEED0, G.TOTAL
FAIL, EVERY = (A.PANIC, A.DEADLOCK, A.TIME_LIMIT), (A.PASS, A.PANIC, A.DEADLOCK, A.TIME_LIMIT)
REPORT_FIELDS = ("seeds_run", "batches_run", "batches_launched", "first_failing_seed", "n_failed", "n_runner", "total_steps", "total_clock_ns")


def report(rep):
    return {f: int(getattr(rep, f)) for f in REPORT_FIELDS}


def mask(include):
    return R.mask(*include)


@pytest.fixture(scope="module")
def truth():
    """The precondition the whole file rests on, asserted on the oracle's results: at least three groups over both PASS and DEADLOCK."""
    w, cfg, want = G.traced_pingpong()
    every = G.all_groups(want, SEED0, G.ALL, A.GROUP_KEY_OBS)
    assert len(every) >= 3 and {g[0] for g in every} >= {A.PASS, A.DEADLOCK}, every
    assert len(G.all_groups(want, SEED0, G.FAILURES, A.GROUP_KEY_OBS)) == 3
    assert len(G.all_groups(want, SEED0, G.ALL, A.GROUP_KEY_MSGS)) > 8                     # "msgs": many small groups, more than a short list holds
    return w, cfg, want


def check(groups, results, seed0, include, key, cap, what):
    want, got = G.groups_truth(results, seed0, mask(include), A.GROUP_KEY_NAMES.index(key), cap), G.of_report(groups)
    print(what, "groups", got["groups"][:4], "want", want["groups"][:4], "grouped", got["n_grouped"], want["n_grouped"], "ungrouped", got["n_ungrouped"],
          want["n_ungrouped"])
    assert got == want, what
    assert (groups.include, groups.key, groups.max_groups) == (mask(include), key, cap) and (groups.groups["reserved"] == 0).all()
    assert got["n_grouped"] + got["n_ungrouped"] == int(G.counted(results, mask(include)).sum())
    return groups.groups.tobytes()


@pytest.mark.parametrize("key", ["obs", "msgs"])
@pytest.mark.parametrize("include", [FAIL, EVERY])
def test_groups_are_the_oracles_whatever_the_cut(hip, truth, include, key):
    """batch (1 000: partial waves; 65 536: one batch for everything), batches in flight, the size of the list: the same groups, the same bytes."""
    w, cfg, want = truth
    for cap in (0, 1, 64):
        first = None
        for batch, in_flight in ((1000, 1), (1000, 3), (4096, 3), (65_536, 1)):
            rep, groups = hip.run_campaign_groups(w, SEED0, TOTAL, batch, in_flight, False, cfg, include=include, key=key, max_groups=cap)
            b = check(groups, want, SEED0, include, key, cap, (include, key, cap, batch, in_flight))
            first = b if first is None else first
            assert b == first
            assert report(rep) == report(hip.run_campaign(w, SEED0, TOTAL, batch, in_flight, False, cfg))
            assert len(groups) == min(cap, len(G.all_groups(want, SEED0, mask(include), A.GROUP_KEY_NAMES.index(key))))


def test_one_two_and_three_contexts(hip, truth):
    w, cfg, want = truth
    with hip.Context(0) as c0, hip.Context(0) as c1, hip.Context(0) as c2:
        rep, groups = c0.run_campaign_groups(w, SEED0, TOTAL, 4096, 3, False, cfg, max_groups=8)
        first = check(groups, want, SEED0, FAIL, "obs", 8, "context form")
        assert report(rep) == report(c0.run_campaign(w, SEED0, TOTAL, 4096, 3, False, cfg))
        for ctxs in ([c0], [c0, c1], [c0, c1, c2]):
            for batch, in_flight in ((1000, 3), (4096, 1)):
                rep, groups = hip.run_campaign_groups_multi(ctxs, w, SEED0, TOTAL, batch, in_flight, False, cfg, max_groups=8)
                assert check(groups, want, SEED0, FAIL, "obs", 8, (len(ctxs), batch, in_flight)) == first
                assert report(rep) == report(hip.run_campaign_multi(ctxs, w, SEED0, TOTAL, batch, in_flight, False, cfg))
            rep, groups = hip.run_campaign_groups_multi(ctxs, w, SEED0, TOTAL, 1000, 2, False, cfg, include=EVERY, key="msgs", max_groups=5)
            check(groups, want, SEED0, EVERY, "msgs", 5, (len(ctxs), "msgs"))


def test_stop_at_groups(hip, truth):
    """"Find me two different failures": the campaign stops within the batches in flight, and everything it reports is the prefix's."""
    w, cfg, want = truth
    batch, in_flight = 1000, 3
    dead = G.all_groups(want, SEED0, G.FAILURES, A.GROUP_KEY_OBS)
    stop_batch = (dead[1][3] - SEED0) // batch                                               # the batch that holds the second mode's first seed
    assert stop_batch + 1 < TOTAL // batch
    rep, groups = hip.run_campaign_groups(w, SEED0, TOTAL, batch, in_flight, False, cfg, max_groups=2, stop_at_groups=True)
    assert rep.seeds_run == (stop_batch + 1) * batch and rep.batches_run == stop_batch + 1
    assert rep.batches_run <= rep.batches_launched <= rep.batches_run + in_flight - 1
    prefix = want[:rep.seeds_run]
    check(groups, prefix, SEED0, FAIL, "obs", 2, "stop at groups")
    assert len(groups) == 2
    plain = hip.run_campaign(w, SEED0, int(rep.seeds_run), batch, in_flight, False, cfg)       # the plain campaign over the same prefix
    assert {f: v for f, v in report(rep).items() if f != "batches_launched"} == {f: v for f, v in report(plain).items() if f != "batches_launched"}
    # without the flag the same call runs to the end; the plain entry points ignore the flag's bit
    rep, groups = hip.run_campaign_groups(w, SEED0, TOTAL, batch, in_flight, False, cfg, max_groups=2)
    assert rep.seeds_run == TOTAL and len(groups) == 2
    # combined with STOP_AT_FAILURE: the first failing batch stops it, one mode found so far
    rep, groups = hip.run_campaign_groups(w, SEED0, TOTAL, batch, in_flight, True, cfg, max_groups=2, stop_at_groups=True)
    plain = hip.run_campaign(w, SEED0, TOTAL, batch, in_flight, True, cfg)
    assert report(rep)["seeds_run"] == report(plain)["seeds_run"] == ((dead[0][3] - SEED0) // batch + 1) * batch
    assert {f: v for f, v in report(rep).items() if f != "batches_launched"} == {f: v for f, v in report(plain).items() if f != "batches_launched"}
    check(groups, want[:rep.seeds_run], SEED0, FAIL, "obs", 2, "stop at failure and groups")
    assert 1 <= len(groups) <= 2


def test_the_whole_triage_report_in_one_call(hip, truth):
    """With a collect list and statistics given, all three outputs equal those of the three separate calls."""
    w, cfg, want = truth
    crep, cfails, chist = hip.run_campaign(w, SEED0, TOTAL, 4096, 3, False, cfg, collect=100)
    srep, sstats = hip.run_campaign_stats(w, SEED0, TOTAL, 4096, 3, False, cfg, include=(A.PASS,), top_k=16)
    grep, ggroups = hip.run_campaign_groups(w, SEED0, TOTAL, 4096, 3, False, cfg, max_groups=8)
    rep, fails, hist, stats, groups = hip.run_campaign_groups(w, SEED0, TOTAL, 4096, 3, False, cfg, max_groups=8, collect=100, stats=((A.PASS,), 16))
    assert report(rep) == report(crep) == report(srep) == report(grep)
    assert fails.tobytes() == cfails.tobytes() and len(fails) == 100 and (hist == chist).all() and (hist == np.bincount(want["verdict"], minlength=8)).all()
    assert R.same(R.of_stats(stats), R.of_stats(sstats)) and R.same(R.of_stats(stats), R.stats_truth(want, SEED0, R.mask(A.PASS), 16))
    assert groups.groups.tobytes() == ggroups.groups.tobytes()
    check(groups, want, SEED0, FAIL, "obs", 8, "all three")
    # statistics without extreme seeds (their words are then not part of the report), and statistics alone
    rep, stats, groups = hip.run_campaign_groups(w, SEED0, TOTAL, 1000, 2, False, cfg, include=EVERY, max_groups=8, stats=((A.PASS, A.DEADLOCK), 0))
    assert R.same(R.of_stats(stats), R.stats_truth(want, SEED0, R.mask(A.PASS, A.DEADLOCK), 0))
    check(groups, want, SEED0, EVERY, "obs", 8, "with statistics")
    rep, fails, hist, groups = hip.run_campaign_groups(w, SEED0, TOTAL, 1000, 2, False, cfg, max_groups=1, collect=0)
    assert len(fails) == 0 and (hist == chist).all()
    check(groups, want, SEED0, FAIL, "obs", 1, "with a histogram")


def test_small_campaigns_and_argument_errors(hip, truth):
    w, cfg, want = truth
    dead = int(np.nonzero(want["verdict"] == A.DEADLOCK)[0][0])
    for seed0, total in ((SEED0 + dead, 1), (SEED0, 1), (SEED0, 65)):
        rep, groups = hip.run_campaign_groups(w, seed0, total, 0, 0, False, cfg, include=EVERY, max_groups=4)
        check(groups, want[seed0 - SEED0:seed0 - SEED0 + total], seed0, EVERY, "obs", 4, (seed0, total))
        assert report(rep) == report(hip.run_campaign(w, seed0, total, 0, 0, False, cfg))
    rep, groups = hip.run_campaign_groups(w, SEED0, 0, max_groups=4)                          # no seeds: no groups
    assert (rep.seeds_run, len(groups), groups.n_grouped, groups.n_ungrouped) == (0, 0, 0, 0)
    # the errors that need a context to be reached by the mirror's own forms
    for kw in (dict(include=()), dict(include=(A.OVERFLOW,)), dict(key="pc"), dict(max_groups=0, stop_at_groups=True), dict(in_flight=9),
               dict(batch=(1 << 20) + 1), dict(collect=0, stop_at_cap=True), dict(stats=((A.PASS,), 17))):
        with pytest.raises(hip.MadsimHipError):
            hip.run_campaign_groups(w, SEED0, 1 << 21, **kw)
    with hip.Context(0) as c0:
        with pytest.raises(hip.MadsimHipError):
            hip.run_campaign_groups_multi([c0, c0], w, SEED0, 1000, max_groups=4)             # the same context twice
        with pytest.raises(hip.MadsimHipError):
            c0.run_campaign_groups(w, NONE - 5, 1000, max_groups=4)                           # seed0 + total wraps
