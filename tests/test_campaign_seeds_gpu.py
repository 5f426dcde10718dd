"""List campaigns on the MI355X: madsim_hip_run_seeds_campaign and madsim_hip_run_seeds_campaign_diff (and their context / several-contexts
forms) against tests/seedlist_ref.py over the CPU oracle's per-seed results of every listed seed — never against a second call of the code
under test, except where the issue is identity with the range entry point, and then the truth is held too.  The range is
tests/test_collect_gpu.py's lossy four-node ping-pong: 40 000 seeds from 5 000 000, 4 670 of them deadlock (asserted there against the
oracle, cached); seeds outside it get one oracle call each."""
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import oracle
from madsim_amd import _abi as A
from tests import diff_ref as D
from tests import groups_ref as G
from tests import seedlist_ref as S
from tests import stats_ref as R
from tests.test_campaign_resolve_gpu import account, account_truth, jittery, JSEED0, JTOTAL
from tests.test_collect_gpu import SEED0, TOTAL, lossy_pingpong

pytestmark = pytest.mark.gpu

NONE = (1 << 64) - 1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BATCH = 1024
FIELDS = ("seeds_run", "batches_run", "batches_launched", "first_failing_seed", "n_failed", "n_runner", "total_steps", "total_clock_ns")
STATS = ((A.PASS, A.DEADLOCK), 16)
STATS_MASK = R.mask(A.PASS, A.DEADLOCK)
GROUPS = ((A.PANIC, A.DEADLOCK, A.TIME_LIMIT), "trace", 64)                 # by trace_hash: nearly every deadlock is a group of its own
GROUPS_MASK = G.FAILURES


def report(rep, skip=()):
    return {f: int(getattr(rep, f)) for f in FIELDS if f not in skip}


@functools.lru_cache(maxsize=None)
def fixed_side():
    """The oracle's results of the range on a network that loses nothing (side B of the diffs): every seed passes."""
    w, _, _ = lossy_pingpong()
    b, _ = oracle.run_batch(w, SEED0, TOTAL, A.Config.default())
    assert (b["verdict"] == A.PASS).all()
    b.setflags(write=False)
    return b


def results_of(seeds, side_b=False):
    """The oracle's per-seed results of a list: the cached range indexed by seeds - SEED0, one oracle call per seed outside it."""
    w, cfg, want = lossy_pingpong()
    src, cfg = (fixed_side(), A.Config.default()) if side_b else (want, cfg)
    out = np.zeros(len(seeds), dtype=A.RESULT_DTYPE)
    for i, s in enumerate(int(x) for x in seeds):
        out[i] = src[s - SEED0] if SEED0 <= s < SEED0 + TOTAL else oracle.run_batch(w, s, 1, cfg)[0][0]
    return out


def failing_seeds():
    _, _, want = lossy_pingpong()
    return np.uint64(SEED0) + np.nonzero(want["verdict"] != A.PASS)[0].astype(np.uint64)


def mixed_list():
    """Every third seed of the range, united with the failing seeds."""
    return np.union1d(np.uint64(SEED0) + np.arange(0, TOTAL, 3, dtype=np.uint64), failing_seeds())


def check_all(hip, seeds, res_a, res_b, got, cap, diff_cap, batch, what):
    """`got` = (campaign, failures, by_verdict, CampaignStats, CampaignGroups) and (campaign A, campaign B, CampaignDiff) of one list, whole."""
    (rep, fails, hist, st, grp), (rep_a, rep_b, d) = got
    n = len(seeds)
    for r, res in ((rep, res_a), (rep_a, res_a), (rep_b, res_b)):
        assert S.of_campaign(r) == S.campaign_truth(res, seeds), (what, S.of_campaign(r), S.campaign_truth(res, seeds))
        assert r.batches_run == (n + batch - 1) // batch == r.batches_launched, (what, r.batches_run, r.batches_launched)
    words, rec_bytes = S.collect_truth(res_a, seeds, cap, 0)
    assert fails.tobytes() == rec_bytes and [int(x) for x in hist] == [int(x) for x in words[6:14]], (what, "collect", len(fails), hist)
    assert R.same(R.of_stats(st), S.stats_truth(res_a, seeds, STATS_MASK, STATS[1])), (what, "statistics")
    assert G.of_report(grp) == S.groups_truth(res_a, seeds, GROUPS_MASK, A.GROUP_KEY_TRACE, GROUPS[2]), (what, "groups", len(grp))
    assert D.of_report(d) == S.diff_truth(res_a, res_b, seeds, A.DIFF_ALL, diff_cap), (what, "diff", d.n_differ)
    return fails.tobytes() + hist.tobytes() + repr(R.of_stats(st)).encode() + repr(G.of_report(grp)).encode() + repr(D.of_report(d)).encode()


def run_all(hip, seeds, cap, diff_cap, batch, in_flight, ctxs=None):
    w, cfg, _ = lossy_pingpong()
    kw = dict(batch=batch, in_flight=in_flight, config=cfg)
    if ctxs is None:
        return (hip.run_campaign_seeds(w, seeds, collect=cap, stats=STATS, groups=GROUPS, **kw),
                hip.run_campaign_diff_seeds(w, seeds, other_config=A.Config.default(), max_listed=diff_cap, **kw))
    return (hip.run_campaign_seeds_multi(ctxs, w, seeds, collect=cap, stats=STATS, groups=GROUPS, **kw),
            hip.run_campaign_diff_seeds_multi(ctxs, w, seeds, other_config=A.Config.default(), max_listed=diff_cap, **kw))


# ---- identity ------------------------------------------------------------------------------------------------------------------------
def test_a_dense_list_is_the_range(hip):
    """seeds = SEED0 .. SEED0 + 2 999 in batches of 1 024 (the last holds 952): every integer field and every record of the plain form,
    collect, statistics, groups and diff equals the range entry point's — and the truth's."""
    w, cfg, want = lossy_pingpong()
    n = 3000
    seeds = np.arange(SEED0, SEED0 + n, dtype=np.uint64)
    res_a, res_b = want[:n], fixed_side()[:n]
    kw = dict(batch=BATCH, in_flight=3, config=cfg)
    plain = hip.run_campaign_seeds(w, seeds, **kw)
    assert report(plain) == report(hip.run_campaign(w, SEED0, n, BATCH, 3, False, cfg)) and (plain.batches_run, plain.seeds_run) == (3, n)
    assert S.of_campaign(plain) == S.campaign_truth(res_a, seeds)
    got = hip.run_campaign_seeds(w, seeds, collect=100, stats=STATS, groups=GROUPS, **kw)
    rng = hip.run_campaign_groups(w, SEED0, n, BATCH, 3, False, cfg, include=GROUPS[0], key=GROUPS[1], max_groups=GROUPS[2], collect=100, stats=STATS)
    assert report(got[0]) == report(rng[0]) == report(plain)
    assert got[1].tobytes() == rng[1].tobytes() and len(got[1]) == 100 and got[2].tobytes() == rng[2].tobytes()
    assert R.same(R.of_stats(got[3]), R.of_stats(rng[3])) and got[3].n_top == 16
    assert got[4].groups.tobytes() == rng[4].groups.tobytes() and (got[4].n_grouped, got[4].n_ungrouped) == (rng[4].n_grouped, rng[4].n_ungrouped)
    assert len(got[4]) == 64 and got[4].n_ungrouped > 0                                        # many groups: the list is full
    # each part alone is the range's own entry point
    alone = hip.run_campaign_seeds(w, seeds, collect=100, **kw)
    ranged = hip.run_campaign(w, SEED0, n, BATCH, 3, False, cfg, collect=100)
    assert report(alone[0]) == report(ranged[0]) and alone[1].tobytes() == ranged[1].tobytes() and alone[2].tobytes() == ranged[2].tobytes()
    alone = hip.run_campaign_seeds(w, seeds, stats=STATS, **kw)
    assert R.same(R.of_stats(alone[1]), R.of_stats(hip.run_campaign_stats(w, SEED0, n, BATCH, 3, False, cfg, include=STATS[0], top_k=16)[1]))
    dl = hip.run_campaign_diff_seeds(w, seeds, other_config=A.Config.default(), max_listed=100, **kw)
    dr = hip.run_campaign_diff(w, SEED0, n, config=cfg, other_config=A.Config.default(), max_listed=100, batch=BATCH, in_flight=3)
    assert report(dl[0]) == report(dr[0]) and report(dl[1]) == report(dr[1]) and D.of_report(dl[2]) == D.of_report(dr[2]) and len(dl[2]) == 100
    check_all(hip, seeds, res_a, res_b, (got, dl), 100, 100, BATCH, "dense")


# ---- the corpus ------------------------------------------------------------------------------------------------------------------------
def test_the_corpus_of_failing_seeds(hip):
    """The list is exactly the 4 670 failing seeds: every one deadlocks, the collect list is the oracle's records in order, and against a
    network that loses nothing every one goes from deadlock to pass."""
    seeds = failing_seeds()
    assert len(seeds) == 4670
    res_a, res_b = results_of(seeds), results_of(seeds, side_b=True)
    got = run_all(hip, seeds, 8192, 8192, BATCH, 3)
    check_all(hip, seeds, res_a, res_b, got, 8192, 8192, BATCH, "corpus")
    (rep, fails, hist, st, grp), (rep_a, rep_b, d) = got
    assert int(hist[A.DEADLOCK]) == 4670 == rep.n_failed == rep.seeds_run and rep.first_failing_seed == SEED0 + 4
    assert (fails["seed"] == seeds).all() and len(fails) == 4670
    assert int(d.transitions[A.DEADLOCK][A.PASS]) == 4670 == d.n_differ == len(d) and int(d.transitions.sum()) == 4670
    assert (d.records["seed"] == seeds).all() and rep_b.n_failed == 0 and rep_a.n_failed == 4670
    assert st.n == 4670 and st.hist["steps"].sum() == 4670


# ---- mixed and scattered ---------------------------------------------------------------------------------------------------------------
def test_a_mixed_list(hip):
    seeds = mixed_list()
    assert len(seeds) > 13_334 and (np.diff(seeds.astype(np.int64)) > 0).all()
    res_a, res_b = results_of(seeds), results_of(seeds, side_b=True)
    check_all(hip, seeds, res_a, res_b, run_all(hip, seeds, 300, 50, BATCH, 3), 300, 50, BATCH, "mixed")


def test_six_scattered_seeds(hip):
    """0, 1, 2^32, 2^63, 2^64 - 1 and a failing seed of the range in one call with batch = 4: a partial wave, and two batches."""
    seeds = np.array(sorted([0, 1, 1 << 32, 1 << 63, NONE, SEED0 + 4]), dtype=np.uint64)
    res_a, res_b = results_of(seeds), results_of(seeds, side_b=True)
    assert res_a["verdict"][int(np.nonzero(seeds == np.uint64(SEED0 + 4))[0][0])] == A.DEADLOCK and int(seeds[-1]) == NONE
    got = run_all(hip, seeds, 6, 6, 4, 2)
    check_all(hip, seeds, res_a, res_b, got, 6, 6, 4, "scattered")
    assert got[0][0].batches_run == 2 and got[0][0].first_failing_seed == min(int(s) for s, r in zip(seeds, res_a) if r["verdict"] != A.PASS)
    top = got[0][3].top("clock_ns")
    assert len(top) == 6 and set(int(s) for s in top["seed"]) == set(int(s) for s in seeds)      # every seed whole: bit 63, 2^64 - 1, 2^32


# ---- the cut does not matter -----------------------------------------------------------------------------------------------------------
def test_the_cut_does_not_matter(hip):
    seeds = mixed_list()[:5000]
    n = len(seeds)
    res_a, res_b = results_of(seeds), results_of(seeds, side_b=True)
    first = None
    for batch, in_flight in ((100, 1), (100, 8), (1024, 3), (n, 1)):
        b = check_all(hip, seeds, res_a, res_b, run_all(hip, seeds, 200, 40, batch, in_flight), 200, 40, batch, (batch, in_flight))
        first = b if first is None else first
        assert b == first, (batch, in_flight)
    with hip.Context(0) as c0, hip.Context(0) as c1:
        assert check_all(hip, seeds, res_a, res_b, run_all(hip, seeds, 200, 40, 100, 2, [c0, c1]), 200, 40, 100, "two contexts") == first
        w, cfg, _ = lossy_pingpong()
        one = (c0.run_campaign_seeds(w, seeds, collect=200, stats=STATS, groups=GROUPS, batch=1024, in_flight=2, config=cfg),
               c0.run_campaign_diff_seeds(w, seeds, other_config=A.Config.default(), max_listed=40, batch=1024, in_flight=2, config=cfg))
        assert check_all(hip, seeds, res_a, res_b, one, 200, 40, 1024, "context form") == first
    for s in (SEED0 + 4, SEED0):                                                             # n = 1: a failing seed, a passing seed
        one = np.array([s], dtype=np.uint64)
        check_all(hip, one, results_of(one), results_of(one, side_b=True), run_all(hip, one, 4, 4, 0, 0), 4, 4, 65536, ("n = 1", s))


# ---- stop rules ------------------------------------------------------------------------------------------------------------------------
def test_stop_rules_on_the_mixed_list(hip):
    """Each stop flag: seeds_run is a whole number of batches, the reports are the truth of seeds[0 .. seeds_run), batches_launched lies within
    the bounds of the range forms (the batches in flight when the stopping one was read)."""
    w, cfg, _ = lossy_pingpong()
    seeds = mixed_list()
    res = results_of(seeds)
    batch, in_flight = 512, 3
    kw = dict(batch=batch, in_flight=in_flight, config=cfg)
    failing = np.nonzero(res["verdict"] != A.PASS)[0]

    def prefix(rep, stop_batch, what):
        run = (stop_batch + 1) * batch
        assert rep.seeds_run == run and rep.batches_run == stop_batch + 1 and run % batch == 0, (what, rep.seeds_run, run)
        assert rep.batches_run <= rep.batches_launched <= rep.batches_run + in_flight - 1, (what, rep.batches_launched)
        assert S.of_campaign(rep) == S.campaign_truth(res[:run], seeds[:run]), what
        return run

    rep = hip.run_campaign_seeds(w, seeds, stop_at_failure=True, **kw)
    prefix(rep, int(failing[0]) // batch, "stop at failure")
    assert rep.first_failing_seed == int(seeds[failing[0]])
    later = seeds[int(failing[0]) + 1:]                                                       # ... and from behind the first failure: the next one
    rep = hip.run_campaign_seeds(w, later, stop_at_failure=True, **kw)
    assert rep.first_failing_seed == int(seeds[failing[1]]) and rep.seeds_run == (int(failing[1] - failing[0] - 1) // batch + 1) * batch
    cap = 150
    rep, fails, hist = hip.run_campaign_seeds(w, seeds, collect=cap, stop_at_cap=True, **kw)
    run = prefix(rep, int(failing[cap - 1]) // batch, "stop at cap")
    assert fails.tobytes() == S.collect_truth(res[:run], seeds[:run], cap, 0)[1] and len(fails) == cap
    assert [int(x) for x in hist] == np.bincount(res["verdict"][:run], minlength=8).tolist()
    n_groups = 40
    rep, grp = hip.run_campaign_seeds(w, seeds, groups=(GROUPS[0], "trace", n_groups), stop_at_groups=True, **kw)
    every = S.all_groups(res, seeds, GROUPS_MASK, A.GROUP_KEY_TRACE)
    stop_pos = int(np.nonzero(seeds == np.uint64(every[n_groups - 1][3]))[0][0])              # where the 40th mode first appears
    run = prefix(rep, stop_pos // batch, "stop at groups")
    assert G.of_report(grp) == S.groups_truth(res[:run], seeds[:run], GROUPS_MASK, A.GROUP_KEY_TRACE, n_groups) and len(grp) == n_groups
    res_b = results_of(seeds, side_b=True)
    differs = np.nonzero(D.masks(res, res_b, A.DIFF_VERDICT))[0]
    rep_a, rep_b, d = hip.run_campaign_diff_seeds(w, seeds, other_config=A.Config.default(), fields=A.DIFF_VERDICT, max_listed=cap, stop_at_diffs=True, **kw)
    run = prefix(rep_a, int(differs[cap - 1]) // batch, "stop at diffs")
    assert rep_b.seeds_run == run and D.of_report(d) == S.diff_truth(res[:run], res_b[:run], seeds[:run], A.DIFF_VERDICT, cap) and len(d) == cap
    # without a flag the whole list runs
    assert hip.run_campaign_seeds(w, seeds, collect=cap, **kw)[0].seeds_run == len(seeds)


# ---- resolve ---------------------------------------------------------------------------------------------------------------------------
def test_resolving_list_campaigns(hip):
    """The jittery ping-pong's ladder (tests/test_campaign_resolve_gpu.py) is the per-seed truth under grown limits.  The list: every seed the
    first pass leaves re-runnable, united with every fifth seed.  Every report is over the resolved results restricted to the list, and the
    account is account_truth of the restricted ladder."""
    w, cfg, lim, resolved, k, rungs, _ = jittery(hip, 2)
    at = np.union1d(np.nonzero(k > 0)[0], np.arange(0, JTOTAL, 5))
    seeds = np.uint64(JSEED0) + at.astype(np.uint64)
    res = resolved[at]
    want_acct = account_truth(k[at], [r[at] for r in rungs], res, lim, 2, BATCH)
    assert want_acct["n_first_pass"] > 200 and want_acct["n_by_round"][1] > 100 and len(seeds) > want_acct["n_first_pass"] + 500
    kw = dict(batch=BATCH, in_flight=2, config=cfg, limits=lim, resolve=2)
    rep = hip.run_campaign_seeds(w, seeds, **kw)
    assert S.of_campaign(rep) == S.campaign_truth(res, seeds), (S.of_campaign(rep), S.campaign_truth(res, seeds))
    assert account(hip.campaign_resolved()) == want_acct, (account(hip.campaign_resolved()), want_acct)
    rep, fails, hist = hip.run_campaign_seeds(w, seeds, collect=len(seeds), list_runner=True, **kw)
    words, rec_bytes = S.collect_truth(res, seeds, len(seeds), 1)
    assert S.of_campaign(rep) == S.campaign_truth(res, seeds) and fails.tobytes() == rec_bytes and [int(x) for x in hist] == [int(x) for x in words[6:14]]
    assert account(hip.campaign_resolved()) == want_acct
    # without the flag the first pass's runner verdicts are what is counted
    first = hip.run_campaign_seeds(w, seeds, batch=BATCH, in_flight=2, config=cfg, limits=lim)
    assert first.n_runner == int((rungs[0][at]["verdict"] >= A.OVERFLOW).sum()) >= want_acct["n_first_pass"] and bytes(hip.campaign_resolved()) == bytes(112)
    # the differential form: both sides the same run, each resolved on its own — nothing differs, and the account sums the two sides
    rep_a, rep_b, d = hip.run_campaign_diff_seeds(w, seeds, max_listed=16, **kw)
    assert S.of_campaign(rep_a) == S.of_campaign(rep_b) == S.campaign_truth(res, seeds)
    assert D.of_report(d) == S.diff_truth(res, res, seeds, A.DIFF_ALL, 16) and d.n_differ == 0 and d.n_incomparable == rep_a.n_runner
    both = account(hip.campaign_resolved())
    assert both == {f: (v if f in ("rounds", "reserved") else [2 * x for x in v] if f == "n_by_round" else 2 * v) for f, v in want_acct.items()}, both


# ---- observe composition ---------------------------------------------------------------------------------------------------------------
def test_observe_explains_the_listed_seeds(hip):
    w, cfg, _ = lossy_pingpong()
    seeds = failing_seeds()
    rep, fails, hist, obs = hip.run_campaign_seeds(w, seeds, batch=BATCH, config=cfg, collect=8, observe=16)
    assert (fails["seed"] == seeds[:8]).all() and rep.seeds_run == len(seeds)
    traces = hip.trace_seeds(w, [int(s) for s in seeds[:8]], cfg, obs_cap=16)
    assert obs == [t.observations for t in traces] and len(obs) == 8
    w2, cfg2, want2 = G.traced_pingpong()                                                    # ... and a workload that does trace something
    corpus = np.uint64(G.SEED0) + np.nonzero(want2["verdict"] != A.PASS)[0].astype(np.uint64)
    rep, grp = hip.run_campaign_seeds(w2, corpus, batch=BATCH, config=cfg2, groups=(GROUPS[0], "obs", 8), observe=16)
    idx = (corpus - np.uint64(G.SEED0)).astype(np.int64)
    assert G.of_report(grp) == S.groups_truth(want2[idx], corpus, GROUPS_MASK, A.GROUP_KEY_OBS, 8) and 2 <= len(grp) <= 3
    assert grp.observations == [t.observations for t in hip.trace_seeds(w2, [int(g["first_seed"]) for g in grp.groups], cfg2, obs_cap=16)]
    assert sorted(len(o) for o in grp.observations)[0] == 0 and any(len(o) == 1 for o in grp.observations)


# ---- the example -----------------------------------------------------------------------------------------------------------------------
def test_the_corpus_example(hip):
    """examples/corpus_test.cpp, built and run the way tests/test_abi.py builds the examples: a collecting campaign over the range, then the
    fix diffed over exactly the failing seeds."""
    exe = os.path.join(ROOT, "examples", "corpus_test")
    subprocess.check_call(["g++", "-std=c++17", "-O2", os.path.join(ROOT, "examples", "corpus_test.cpp"), "-o", exe,
                           "-L" + os.path.join(ROOT, "madsim_amd"), "-lmadsim_hip", "-Wl,-rpath," + os.path.join(ROOT, "madsim_amd")])
    p = subprocess.run([exe], env=dict(os.environ, MADSIM_TEST_SEED=str(SEED0), MADSIM_TEST_NUM="40000"), capture_output=True, text=True, timeout=120)
    print(p.stdout, p.stderr)
    assert p.returncode == 0, (p.returncode, p.stdout, p.stderr)
    m = re.search(r"(\d+) of (\d+) fixed, 0 broken", p.stdout)
    assert m and m.group(1) == m.group(2) and int(m.group(1)) > 1000, p.stdout
    assert re.search(r"40000 seeds from %d, %s fail" % (SEED0, m.group(1)), p.stdout)
    assert re.search(r"seeds run: 40000 to find them, %s per side" % m.group(1), p.stdout)
