"""Self-resolving campaigns (MADSIM_CAMPAIGN_RESOLVE) on the MI355X, every form, against the per-seed LADDER — never against a second call of
the code under test.  The ladder of a range is madsim_hip_run_batch over the whole range under G^j(lim), j = 0 .. R, with G^j from
madsim_hip_grow_limits; the resolved result of a seed is picked from it on the host by the contract of include/madsim_hip.h (the first rung
whose result is not re-runnable, or rung R), and the host references the suite already has (listed(), stats_ref, groups_ref, diff_ref) run
over that array.  Where the ladder settles a seed its bytes must also be the CPU oracle's.  Every precondition a case rests on — that the
first pass does leave runner verdicts, that seeds settle in different rounds — is asserted from the ladder, so no case passes vacuously."""
import functools

import numpy as np
import pytest

import oracle
from madsim_amd import _abi as A
from madsim_amd import workload as W
from tests import diff_ref as D
from tests import groups_ref as G
from tests import stats_ref as S
from tests.test_collect_gpu import listed

pytestmark = pytest.mark.gpu

NONE = (1 << 64) - 1
BATCH = 4096
REPORT_FIELDS = ("seeds_run", "batches_run", "first_failing_seed", "n_failed", "n_runner", "total_steps", "total_clock_ns")
ACCOUNT_FIELDS = ("n_first_pass", "n_resolved", "n_unresolved", "batches_resolved", "rounds", "reserved")


# ---- the truth ---------------------------------------------------------------------------------------------------------------------
def steps_maxed(lim):
    """The step cap of `lim` sits at its ceiling (step_ceiling of madsim_hip.cpp, restated)."""
    first = lim.max_steps or 1 << 24
    return first >= max(lim.max_steps_ceiling or 1 << 28, first)


def rerunnable(results, lim):
    v = results["verdict"]
    return (v == A.OVERFLOW) | ((v == A.STEP_LIMIT) & (not steps_maxed(lim)))


def ladder(run_batch, grown_limits, w, seed0, total, cfg, lim, rounds):
    """(resolved results, k: the rung each seed's result comes from, the rungs that some seed reached) for `rounds` rounds."""
    lim = lim or A.Limits()
    rungs, k = [], np.zeros(total, dtype=np.int64)
    live = np.ones(total, dtype=bool)                                   # seeds whose every rung so far was re-runnable
    resolved = None
    for j in range(rounds + 1):
        if not live.any():                                              # nobody is left to re-run: the rungs above are never asked for
            break
        lim_j = grown_limits(w, lim, j)
        r = run_batch(w, seed0, total, cfg, lim_j)
        r = r[0] if isinstance(r, tuple) else r
        rungs.append(r)
        if resolved is None:
            resolved = r.copy()
        else:
            resolved[live] = r[live]
        k[live] = j
        if j < rounds:
            live = live & rerunnable(r, lim_j)
    return resolved, k, rungs


def account_truth(k, rungs, resolved, lim, rounds, batch):
    """madsim_resolve_t's integer fields from the ladder; batches_resolved for the cut `batch` (the one field that names the cut)."""
    first = rerunnable(rungs[0], lim or A.Limits())
    assert ((k > 0) == first).all()
    by_round = [int((k >= r).sum()) for r in range(1, 9)]
    n_res = int((first & (resolved["verdict"] < A.OVERFLOW)).sum())
    n_batches = sum(1 for lo in range(0, len(k), batch) if first[lo:lo + batch].any())
    return {"n_first_pass": int(first.sum()), "n_resolved": n_res, "n_unresolved": int(first.sum()) - n_res, "n_by_round": by_round,
            "batches_resolved": n_batches, "rounds": rounds, "reserved": 0}


def account(acct):
    out = {f: int(getattr(acct, f)) for f in ACCOUNT_FIELDS}
    out["n_by_round"] = [int(x) for x in acct.n_by_round]
    return out


def plain_truth(results, seed0, batch):
    """madsim_campaign_t's integer fields for per-seed `results` of a range that ran whole."""
    v = results["verdict"]
    genuine = np.nonzero((v != A.PASS) & (v < A.OVERFLOW))[0]
    return {"seeds_run": len(v), "batches_run": (len(v) + batch - 1) // batch, "first_failing_seed": seed0 + int(genuine[0]) if len(genuine) else NONE,
            "n_failed": len(genuine), "n_runner": int((v >= A.OVERFLOW).sum()), "total_steps": int(results["steps"].astype(np.uint64).sum()),
            "total_clock_ns": int(results["clock_ns"].sum())}


def report(rep):
    return {f: int(getattr(rep, f)) for f in REPORT_FIELDS}


def check_collect(got, results, seed0, cap, batch, list_runner=False, what=None):
    rep, fails, hist = got
    want = listed(results, seed0, cap, list_runner)
    print(what, "listed", len(fails), len(want), "hist", hist.tolist(), np.bincount(np.minimum(results["verdict"], 7), minlength=8).tolist())
    assert report(rep) == plain_truth(results, seed0, batch), (what, report(rep), plain_truth(results, seed0, batch))
    assert fails.tobytes() == want.tobytes(), (what, "the list")
    assert (hist == np.bincount(np.minimum(results["verdict"], 7), minlength=8)).all(), (what, hist)
    assert int(hist[4:].sum()) == rep.n_runner and int(hist[1:4].sum()) == rep.n_failed


# ---- the workloads -----------------------------------------------------------------------------------------------------------------
def jittery_pingpong(nappers=6, rounds=4):
    """A two-node ping-pong on a lossy network beside `nappers` tasks that each draw a bool and sleep two seconds on `true`: the timer heap a seed
    needs is the ping-pong's plus a binomial number of sleeps, so a tight heap quota overflows for some seeds and not for others, and the
    ones it overflows for settle after different numbers of doublings.  (The plain N-node ping-pong needs the same heap for every seed: under
    any quota its seeds overflow all together or not at all — the ladder says so — which cannot show more than one population.)"""
    wl = W.WorkloadBuilder()
    n1, n2 = wl.create_node(), wl.create_node()
    a1, a2 = wl.addr(n1, 1), wl.addr(n2, 1)
    t1 = wl.task(n1)
    t1.bind(a1).sleep(secs=1).set(0, rounds)
    top = t1.label()
    t1.send_to(a1, a2, 1, 7).recv_from(a1, 1).assert_val(9).djnz(0, top).done()
    t2 = wl.task(n2)
    t2.bind(a2).set(0, rounds)
    top = t2.label()
    t2.recv_from(a2, 1).assert_val(7).reply(a2, 1, 9).djnz(0, top).done()
    tasks = [t1, t2]
    for i in range(nappers):
        s = wl.task(n1 if i & 1 else n2)
        s.rand_bool(0)
        skip = len(s.code); s.jeq(0, 0)
        s.sleep(secs=2)
        s.code[skip][2] = s.label()
        s.done()
        tasks.append(s)
    m = wl.main()
    for t in tasks:
        m.spawn(t)
    for t in tasks:
        m.join(t)
    m.done()
    lim = A.Limits()
    lim.heap_lds_slots, lim.heap_spill_slots = 2, 1
    return wl.build(), A.Config.default(packet_loss_rate=0.01, loss_table=(0.3,)), lim


JSEED0, JTOTAL = 20_000, 8192


@functools.lru_cache(maxsize=None)
def jittery(hip, rounds):
    """The jittery ping-pong's ladder for `rounds` rounds over JTOTAL seeds, computed once; the preconditions asserted."""
    w, cfg, lim = jittery_pingpong()
    resolved, k, rungs = ladder(hip.run_batch, hip.grown_limits, w, JSEED0, JTOTAL, cfg, lim, rounds)
    want, _ = oracle.run_batch(w, JSEED0, JTOTAL, cfg, lim)
    settled = resolved["verdict"] < A.OVERFLOW
    assert (resolved[settled] == want[settled]).all()
    pops = np.bincount(k, minlength=4)
    print("jittery ping-pong, rounds", rounds, "seeds by the rung they settle at", pops.tolist(), "unsettled", int((~settled).sum()))
    assert pops[0] > 100 and pops[1] > 100 and (rounds < 2 or pops[2] > 100), pops        # never re-run / settled at round 1 / at round 2
    assert int((want["verdict"] == A.DEADLOCK).sum()) > 100
    for a in (resolved, k) + tuple(rungs):
        a.setflags(write=False)
    return w, cfg, lim, resolved, k, rungs, want


# ---- everything overflows, one round settles all -------------------------------------------------------------------------------------
def test_everything_overflows_and_one_round_settles_all(hip):
    w = W.pingpong(4, 16)
    lim = A.Limits(); lim.heap_lds_slots, lim.heap_spill_slots = 2, 0          # a capacity nobody fits
    total = 3 * BATCH
    resolved, k, rungs = ladder(hip.run_batch, hip.grown_limits, w, 0, total, None, lim, 4)
    want, _ = oracle.run_batch(w, 0, total)
    assert (rungs[0]["verdict"] == A.OVERFLOW).all() and (k == 1).all() and (resolved == want).all()
    # without the flag: the report tests/test_collect_gpu.py describes, and an all-zero account
    rep, fails, hist = hip.run_campaign(w, 0, total, BATCH, 2, True, None, lim, collect=50)
    assert len(fails) == 0 and hist[A.OVERFLOW] == total == rep.n_runner and rep.first_failing_seed == NONE
    assert bytes(hip.campaign_resolved()) == bytes(112)
    # with it: the oracle's report, list and histogram
    got = hip.run_campaign(w, 0, total, BATCH, 2, True, None, lim, collect=50, resolve=True)
    check_collect(got, want, 0, 50, BATCH, what="all overflow, resolved")
    acct = hip.campaign_resolved()
    assert got[0].n_runner == 0 and got[0].n_failed == 0 and got[2][A.PASS] == total
    assert account(acct) == account_truth(k, rungs, resolved, lim, 4, BATCH) and account(acct)["n_by_round"] == [total, 0, 0, 0, 0, 0, 0, 0]
    assert (acct.n_first_pass, acct.n_resolved, acct.n_unresolved, acct.batches_resolved, acct.rounds) == (total, total, 0, 3, 4)
    assert 0 < acct.rerun_kernel_ms < got[0].kernel_ms
    plain = hip.run_campaign(w, 0, total, BATCH, 2, True, None, lim, resolve=True)                  # the plain form, LIST_RUNNER riding along
    assert report(plain) == plain_truth(want, 0, BATCH)
    got = hip.run_campaign(w, 0, total, BATCH, 2, True, None, lim, collect=50, list_runner=True, resolve=1)
    check_collect(got, want, 0, 50, BATCH, list_runner=True, what="all overflow, one round")
    assert hip.campaign_resolved().rounds == 1
    # the flag is per call: the next call without it reports the first pass again, and the account is that call's
    assert hip.run_campaign(w, 0, total, BATCH, 2, True, None, lim).n_runner == total and bytes(hip.campaign_resolved()) == bytes(112)


# ---- a natural mix -------------------------------------------------------------------------------------------------------------------
def streaming(state, spill=None):
    """The lossy streaming_topology of tests/test_collect_gpu.py in one of its two state layouts; `spill`: a tighter heap-spill quota than the
    workload's own (161 / 184 entries), under which the first pass answers many seeds with an overflow."""
    w, cfg, lim = W.streaming_topology(), A.Config.default(packet_loss_rate=0.05), W.streaming_topology_limits()
    if state == "lds":
        lim.state_mem, lim.heap_lds_slots, lim.heap_spill_slots = A.STATE_LDS, 8, 184
    if spill is not None:
        lim.heap_spill_slots = spill
    return w, cfg, lim


@pytest.mark.parametrize("state,spill", [("global", None), ("lds", None), ("global", 56), ("lds", 56)])
def test_a_natural_mix(hip, state, spill):
    """The lossy streaming_topology in both state layouts, 46 % of whose range panics: under the workload's own limits (what the first pass
    leaves unsettled there is printed: on these 4 096 seeds it is nothing, and the campaign must then report what it reports without the
    flag), and under a spill quota of 56, where the first pass overflows for hundreds of seeds."""
    w, cfg, lim = streaming(state, spill)
    seed0, total, batch = 1000, 4096, 1500
    resolved, k, rungs = ladder(hip.run_batch, hip.grown_limits, w, seed0, total, cfg, lim, 4)
    want, _ = oracle.run_batch(w, seed0, total, cfg, lim)
    first_runner = int((rungs[0]["verdict"] >= A.OVERFLOW).sum())
    settled = resolved["verdict"] < A.OVERFLOW
    print(state, "first pass runner verdicts", first_runner, "by rung", np.bincount(k, minlength=5).tolist(), "unsettled", int((~settled).sum()))
    if spill is not None:                                                                   # the gap this closes is there
        assert first_runner > 400 and (k > 0).sum() == first_runner
    else:
        assert hip.run_campaign(w, seed0, total, batch, 2, False, cfg, lim).n_runner == first_runner
    assert (resolved[settled] == want[settled]).all() and int((want["verdict"] == A.PANIC).sum()) == 1884
    got = hip.run_campaign(w, seed0, total, batch, 2, False, cfg, lim, collect=2000, resolve=True)
    check_collect(got, resolved, seed0, 2000, batch, what=("streaming_topology", state))
    assert account(hip.campaign_resolved()) == account_truth(k, rungs, resolved, lim, 4, batch)
    if settled.all() and int((want["verdict"] != A.PASS).sum()) <= 2000:                       # every seed settled: the oracle's panics, all of them
        assert got[0].n_runner == 0 and got[2][A.PANIC] == 1884
        panics = got[1][got[1]["verdict"] == A.PANIC]
        assert len(panics) == 1884 and (panics["seed"] == seed0 + np.nonzero(want["verdict"] == A.PANIC)[0]).all()
    # STOP_AT_FAILURE: the first genuine failure of the RESOLVED results, in the batch that holds it
    genuine = np.nonzero((resolved["verdict"] != A.PASS) & (resolved["verdict"] < A.OVERFLOW))[0]
    stop = int(genuine[0]) // 64
    rep = hip.run_campaign(w, seed0, total, 64, 2, True, cfg, lim, resolve=True)
    n = (stop + 1) * 64
    assert rep.first_failing_seed == seed0 + int(genuine[0]) and rep.seeds_run == n and rep.batches_run == stop + 1 <= rep.batches_launched <= stop + 2
    assert report(rep) == plain_truth(resolved[:n], seed0, 64)


def test_stop_at_failure_finds_the_failure_an_overflow_was_hiding(hip):
    """The jittery ping-pong: a seed that deadlocks once its heap fits, earlier than any failure the first pass shows."""
    w, cfg, lim, resolved, k, rungs, want = jittery(hip, 4)
    genuine = lambda r: np.nonzero((r["verdict"] != A.PASS) & (r["verdict"] < A.OVERFLOW))[0]      # noqa: E731
    first_pass = genuine(rungs[0])
    for at in (int(i) for i in genuine(resolved) if k[i] > 0):                               # a failure the first pass answered with an overflow ...
        lo = at - at % 64
        if lo + int(genuine(resolved[lo:])[0]) == at and not ((first_pass >= lo) & (first_pass < lo + 64)).any():
            break                                                                         # ... first of its batch, which shows the first pass no failure
    else:
        pytest.fail("no batch of 64 whose only failures hide behind overflows")
    total = JTOTAL - lo
    rep = hip.run_campaign(w, JSEED0 + lo, total, 64, 3, True, cfg, lim, resolve=True)
    assert rep.first_failing_seed == JSEED0 + at and (rep.seeds_run, rep.batches_run) == (64, 1)
    assert report(rep) == plain_truth(resolved[lo:lo + 64], JSEED0 + lo, 64)
    without = hip.run_campaign(w, JSEED0 + lo, total, 64, 3, True, cfg, lim)
    assert without.first_failing_seed > rep.first_failing_seed and without.seeds_run > 64       # the search went past it


def test_grown_limits_that_fit_no_build_fail_the_call(hip):
    """Sixteen sockets with mailboxes of 64 in the LDS layout: the first pass runs (and overflows its two heap slots), the first round's limits
    ask for mailboxes of 128 / 127, and sixteen of those are more per-seed LDS than any build of the layout has.  (A base-op workload's
    mbox_msgs alone no longer does it: its ladder ends at 127, the most its builds take.)  The call fails as madsim_hip_run_batch fails under
    those limits, with every stream drained: the context runs the next campaigns as if nothing had happened."""
    w, total = W.pingpong(16, 2), 8192
    lim = A.Limits()
    lim.state_mem, lim.heap_lds_slots, lim.heap_spill_slots, lim.mbox_regs, lim.mbox_msgs = A.STATE_LDS, 2, 0, 64, 64
    first, _ = hip.run_batch(w, 0, 256, None, lim)
    grown = hip.grown_limits(w, lim, 1)
    assert (first["verdict"] == A.OVERFLOW).all() and (grown.mbox_regs, grown.mbox_msgs) == (128, 127)
    with pytest.raises(hip.MadsimHipError, match="per-seed LDS state too large"):
        hip.run_batch(w, 0, 256, None, grown)
    with pytest.raises(hip.MadsimHipError, match="per-seed LDS state too large"):
        hip.run_campaign(w, 0, total, 2048, 3, False, None, lim, resolve=True)
    rep = hip.run_campaign(w, 0, total, 2048, 3, False, None, lim)                               # without the flag: the first pass, whole
    assert (rep.seeds_run, rep.n_runner, rep.batches_run) == (total, total, 4) and bytes(hip.campaign_resolved()) == bytes(112)
    lim.mbox_regs = lim.mbox_msgs = 0
    rep = hip.run_campaign(w, 0, total, 2048, 3, False, None, lim, resolve=True)                 # limits that grow: every seed settles
    assert (rep.seeds_run, rep.n_runner, rep.n_failed) == (total, 0, 0) and hip.campaign_resolved().n_by_round[0] == total


# ---- more than one round -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rounds", [4, 2, 1])
def test_more_than_one_round(hip, rounds):
    """Seeds never re-run, settled at round 1, at round 2 (and 3); with fewer rounds than the ladder needs the rest stays a runner verdict."""
    w, cfg, lim, resolved, k, rungs, want = jittery(hip, rounds)
    truth = account_truth(k, rungs, resolved, lim, rounds, BATCH)
    unsettled = int((resolved["verdict"] >= A.OVERFLOW).sum())
    assert (unsettled == 0) == (rounds == 4) and truth["n_unresolved"] == unsettled
    assert truth["n_by_round"][0] > truth["n_by_round"][1] > 0 or rounds == 1
    got = hip.run_campaign(w, JSEED0, JTOTAL, BATCH, 2, False, cfg, lim, collect=JTOTAL, list_runner=True, resolve=rounds)
    check_collect(got, resolved, JSEED0, JTOTAL, BATCH, list_runner=True, what=("jittery", rounds))
    have = account(hip.campaign_resolved())
    print("account", have, truth)
    assert have == truth
    assert got[0].n_runner == unsettled and sum(have["n_by_round"][rounds:]) == 0


# ---- the step cap --------------------------------------------------------------------------------------------------------------------
def test_the_step_cap(hip):
    w, total = W.pingpong(4, 16), BATCH + 100
    lim = A.Limits(); lim.max_steps, lim.max_steps_ceiling = 64, 1024
    resolved, k, rungs = ladder(hip.run_batch, hip.grown_limits, w, 0, total, None, lim, 4)
    want, _ = oracle.run_batch(w, 0, total)
    assert (rungs[0]["verdict"] == A.STEP_LIMIT).all() and (k == 1).all() and (resolved == want).all()      # one round settles every seed
    got = hip.run_campaign(w, 0, total, BATCH, 2, False, None, lim, collect=10, list_runner=True, resolve=True)
    check_collect(got, want, 0, 10, BATCH, list_runner=True, what="step cap, room to grow")
    assert account(hip.campaign_resolved()) == account_truth(k, rungs, resolved, lim, 4, BATCH)
    assert got[0].n_runner == 0 and hip.campaign_resolved().n_by_round[0] == total
    # a ceiling the workload exceeds: one round, at the ceiling, and the seeds keep their verdict
    lim.max_steps_ceiling = 128
    assert int(want["steps"].min()) > 128
    resolved, k, rungs = ladder(hip.run_batch, hip.grown_limits, w, 0, total, None, lim, 4)
    assert (resolved["verdict"] == A.STEP_LIMIT).all() and (k == 1).all() and steps_maxed(hip.grown_limits(w, lim, 1)) and not steps_maxed(lim)
    got = hip.run_campaign(w, 0, total, BATCH, 2, False, None, lim, collect=10, list_runner=True, resolve=True)
    check_collect(got, resolved, 0, 10, BATCH, list_runner=True, what="step cap, at the ceiling")
    acct = hip.campaign_resolved()
    assert account(acct) == account_truth(k, rungs, resolved, lim, 4, BATCH)
    assert (acct.n_unresolved, acct.n_resolved, acct.n_by_round[0], acct.n_by_round[1], got[0].n_runner) == (total, 0, total, 0, total)
    # a cap that already sits at its ceiling: nothing is re-runnable, no round runs
    lim.max_steps, lim.max_steps_ceiling = 64, 64
    got = hip.run_campaign(w, 0, total, BATCH, 2, False, None, lim, resolve=True)
    acct = hip.campaign_resolved()
    assert got.n_runner == total and (acct.n_first_pass, acct.batches_resolved, acct.rounds, acct.rerun_kernel_ms) == (0, 0, 4, 0.0)


# ---- every form ----------------------------------------------------------------------------------------------------------------------
def test_every_form(hip):
    w, cfg, lim, resolved, k, rungs, want = jittery(hip, 2)                                    # two rounds: settled seeds and unsettled ones
    assert (resolved["verdict"] >= A.OVERFLOW).any() and (k == 2).any()
    include, mask = (A.PASS, A.DEADLOCK), S.mask(A.PASS, A.DEADLOCK)
    cap = 300
    want_list = listed(resolved, JSEED0, cap, True).tobytes()
    want_stats = S.stats_truth(resolved, JSEED0, mask, 16)
    want_groups = G.groups_truth(resolved, JSEED0, mask, A.GROUP_KEY_OBS, 32)
    kw = dict(config=cfg, limits=lim, collect=cap, list_runner=True, resolve=2)
    got = hip.run_campaign(w, JSEED0, JTOTAL, BATCH, 2, **kw)
    check_collect(got, resolved, JSEED0, cap, BATCH, list_runner=True, what="collect")
    rep, fails, hist, stats = hip.run_campaign_stats(w, JSEED0, JTOTAL, BATCH, 2, include=include, top_k=16, **kw)
    check_collect((rep, fails, hist), resolved, JSEED0, cap, BATCH, list_runner=True, what="stats: collect riding along")
    assert S.same(S.of_stats(stats), want_stats)
    rep, fails, hist, stats, groups = hip.run_campaign_groups(w, JSEED0, JTOTAL, BATCH, 2, include=include, key="obs", max_groups=32, stats=(include, 16), **kw)
    check_collect((rep, fails, hist), resolved, JSEED0, cap, BATCH, list_runner=True, what="groups: collect riding along")
    assert fails.tobytes() == want_list and S.same(S.of_stats(stats), want_stats)
    assert G.of_report(groups) == want_groups, (G.of_report(groups), want_groups)
    assert account(hip.campaign_resolved()) == account_truth(k, rungs, resolved, lim, 2, BATCH)
    # the statistics of the issue's own setting: PASS | PANIC over the lossy streaming_topology, with the groups by obs
    w2, cfg2, lim2 = streaming("global", 56)
    res2, k2, rungs2 = ladder(hip.run_batch, hip.grown_limits, w2, 1000, 4096, cfg2, lim2, 4)
    assert (k2 > 0).sum() > 400 and (res2["verdict"] < A.OVERFLOW).all()
    inc2, mask2 = (A.PASS, A.PANIC), S.mask(A.PASS, A.PANIC)
    rep, fails, hist, stats, groups = hip.run_campaign_groups(w2, 1000, 4096, 1500, 2, config=cfg2, limits=lim2, include=inc2, key="obs", max_groups=32,
                                                              stats=(inc2, 16), collect=100, list_runner=True, resolve=True)
    check_collect((rep, fails, hist), res2, 1000, 100, 1500, list_runner=True, what="streaming_topology: groups, stats, collect")
    assert S.same(S.of_stats(stats), S.stats_truth(res2, 1000, mask2, 16))
    assert G.of_report(groups) == G.groups_truth(res2, 1000, mask2, A.GROUP_KEY_OBS, 32)


def test_the_differential_form(hip):
    """A = the tight limits, B = roomy ones, one workload, every field: with the flag nothing differs and only what no round settles is incomparable."""
    w, cfg, lim, resolved, k, rungs, want = jittery(hip, 4)
    roomy = A.Limits()
    roomy.heap_lds_slots, roomy.heap_spill_slots = 8, 64
    b, _ = hip.run_batch(w, JSEED0, JTOTAL, cfg, roomy)
    assert (b == want).all() and (b["verdict"] < A.OVERFLOW).all()                              # side B never needs a round
    first_runner = int((rungs[0]["verdict"] >= A.OVERFLOW).sum())
    assert first_runner > 1000
    for batch, in_flight in ((BATCH, 2), (1000, 3)):
        rep_a, rep_b, d = got = hip.run_campaign_diff_resolved(w, JSEED0, JTOTAL, True, config=cfg, limits=lim, other_limits=roomy, max_listed=8,
                                                               batch=batch, in_flight=in_flight)
        assert D.of_report(d) == D.diff_truth(resolved, b, JSEED0, A.DIFF_ALL, 8)
        assert d.n_differ == 0 and d.n_incomparable == 0 and int(np.trace(d.transitions)) == int(rep_a.seeds_run) == JTOTAL
        assert report(rep_a) == plain_truth(resolved, JSEED0, batch) and report(rep_b) == plain_truth(b, JSEED0, batch)
        assert account(hip.campaign_resolved()) == account_truth(k, rungs, resolved, lim, 4, batch)
    # two rounds: the seeds they leave unsettled, and no other, are incomparable
    res2, k2, rungs2 = jittery(hip, 2)[3:6]
    left = int((res2["verdict"] >= A.OVERFLOW).sum())
    assert 0 < left < first_runner
    with hip.Context(0) as c0, hip.Context(0) as c1:
        for got in (c0.run_campaign_diff(w, JSEED0, JTOTAL, config=cfg, limits=lim, other_limits=roomy, max_listed=8, batch=1000, resolve=2),
                    hip.run_campaign_diff_multi([c0, c1], w, JSEED0, JTOTAL, config=cfg, limits=lim, other_limits=roomy, max_listed=8, batch=1000, resolve=2)):
            rep_a, rep_b, d = got
            assert D.of_report(d) == D.diff_truth(res2, b, JSEED0, A.DIFF_ALL, 8)
            assert d.n_differ == 0 and d.n_incomparable == left == rep_a.n_runner and int(np.trace(d.transitions)) == JTOTAL - left
            assert account(c0.campaign_resolved()) == account_truth(k2, rungs2, res2, lim, 2, 1000)
        assert account(c1.campaign_resolved()) == account(c0.campaign_resolved())            # a _multi call: the same totals in every context
    # both sides tight: both are resolved, each under its own limits, and the account sums them
    rep_a, rep_b, d = hip.run_campaign_diff_resolved(w, JSEED0, JTOTAL, 4, config=cfg, limits=lim, other_limits=lim, batch=BATCH)
    one = account_truth(k, rungs, resolved, lim, 4, BATCH)
    both = account(hip.campaign_resolved())
    assert d.n_differ == 0 and d.n_incomparable == 0 and report(rep_a) == report(rep_b) == plain_truth(resolved, JSEED0, BATCH)
    assert both["n_first_pass"] == 2 * one["n_first_pass"] and both["n_by_round"] == [2 * x for x in one["n_by_round"]] and both["batches_resolved"] == 2 * one["batches_resolved"]
    # without the flag: every first-pass runner verdict is incomparable, and the account is all zero
    rep_a, rep_b, d = hip.run_campaign_diff(w, JSEED0, JTOTAL, config=cfg, limits=lim, other_limits=roomy, batch=BATCH)
    assert d.n_incomparable == first_runner == rep_a.n_runner and D.of_report(d) == D.diff_truth(rungs[0], b, JSEED0, A.DIFF_ALL, 0)
    assert bytes(hip.campaign_resolved()) == bytes(112)


# ---- the cut does not matter ---------------------------------------------------------------------------------------------------------
def test_the_cut_does_not_matter(hip):
    """batch (100: partial waves; 4 096; the whole range), batches in flight, one context, two, the context form: the same bytes in every
    struct, and the same account but for rerun_kernel_ms — and batches_resolved, which counts batches and follows from the ladder per cut."""
    w, cfg, lim, resolved, k, rungs, want = jittery(hip, 4)
    include, mask, cap = (A.PASS, A.DEADLOCK), S.mask(A.PASS, A.DEADLOCK), 500
    want_list, want_stats = listed(resolved, JSEED0, cap).tobytes(), S.stats_truth(resolved, JSEED0, mask, 16)
    want_groups = G.groups_truth(resolved, JSEED0, mask, A.GROUP_KEY_OBS, 32)

    def one(call, batch, in_flight, acct_of, what):
        rep, fails, hist, stats, groups = call(w, JSEED0, JTOTAL, batch, in_flight, config=cfg, limits=lim, include=include, key="obs", max_groups=32,
                                               stats=(include, 16), collect=cap, resolve=True)
        check_collect((rep, fails, hist), resolved, JSEED0, cap, batch, what=what)
        assert fails.tobytes() == want_list and S.same(S.of_stats(stats), want_stats) and G.of_report(groups) == want_groups, what
        have, truth = account(acct_of()), account_truth(k, rungs, resolved, lim, 4, batch)
        assert have == truth, (what, have, truth)
        return {f: v for f, v in have.items() if f != "batches_resolved"}
    first = None
    for batch in (100, BATCH, JTOTAL):
        for in_flight in (1, 3, 8):
            acct = one(hip.run_campaign_groups, batch, in_flight, hip.campaign_resolved, (batch, in_flight))
            first = first or acct
            assert acct == first
    with hip.Context(0) as c0, hip.Context(0) as c1:
        assert one(c0.run_campaign_groups, BATCH, 3, c0.campaign_resolved, "context form") == first
        for batch, in_flight in ((100, 3), (BATCH, 2)):
            call = lambda *a, **kw: hip.run_campaign_groups_multi([c0, c1], *a, **kw)                # noqa: E731
            assert one(call, batch, in_flight, c1.campaign_resolved, ("two contexts", batch)) == first
            assert account(c0.campaign_resolved()) == account(c1.campaign_resolved())
