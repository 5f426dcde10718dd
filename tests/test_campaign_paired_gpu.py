"""Paired campaigns on the MI355X: madsim_hip_run_paired_campaign (and its context / several-contexts / list forms) against
tests/paired_ref.py's paired_truth over the CPU oracle's per-seed results of each side — never against a second call of the code under test.
The range is the four-node ping-pong over seeds 1 000 .. 10 999: the default config against a send latency of 2 .. 10 ms (every seed passes
on both sides and nearly every one ends at another virtual time), and against a packet loss of 0.002 (1 154 seeds deadlock on side B).
The populations of each case are asserted on the oracle's results in the fixture, so no case passes vacuously."""
import numpy as np
import pytest

import oracle
from madsim_amd import _abi as A
from madsim_amd import workload as W
from tests import diff_ref as D
from tests import paired_ref as R
from tests import test_campaign_resolve_gpu as RG

pytestmark = pytest.mark.gpu

SEED0, TOTAL = 1000, 10_000
CUTS = ((1000, 3), (4096, 1), (10_000, 2))
REPORT_FIELDS = ("seeds_run", "batches_run", "batches_launched", "first_failing_seed", "n_failed", "n_runner", "total_steps", "total_clock_ns")
PASS, PASS_OR_DEADLOCK = (A.PASS,), (A.PASS, A.DEADLOCK)


def report(rep):
    return {f: int(getattr(rep, f)) for f in REPORT_FIELDS}


def moved(t):
    """[(up, down, equal)] per metric of a truth."""
    return [(t[m]["dir"][R.UP]["n"], t[m]["dir"][R.DOWN]["n"], t[m]["n_equal"]) for m in R.METRICS]


def image(p):
    """Every byte a runtime.CampaignPaired carries, in one hashable value: two reports are the same bytes iff their images are equal."""
    out = [p.include_a, p.include_b, p.top_k, p.n_paired, p.n_unpaired, p.n_incomparable]
    for m in R.METRICS:
        out += [p.n_equal[m], p.sum_a[m], p.sum_b[m], p.n[m], p.min[m], p.max[m], p.sum[m], p.hist[m][0].tobytes(), p.hist[m][1].tobytes(),
                p.regressions(m).tobytes(), p.improvements(m).tobytes()]
    return tuple(out)


@pytest.fixture(scope="module")
def truth():
    """(workload, {name: config}, {name: the oracle's results — read-only}) with the populations the cases rest on asserted."""
    w = W.pingpong(4, 16)
    cfgs = {"default": A.Config.default(), "slow": A.Config.default(lat_lo_ns=2_000_000, lat_hi_ns=10_000_000), "lossy": A.Config.default(packet_loss_rate=0.002)}
    res = {}
    for name, cfg in cfgs.items():
        res[name], _ = oracle.run_batch(w, SEED0, TOTAL, cfg)
        res[name].setflags(write=False)
    assert (res["default"]["verdict"] == A.PASS).all() and (res["slow"]["verdict"] == A.PASS).all()
    t = R.paired_truth(res["default"], res["slow"], SEED0, 1, 1, 0)
    assert t["n_paired"] == TOTAL and moved(t) == [(8781, 1219, 0), (2344, 2238, 5418), (0, 0, 10_000), (4126, 4047, 1827)]
    assert np.bincount(res["lossy"]["verdict"], minlength=4).tolist() == [8846, 0, 1154, 0]
    t = R.paired_truth(res["default"], res["lossy"], SEED0, 1, 1, 0)
    assert (t["n_paired"], t["n_unpaired"], t["n_incomparable"]) == (8846, 1154, 0) and moved(t) == [(0, 0, 8846)] * 4
    t = R.paired_truth(res["default"], res["lossy"], SEED0, 1, 1 | 1 << A.DEADLOCK, 0)
    assert (t["n_paired"], t["n_unpaired"], t["n_incomparable"]) == (TOTAL, 0, 0) and moved(t)[:2] == [(331, 823, 8846), (0, 1154, 8846)]
    return w, cfgs, res


def check(got, a, b, seeds, inc_a, inc_b, k, what):
    """A call's CampaignPaired against the truth over the oracle's results; returns its image."""
    p = got[2]
    want = R.paired_truth(a, b, seeds, inc_a, inc_b, k)
    bad = R.differences(R.of_report(p), want)
    print(what, "paired", p.n_paired, want["n_paired"], "unpaired", p.n_unpaired, "incomparable", p.n_incomparable, "moved", moved(R.of_report(p)), bad)
    assert bad == [], (what, bad)
    assert (p.include_a, p.include_b, p.top_k) == (inc_a, inc_b, k)
    assert p.n_paired + p.n_unpaired + p.n_incomparable == int(got[0].seeds_run) == int(got[1].seeds_run) == len(a)
    return image(p)


def test_latency_shift_whatever_the_cut(hip, truth):
    """batch, batches in flight, two contexts on one device, the Context method: the truth, and the same bytes every time."""
    w, cfgs, res = truth
    a, b = res["default"], res["slow"]
    kw = dict(config=cfgs["default"], other_config=cfgs["slow"])
    for k in (16, 0):
        first = None
        for batch, in_flight in CUTS:
            got = hip.run_campaign_paired(w, SEED0, TOTAL, top_k=k, batch=batch, in_flight=in_flight, **kw)
            img = check(got, a, b, SEED0, 1, 1, k, ("range", k, batch, in_flight))
            first = img if first is None else first
            assert img == first
            assert RG.report(got[0]) == RG.plain_truth(a, SEED0, batch) and RG.report(got[1]) == RG.plain_truth(b, SEED0, batch)
        with hip.Context(0) as c0, hip.Context(0) as c1:
            assert check(c0.run_campaign_paired(w, SEED0, TOTAL, top_k=k, batch=1000, in_flight=3, **kw), a, b, SEED0, 1, 1, k, "context form") == first
            for batch, in_flight in CUTS[:2]:
                got = hip.run_campaign_paired_multi([c0, c1], w, SEED0, TOTAL, top_k=k, batch=batch, in_flight=in_flight, **kw)
                assert check(got, a, b, SEED0, 1, 1, k, ("two contexts", k, batch, in_flight)) == first
    p = hip.run_campaign_paired(w, SEED0, TOTAL, top_k=3, **kw)[2]
    assert p.mean_delta("clock_ns") > 0 and p.means("clock_ns")[1] - p.means("clock_ns")[0] == p.mean_delta("clock_ns")
    assert [int(s) for s in p.regressions("clock_ns")["seed"]] == [2690, 8727, 9725]           # (the oracle's three worst, checked above against the truth)
    lo, hi = p.quantile_bounds("clock_ns", A.PAIRED_UP, 0.5)
    assert p.min["clock_ns"][0] <= lo <= hi <= p.max["clock_ns"][0]


def test_packet_loss_and_the_include_masks(hip, truth):
    w, cfgs, res = truth
    a, b = res["default"], res["lossy"]
    kw = dict(config=cfgs["default"], other_config=cfgs["lossy"], top_k=4)
    for batch, in_flight in CUTS[:2]:
        got = hip.run_campaign_paired(w, SEED0, TOTAL, batch=batch, in_flight=in_flight, **kw)
        check(got, a, b, SEED0, 1, 1, 4, ("pass / pass", batch))
        assert (got[2].n_paired, got[2].n_unpaired, got[2].n_incomparable) == (8846, 1154, 0) and got[2].net_sum("clock_ns") == 0
        got = hip.run_campaign_paired(w, SEED0, TOTAL, other_include=PASS_OR_DEADLOCK, batch=batch, in_flight=in_flight, **kw)
        check(got, a, b, SEED0, 1, 5, 4, ("pass / pass or deadlock", batch))
        assert got[2].n_paired == TOTAL and got[2].n["clock_ns"] == (331, 823) and got[2].n["steps"] == (0, 1154)
    # the sides the other way round, and a mask that pairs only the seeds the loss broke
    got = hip.run_campaign_paired(w, SEED0, TOTAL, config=cfgs["lossy"], other_config=cfgs["default"], include=(A.DEADLOCK,), other_include=PASS, top_k=16, batch=3000)
    check(got, b, a, SEED0, 1 << A.DEADLOCK, 1, 16, "deadlock / pass")
    assert (got[2].n_paired, got[2].n_unpaired) == (1154, 8846) and got[2].n["steps"] == (1154, 0)
    # small ranges: fewer seeds than a batch, than a wave, one seed, none
    for at, total in ((0, 1), (0, 65), (5000, 700)):
        got = hip.run_campaign_paired(w, SEED0 + at, total, other_include=PASS_OR_DEADLOCK, **kw)
        check(got, a[at:at + total], b[at:at + total], SEED0 + at, 1, 5, 4, (at, total))
    rep_a, rep_b, p = hip.run_campaign_paired(w, SEED0, 0, **kw)
    assert (rep_a.seeds_run, p.n_paired, p.n_unpaired, p.n_incomparable, p.min["clock_ns"], p.max["clock_ns"]) == (0, 0, 0, 0, (A.U64_MAX,) * 2, (0, 0))


def test_list_forms(hip, truth):
    """A dense list is the range form byte for byte; a sparse list — every third seed and every seed side B fails — is the truth over those."""
    w, cfgs, res = truth
    a, b = res["default"], res["lossy"]
    kw = dict(config=cfgs["default"], other_config=cfgs["lossy"], other_include=PASS_OR_DEADLOCK, top_k=16)
    dense = np.arange(SEED0, SEED0 + TOTAL, dtype=np.uint64)
    rng = hip.run_campaign_paired(w, SEED0, TOTAL, batch=1000, in_flight=3, **kw)
    lst = hip.run_campaign_paired_seeds(w, dense, batch=1000, in_flight=3, **kw)
    assert check(lst, a, b, dense, 1, 5, 16, "dense list") == check(rng, a, b, SEED0, 1, 5, 16, "range")
    assert report(lst[0]) == report(rng[0]) and report(lst[1]) == report(rng[1])
    idx = np.unique(np.concatenate([np.arange(0, TOTAL, 3), np.nonzero(b["verdict"] != A.PASS)[0]]))
    sparse = dense[idx]
    assert len(sparse) > TOTAL // 3 + 700
    first = None
    with hip.Context(0) as c0, hip.Context(0) as c1:
        for what, call in (("default", lambda **k: hip.run_campaign_paired_seeds(w, sparse, **k)), ("context", lambda **k: c0.run_campaign_paired_seeds(w, sparse, **k)),
                           ("two contexts", lambda **k: hip.run_campaign_paired_seeds_multi([c0, c1], w, sparse, **k))):
            for batch, in_flight in ((500, 3), (4096, 1)):
                img = check(call(batch=batch, in_flight=in_flight, **kw), a[idx], b[idx], sparse, 1, 5, 16, ("sparse list", what, batch))
                first = img if first is None else first
                assert img == first


def test_with_a_diff_report(hip, truth):
    """diff given: the diff report is run_campaign_diff's, both plain reports are run_campaign's, and the paired report does not change."""
    w, cfgs, res = truth
    a, b = res["default"], res["lossy"]
    kw = dict(config=cfgs["default"], other_config=cfgs["lossy"])
    for batch, in_flight in CUTS[:2]:
        rep_a, rep_b, p, d = got = hip.run_campaign_paired(w, SEED0, TOTAL, other_include=PASS_OR_DEADLOCK, top_k=2, fields=A.DIFF_ALL, max_listed=8, batch=batch,
                                                           in_flight=in_flight, **kw)
        img = check(got, a, b, SEED0, 1, 5, 2, ("with diff", batch))
        assert D.of_report(d) == D.diff_truth(a, b, SEED0, A.DIFF_ALL, 8)
        ref_a, ref_b, ref_d = hip.run_campaign_diff(w, SEED0, TOTAL, max_listed=8, batch=batch, in_flight=in_flight, **kw)
        assert D.of_report(d) == D.of_report(ref_d) and d.records.tobytes() == ref_d.records.tobytes()
        assert report(rep_a) == report(ref_a) == report(hip.run_campaign(w, SEED0, TOTAL, batch, in_flight, False, cfgs["default"]))
        assert report(rep_b) == report(ref_b) == report(hip.run_campaign(w, SEED0, TOTAL, batch, in_flight, False, cfgs["lossy"]))
        without = hip.run_campaign_paired(w, SEED0, TOTAL, other_include=PASS_OR_DEADLOCK, top_k=2, batch=batch, in_flight=in_flight, **kw)
        assert image(without[2]) == img and report(without[0]) == report(rep_a) and report(without[1]) == report(rep_b)
    lst = hip.run_campaign_paired_seeds(w, np.arange(SEED0, SEED0 + TOTAL, dtype=np.uint64), other_include=PASS_OR_DEADLOCK, top_k=2, fields=A.DIFF_VERDICT,
                                        max_listed=4, batch=4096, **kw)
    assert D.of_report(lst[3]) == D.diff_truth(a, b, SEED0, A.DIFF_VERDICT, 4) and image(lst[2]) == img


def test_resolving(hip):
    """Side A under limits that make some first-pass seeds overflow (tests/test_campaign_resolve_gpu.py's jittery ping-pong), side B roomy and
    under another latency: with the flag the report is the truth over the per-seed ladder, and n_incomparable is what the ladder leaves."""
    w, cfg, lim, resolved, k, rungs, want = RG.jittery(hip, 4)
    roomy = A.Limits()
    roomy.heap_lds_slots, roomy.heap_spill_slots = 8, 64
    cfg_b = A.Config.default(packet_loss_rate=0.01, loss_table=(0.3,), lat_lo_ns=2_000_000, lat_hi_ns=10_000_000)
    b, _ = oracle.run_batch(w, RG.JSEED0, RG.JTOTAL, cfg_b, roomy)
    assert (b["verdict"] < A.OVERFLOW).all()                                                  # side B never needs a round
    first_runner = int((rungs[0]["verdict"] >= A.OVERFLOW).sum())
    assert first_runner > 1000 and (resolved["verdict"] < A.OVERFLOW).all()
    inc = (A.PASS, A.DEADLOCK)
    kw = dict(config=cfg, other_config=cfg_b, limits=lim, other_limits=roomy, include=inc, top_k=16)
    t = R.paired_truth(resolved, b, RG.JSEED0, 5, 5, 16)
    assert t["n_incomparable"] == 0 and t["n_paired"] > 8000 and t["clock_ns"]["dir"][R.UP]["n"] > 500
    first = None
    for batch, in_flight in ((RG.BATCH, 2), (1000, 3)):
        got = hip.run_campaign_paired(w, RG.JSEED0, RG.JTOTAL, resolve=True, batch=batch, in_flight=in_flight, **kw)
        img = check(got, resolved, b, RG.JSEED0, 5, 5, 16, ("resolved", batch))
        first = img if first is None else first
        assert img == first and got[2].n_incomparable == 0
        assert RG.report(got[0]) == RG.plain_truth(resolved, RG.JSEED0, batch) and RG.report(got[1]) == RG.plain_truth(b, RG.JSEED0, batch)
        assert RG.account(hip.campaign_resolved()) == RG.account_truth(k, rungs, resolved, lim, 4, batch)
    # two rounds: the seeds they leave unsettled, and no other, are incomparable — with a diff report beside it
    res2 = RG.jittery(hip, 2)[3]
    left = int((res2["verdict"] >= A.OVERFLOW).sum())
    assert 0 < left < first_runner
    got = hip.run_campaign_paired(w, RG.JSEED0, RG.JTOTAL, resolve=2, fields=A.DIFF_VERDICT, batch=1000, **kw)
    check(got, res2, b, RG.JSEED0, 5, 5, 16, "two rounds")
    assert got[2].n_incomparable == left == got[3].n_incomparable == got[0].n_runner
    # without the flag every first-pass runner verdict is incomparable
    got = hip.run_campaign_paired(w, RG.JSEED0, RG.JTOTAL, batch=RG.BATCH, **kw)
    check(got, rungs[0], b, RG.JSEED0, 5, 5, 16, "unresolved")
    assert got[2].n_incomparable == first_runner


def test_the_example(hip, truth):
    """examples/latency_shift_test.cpp, built and run the way tests/test_campaign_sweep_gpu.py builds loss_sweep_test: its printed counts, mean
    shift and worst regressions are the oracle's."""
    import os
    import re
    import subprocess
    w, cfgs, res = truth
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "examples", "latency_shift_test")
    subprocess.check_call(["g++", "-std=c++17", "-O2", os.path.join(root, "examples", "latency_shift_test.cpp"), "-o", exe,
                           "-L" + os.path.join(root, "madsim_amd"), "-lmadsim_hip", "-Wl,-rpath," + os.path.join(root, "madsim_amd")])
    p = subprocess.run([exe], env=dict(os.environ, MADSIM_TEST_SEED=str(SEED0), MADSIM_TEST_NUM=str(TOTAL)), capture_output=True, text=True, timeout=120)
    print(p.stdout, p.stderr)
    assert p.returncode == 0, (p.returncode, p.stdout, p.stderr)
    t = R.paired_truth(res["default"], res["slow"], SEED0, 1, 1, 3)
    assert re.search(r"%d seeds from %d, %d paired, 0 unpaired, 0 incomparable" % (TOTAL, SEED0, TOTAL), p.stdout)
    for name, (up, down, equal) in zip(R.METRICS, moved(t)):
        assert re.search(r"%s\s+up %d, down %d, equal %d\n" % (name, up, down, equal), p.stdout), name
    net = t["clock_ns"]["dir"][R.UP]["sum"] - t["clock_ns"]["dir"][R.DOWN]["sum"]
    assert "mean shift of clock_ns: %+.1f ns" % (net / TOTAL) in p.stdout
    listed = re.findall(r"seed (\d+): (\d+) ns -> (\d+) ns", p.stdout)
    assert [tuple(int(x) for x in e) for e in listed] == t["clock_ns"]["dir"][R.UP]["top"] and len(listed) == 3
