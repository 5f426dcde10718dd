"""Sweep campaigns on the MI355X: madsim_hip_run_sweep_campaign (and its context / several-contexts forms) against tests/sweep_ref.py's
sweep_truth over the CPU oracle's per-seed results of each variant — never against a second call of the code under test.  The fixture is
the four-node ping-pong at loss 0, 0.0005, 0.002 and 0.01 over 10 000 seeds: the oracle says 0 / 299 / 1 149 / 4 684 of them deadlock, in
failing sets that nest (asserted below, so no case passes vacuously)."""
import copy
import os
import re
import subprocess

import numpy as np
import pytest

import oracle
from madsim_amd import _abi as A
from tests import lifecycle_workloads as LW
from tests import sweep_ref as R
from tests.test_campaign_resolve_gpu import JSEED0, JTOTAL, account, account_truth, jittery, plain_truth
from tests.test_campaign_resolve_gpu import report as resolved_report

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE = (1 << 64) - 1
SEED0, TOTAL = R.SEED0, R.TOTAL
REPORT_FIELDS = ("seeds_run", "batches_run", "batches_launched", "first_failing_seed", "n_failed", "n_runner", "total_steps", "total_clock_ns")


def report(rep, skip=()):
    return {f: int(getattr(rep, f)) for f in REPORT_FIELDS if f not in skip}


@pytest.fixture(scope="module")
def truth():
    """The preconditions the file rests on, asserted on the oracle's results."""
    w, cfgs, res = R.four_configs()
    assert [int((r["verdict"] == A.DEADLOCK).sum()) for r in res] == list(R.FAILURES) == [int((r["verdict"] != A.PASS).sum()) for r in res]
    t = R.sweep_truth(res, SEED0, A.DIFF_ALL, R.MIXED, 0)
    assert {m: c for m, c in enumerate(t["n_by_mask"]) if c} == R.MASKS and t["n_incomparable"] == 0
    assert t["n_differ_from_first"] == list(R.FAILURES) + [0] * 4
    mixed = R.selected(*R.classify(res, A.DIFF_VERDICT), R.MIXED, 4)
    assert [int(mixed[k:k + 1000].sum()) for k in (0, 1000)] == [469, 470]
    return w, cfgs, res


def variants_of(w, cfgs, lims=None):
    return [(w, c, lims[v] if lims else None) for v, c in enumerate(cfgs)]


def check(got, res, seeds, fields, rule, cap, what):
    reps, sw = got
    want, have = R.sweep_truth(res, seeds, fields, rule, cap), R.of_report(sw)
    print(what, "selected", have["n_selected"], want["n_selected"], "listed", have["n_listed"], want["n_listed"], "masks",
          {m: c for m, c in enumerate(have["n_by_mask"]) if c})
    assert have == want, what
    assert (sw.fields, sw.list_rule, sw.max_listed, sw.n_variants) == (fields, rule, cap, len(res)) and len(reps) == len(res)
    for v, rep in enumerate(reps):                                                       # the plain report of each variant, seen in the counts
        assert int(rep.seeds_run) == len(res[0]) == sw.n_settled + sw.n_incomparable
        assert int(rep.n_runner) == int(sw.n_runner_by_variant[v])
        if sw.n_incomparable == 0:
            assert int(rep.n_failed) == sw.fails(v)
    return sw.records.tobytes()


def test_the_four_loss_rates_whatever_the_cut(hip, truth):
    """batch, batches in flight, the default context, a context, one and two contexts: the whole struct is the truth, and the same bytes."""
    w, cfgs, res = truth
    variants = variants_of(w, cfgs)
    plain = {}
    for fields, rule, cap in ((A.DIFF_ALL, "mixed", 64), (A.DIFF_VERDICT, "failing", R.FAILURES[3] + 10), (A.DIFF_OBS | A.DIFF_STEPS, "differing", 0)):
        rule_n = A.SWEEP_LIST_NAMES.index(rule)
        kw = dict(fields=fields, list_rule=rule, max_listed=cap)
        first = None
        for batch, in_flight in ((1000, 3), (4096, 1), (10_000, 2)):
            got = hip.run_campaign_sweep(variants, SEED0, TOTAL, batch=batch, in_flight=in_flight, **kw)
            recs = check(got, res, SEED0, fields, rule_n, cap, (fields, rule, cap, batch, in_flight))
            first = recs if first is None else first
            assert recs == first
            assert got[1].nested() and got[1].first_failing().tolist() == [0, 299, 850, 3535]
            for v, cfg in enumerate(cfgs):                                               # each variant's report: the plain campaign's for that config
                if (v, batch, in_flight) not in plain:
                    plain[v, batch, in_flight] = report(hip.run_campaign(w, SEED0, TOTAL, batch, in_flight, False, cfg))
                assert report(got[0][v]) == plain[v, batch, in_flight], (v, batch, in_flight)
                assert got[0][v].kernel_ms > 0 and got[0][v].wall_s > 0
        with hip.Context(0) as c0, hip.Context(0) as c1:
            for batch, in_flight in ((1000, 3), (4096, 1), (10_000, 2)):
                got = c0.run_campaign_sweep(variants, SEED0, TOTAL, batch=batch, in_flight=in_flight, **kw)
                assert check(got, res, SEED0, fields, rule_n, cap, ("context form", batch, in_flight)) == first
                got = hip.run_campaign_sweep_multi([c0, c1], variants, SEED0, TOTAL, batch=batch, in_flight=in_flight, **kw)
                assert check(got, res, SEED0, fields, rule_n, cap, ("two contexts", batch, in_flight)) == first
                assert report(got[0][3], ("batches_launched",)) == {k: v for k, v in plain[3, batch, in_flight].items() if k != "batches_launched"}


def test_stop_at_sweep(hip, truth):
    """"Show me 500 seeds the rates disagree on" at batch 1 000: the first batch holds 469 mixed seeds and the second 470, so two batches are
    read; everything reported is the prefix's."""
    w, cfgs, res = truth
    variants = variants_of(w, cfgs)
    with hip.Context(0) as c0, hip.Context(0) as c1:
        for ctxs in ([c0], [c0, c1]):
            reps, sw = got = hip.run_campaign_sweep_multi(ctxs, variants, SEED0, TOTAL, max_listed=500, stop_at_listed=True, batch=1000, in_flight=3)
            for rep in reps:
                assert rep.seeds_run == 2000 and rep.batches_run == 2
                assert rep.batches_launched >= rep.batches_run and rep.batches_launched == reps[0].batches_launched
            check(got, [r[:2000] for r in res], SEED0, A.DIFF_VERDICT, R.MIXED, 500, ("stop at sweep", len(ctxs)))
            assert len(sw) == 500 and sw.n_selected == 469 + 470
            assert sw.records.tobytes() == R.sweep_truth(res, SEED0, A.DIFF_VERDICT, R.MIXED, 500)["records"]      # ... which are the whole range's first 500
    # without the flag the same call runs to the end; the other stop flags mean nothing to this form
    reps, sw = hip.run_campaign_sweep(variants, SEED0, TOTAL, max_listed=500, batch=1000, in_flight=3)
    assert reps[0].seeds_run == TOTAL and len(sw) == 500 and sw.n_selected == TOTAL - R.MASKS[0]


def test_the_list_form(hip, truth):
    """Over the 4 684 seeds failing at loss 0.01: the truth over those rows; a dense list gives the range call's bytes."""
    w, cfgs, res = truth
    variants = variants_of(w, cfgs)
    idx = np.nonzero(res[3]["verdict"] != A.PASS)[0]
    assert len(idx) == R.FAILURES[3]
    seeds = (idx + SEED0).astype(np.uint64)
    rows = [r[idx] for r in res]
    first = None
    with hip.Context(0) as c0, hip.Context(0) as c1:
        for call in (lambda **kw: hip.run_campaign_sweep(variants, seeds=seeds, **kw), lambda **kw: c0.run_campaign_sweep(variants, seeds=seeds, **kw),
                     lambda **kw: hip.run_campaign_sweep_multi([c0, c1], variants, seeds=seeds, **kw)):
            for batch, in_flight in ((1000, 3), (4096, 1)):
                got = call(fields=A.DIFF_ALL, list_rule="mixed", max_listed=5000, batch=batch, in_flight=in_flight)
                recs = check(got, rows, seeds, A.DIFF_ALL, R.MIXED, 5000, ("list", batch, in_flight))
                first = recs if first is None else first
                assert recs == first and got[1].only(3) == R.MASKS[8] and got[1].n_by_mask[0] == 0
                assert got[0][3].n_failed == len(seeds) and got[0][0].n_failed == 0
    dense = np.arange(SEED0, SEED0 + 3000, dtype=np.uint64)
    for rule in ("mixed", "differing"):
        a = hip.run_campaign_sweep(variants, seeds=dense, fields=A.DIFF_ALL, list_rule=rule, max_listed=100, batch=1024, in_flight=2)
        b = hip.run_campaign_sweep(variants, SEED0, 3000, fields=A.DIFF_ALL, list_rule=rule, max_listed=100, batch=1024, in_flight=2)
        assert R.of_report(a[1]) == R.of_report(b[1]) == R.sweep_truth([r[:3000] for r in res], SEED0, A.DIFF_ALL, A.SWEEP_LIST_NAMES.index(rule), 100)
        assert [report(x) for x in a[0]] == [report(x) for x in b[0]]
    reps, sw = hip.run_campaign_sweep(variants, seeds=[], max_listed=4)                          # an empty list: nothing
    assert [int(r.seeds_run) for r in reps] == [0] * 4 and len(sw) == 0 and sw.n_settled == 0


def test_small_ranges_and_argument_errors(hip, truth):
    w, cfgs, res = truth
    variants = variants_of(w, cfgs)
    first = int(np.nonzero(res[3]["verdict"] == A.DEADLOCK)[0][0])
    for at, total in ((first, 1), (0, 1), (0, 65), (max(first - 3, 0), 700)):
        got = hip.run_campaign_sweep(variants[2:], SEED0 + at, total, fields=A.DIFF_ALL, list_rule="failing", max_listed=4)      # V = 2, total < batch
        check(got, [r[at:at + total] for r in res[2:]], SEED0 + at, A.DIFF_ALL, R.FAILING, 4, (at, total))
    eight = [variants[v % 4] for v in range(8)]                                                  # V = 8: every pointer repeats
    got = hip.run_campaign_sweep(eight, SEED0, 2500, fields=A.DIFF_ALL, list_rule="differing", max_listed=30, batch=1000)
    check(got, [res[v % 4][:2500] for v in range(8)], SEED0, A.DIFF_ALL, R.DIFFERING, 30, "eight variants")
    reps, sw = hip.run_campaign_sweep(variants, SEED0, 0, max_listed=4)                          # no seeds: nothing
    assert [int(r.seeds_run) for r in reps] == [0] * 4 and len(sw) == 0 and int(sw.n_by_mask.sum()) == 0
    for bad in (dict(fields=128), dict(list_rule="differing", fields=0), dict(max_listed=0, stop_at_listed=True), dict(in_flight=9)):
        with pytest.raises(hip.MadsimHipError):
            hip.run_campaign_sweep(variants, SEED0, 1000, **bad)
    with hip.Context(0) as c0:
        with pytest.raises(hip.MadsimHipError):
            hip.run_campaign_sweep_multi([c0, c0], variants, SEED0, 1000)                        # the same context twice
        with pytest.raises(hip.MadsimHipError):
            c0.run_campaign_sweep(variants, NONE - 5, 1000)                                      # seed0 + total wraps


@pytest.mark.parametrize("name", ["kill_restart_with_traffic"])
def test_build_against_build_in_one_call(hip, name):
    """One workload under LDS, global and global + narrow-heap state, V = 3 under ALL: the same 48 bytes for every seed, in one campaign."""
    w, cfg = getattr(LW, name)(), LW.config(name)
    total = 3000
    want, _ = oracle.run_batch(w, 1000, total, cfg or A.Config.default())

    def lim(state_mem):
        x = copy.copy(LW.limits(name) or A.Limits())
        x.state_mem, x.lanes_per_wave = state_mem, 0
        return x
    builds = [lim(A.STATE_LDS), lim(A.STATE_GLOBAL), lim(A.STATE_GLOBAL | A.STATE_NARROW_HEAP)]
    geo = [hip.geometry(w, b).variant for b in builds]
    assert not geo[0] & 16 and geo[1] & 16 and geo[2] & 16 and geo[2] & 0x8000 and not geo[1] & 0x8000, geo
    reps, sw = got = hip.run_campaign_sweep([(w, cfg, b) for b in builds], 1000, total, fields=A.DIFF_ALL, list_rule="differing", max_listed=4, batch=1024)
    print(name, "incomparable", sw.n_incomparable, "differ", sw.n_differ_from_first.tolist(), sw.records)
    assert not sw.n_differ_from_first.any() and sw.n_selected == 0 and len(sw) == 0 and sw.n_settled + sw.n_incomparable == total
    assert report(reps[0]) == report(reps[1]) == report(reps[2])
    if sw.n_incomparable == 0:                                                           # (no capacity verdict in any build: the oracle's counts)
        check(got, [want, want, want], 1000, A.DIFF_ALL, R.DIFFERING, 4, name)
        assert all(int(r.n_failed) == int(((want["verdict"] >= 1) & (want["verdict"] < 4)).sum()) for r in reps)


def test_resolve(hip):
    """Variant 0 = the tight limits, variant 1 = roomy ones, one workload, every field.  Without the flag every first-pass runner verdict is
    incomparable; with it the report is the truth over the resolved arrays and the account is the ladder's."""
    w, cfg, lim, resolved, k, rungs, want = jittery(hip, 4)
    roomy = A.Limits()
    roomy.heap_lds_slots, roomy.heap_spill_slots = 8, 64
    b, _ = oracle.run_batch(w, JSEED0, JTOTAL, cfg, roomy)
    assert (b["verdict"] < A.OVERFLOW).all()                                             # variant 1 never needs a round
    first_runner = int((rungs[0]["verdict"] >= A.OVERFLOW).sum())
    assert first_runner > 1000                                                           # the first pass does leave runner verdicts
    variants = [(w, cfg, lim), (w, cfg, roomy)]
    reps, sw = got = hip.run_campaign_sweep(variants, JSEED0, JTOTAL, fields=A.DIFF_ALL, list_rule="differing", max_listed=8, batch=4096)
    check(got, [rungs[0], b], JSEED0, A.DIFF_ALL, R.DIFFERING, 8, "first pass")
    assert sw.n_incomparable == first_runner == int(sw.n_runner_by_variant[0]) == reps[0].n_runner and sw.n_runner_by_variant[1] == 0
    assert bytes(hip.campaign_resolved()) == bytes(112)
    for batch, in_flight in ((4096, 2), (1000, 3)):
        reps, sw = got = hip.run_campaign_sweep(variants, JSEED0, JTOTAL, fields=A.DIFF_ALL, list_rule="differing", max_listed=8, batch=batch,
                                                in_flight=in_flight, resolve=True)
        check(got, [resolved, b], JSEED0, A.DIFF_ALL, R.DIFFERING, 8, ("resolved", batch, in_flight))
        assert resolved_report(reps[0]) == plain_truth(resolved, JSEED0, batch) and resolved_report(reps[1]) == plain_truth(b, JSEED0, batch)
        assert account(hip.campaign_resolved()) == account_truth(k, rungs, resolved, lim, 4, batch)
    # both variants tight: each is resolved under its own limits, and the account sums them
    reps, sw = hip.run_campaign_sweep([variants[0], variants[0]], JSEED0, JTOTAL, fields=A.DIFF_ALL, list_rule="differing", batch=4096, resolve=4)
    one, both = account_truth(k, rungs, resolved, lim, 4, 4096), account(hip.campaign_resolved())
    assert sw.n_selected == 0 and resolved_report(reps[0]) == resolved_report(reps[1]) == plain_truth(resolved, JSEED0, 4096)
    assert both["n_first_pass"] == 2 * one["n_first_pass"] and both["n_by_round"] == [2 * x for x in one["n_by_round"]]
    assert both["batches_resolved"] == 2 * one["batches_resolved"] and both["n_resolved"] == 2 * one["n_resolved"]


def test_the_loss_sweep_example(hip, truth):
    """examples/loss_sweep_test.cpp, built and run the way tests/test_campaign_seeds_gpu.py builds corpus_test: its printed failures and masks
    are the oracle's."""
    w, cfgs, res = truth
    exe = os.path.join(ROOT, "examples", "loss_sweep_test")
    subprocess.check_call(["g++", "-std=c++17", "-O2", os.path.join(ROOT, "examples", "loss_sweep_test.cpp"), "-o", exe,
                           "-L" + os.path.join(ROOT, "madsim_amd"), "-lmadsim_hip", "-Wl,-rpath," + os.path.join(ROOT, "madsim_amd")])
    p = subprocess.run([exe], env=dict(os.environ, MADSIM_TEST_SEED=str(SEED0), MADSIM_TEST_NUM=str(TOTAL)), capture_output=True, text=True, timeout=120)
    print(p.stdout, p.stderr)
    assert p.returncode == 0, (p.returncode, p.stdout, p.stderr)
    assert re.search(r"%d seeds from %d under loss .*, 0 incomparable" % (TOTAL, SEED0), p.stdout)
    assert re.search(r"failures per rate: %d %d %d %d\n" % R.FAILURES, p.stdout)
    assert {int(m): int(c) for c, m in re.findall(r"(\d+) seeds \(mask (\d+)\)", p.stdout)} == R.MASKS
    assert "the failing sets nest: yes" in p.stdout
    t = R.sweep_truth(res, SEED0, A.DIFF_VERDICT, R.MIXED, 8)
    recs = np.frombuffer(t["records"], dtype=A.SWEEP_RECORD_DTYPE)
    names = ("pass", "panic", "deadlock", "time-limit")
    listed = re.findall(r"seed (\d+): (\S+) / (\S+) / (\S+) / (\S+)\n", p.stdout)
    assert listed == [(str(int(r["seed"])),) + tuple(names[x] for x in r["verdict"][:4]) for r in recs] and len(listed) == 8
    assert "... and %d more" % (t["n_selected"] - 8) in p.stdout
