"""The differential, paired and sweep campaigns share one driver (run_variants_impl, madsim_hip.cpp) and one flight group: the results of
variants 1 .. 7, an event pair per variant and the report words with their initial state behind them.  What that sharing makes possible
is one form inheriting another's state — words a longer form left behind a shorter one's, a batch's results of a variant the next call does
not run, a re-run's buffers.  So: a sequence of calls of every form on ONE context, each held byte for byte against the same call on a
fresh context of its own, and the differential and the sweep call also against the truth over the CPU oracle's per-seed results.

The range is the four-node ping-pong with 8 rounds over 3 000 seeds: side / variant 0 at loss 0, the others at the loss rates of
tests/diff_ref.py and tests/sweep_ref.py, under which the range holds passing and deadlocking seeds (asserted on the oracle's results)."""
import numpy as np
import pytest

import oracle
from madsim_amd import _abi as A
from madsim_amd import workload as W
from tests import diff_ref as D
from tests import sweep_ref as S
from tests.test_campaign_paired_gpu import image as paired_image
from tests.test_campaign_resolve_gpu import account

pytestmark = pytest.mark.gpu

SEED0, TOTAL = D.SEED0, 3000
REPORT_FIELDS = ("seeds_run", "batches_run", "batches_launched", "first_failing_seed", "n_failed", "n_runner", "total_steps", "total_clock_ns")


def report(rep):
    """A madsim_campaign_t but for kernel_ms and wall_s."""
    return {f: int(getattr(rep, f)) for f in REPORT_FIELDS}


def diff_image(got):
    rep_a, rep_b, d = got
    return report(rep_a), report(rep_b), (d.fields, d.max_listed), D.of_report(d)


def sweep_image(got):
    reps, sw = got
    return [report(r) for r in reps], (sw.fields, sw.list_rule, sw.max_listed, sw.n_variants), S.of_report(sw)


def paired_image_of(got):
    return (report(got[0]), report(got[1]), paired_image(got[2])) + ((D.of_report(got[3]),) if len(got) > 3 else ())


@pytest.fixture(scope="module")
def fixture():
    """(workload, the four configs, the oracle's results under each — read-only)."""
    w = W.pingpong(4, 8)
    cfgs = [A.Config.default(packet_loss_rate=p) if p else A.Config.default() for p in S.LOSSES]
    res = [oracle.run_batch(w, SEED0, TOTAL, c)[0] for c in cfgs]
    for r in res:
        r.setflags(write=False)
    dead = [int((r["verdict"] == A.DEADLOCK).sum()) for r in res]
    print("deadlocks per loss rate", dead)
    assert dead[0] == 0 and all(0 < n < TOTAL for n in dead[1:]) and all(set(r["verdict"].tolist()) <= {A.PASS, A.DEADLOCK} for r in res)
    assert S.LOSSES[2] == D.LOSS
    return w, cfgs, res


def calls(w, cfgs, limits=(None,) * 4, resolve=None):
    """[(name, image of c's call)]: the sequence, as functions of the context that runs it."""
    two = dict(config=cfgs[0], other_config=cfgs[2], limits=limits[0], other_limits=limits[1])
    variants = [(w, c, limits[v]) for v, c in enumerate(cfgs)]
    inc = dict(include=(A.PASS,), other_include=(A.PASS, A.DEADLOCK))

    def diff(c):
        return diff_image(c.run_campaign_diff(w, SEED0, TOTAL, fields=A.DIFF_ALL, max_listed=8, batch=1000, in_flight=2, resolve=resolve, **two))

    def sweep(c):
        return sweep_image(c.run_campaign_sweep(variants, SEED0, TOTAL, fields=A.DIFF_ALL, list_rule="mixed", max_listed=8, batch=257, in_flight=3,
                                                resolve=resolve))

    def paired_top(c):
        return paired_image_of(c.run_campaign_paired(w, SEED0, TOTAL, top_k=16, fields=A.DIFF_ALL, max_listed=8, batch=1000, resolve=resolve, **inc, **two))

    def paired_bare(c):
        return paired_image_of(c.run_campaign_paired(w, SEED0, TOTAL, top_k=0, batch=64, resolve=resolve, **inc, **two))

    return diff, sweep, paired_top, paired_bare


def fresh(hip, call, with_account=False):
    with hip.Context(0) as c:
        img = call(c)
        return (img, resolve_account(c)) if with_account else img


def resolve_account(c):
    """campaign_resolved() but for rerun_kernel_ms."""
    return account(c.campaign_resolved())


def test_one_context_through_every_form(hip, fixture):
    """diff, a four-variant sweep, paired with top records and a diff report, paired without either, the first diff again — all on one context:
    every call's reports and records are those of the same call on a fresh context, the diff and the sweep are the oracle's, and call 5 is call 1."""
    w, cfgs, res = fixture
    diff, sweep, paired_top, paired_bare = calls(w, cfgs)
    with hip.Context(0) as c:
        got = [(f.__name__, f(c)) for f in (diff, sweep, paired_top, paired_bare, diff)]
    for (name, img), f in zip(got, (diff, sweep, paired_top, paired_bare, diff)):
        want = fresh(hip, f)
        print(name, "same as on a fresh context:", img == want)
        assert img == want, name
    assert got[4][1] == got[0][1]
    assert got[0][1][3] == D.diff_truth(res[0], res[2], SEED0, A.DIFF_ALL, 8)
    assert got[1][1][2] == S.sweep_truth(res, SEED0, A.DIFF_ALL, S.MIXED, 8)
    assert got[2][1][3] == got[0][1][3]                                    # the paired call's diff report is the differential call's
    assert got[2][1][2] != got[3][1][2]                                    # (top records or none: the two paired images do differ)


def test_one_context_through_the_resolving_forms(hip, fixture):
    """The diff and the sweep with resolve=2 under tests/test_campaign_resolve_gpu.py::test_the_differential_form's limits — side A and the
    even variants tight, the others roomy —, one after the other on one context: reports, records and the resolve account (but for
    rerun_kernel_ms) are those of fresh contexts, and the diff once more is the diff."""
    w, cfgs, _ = fixture
    tight, roomy = A.Limits(), A.Limits()
    tight.heap_lds_slots, tight.heap_spill_slots = 2, 1
    roomy.heap_lds_slots, roomy.heap_spill_slots = 8, 64
    diff, sweep = calls(w, cfgs, (tight, roomy, tight, roomy), resolve=2)[:2]
    with hip.Context(0) as c:
        got = [(f.__name__, f(c), resolve_account(c)) for f in (diff, sweep, diff)]
    for (name, img, acct), f in zip(got, (diff, sweep, diff)):
        want = fresh(hip, f, with_account=True)
        print(name, "account", acct, "same as on a fresh context:", (img, acct) == want)
        assert acct["n_first_pass"] > 0 and acct["rounds"] == 2, (name, "no seed overflowed on the first pass: the leg checks nothing")
        assert (img, acct) == want, name
    assert got[2][1:] == got[0][1:]
