"""One context through every campaign form, one after the other, on the MI355X: each step either enlarges a buffer the step before it left in
the context's flights or reuses one that is larger than it needs, and every answer must be the one the session's default context gives to the
same call (that context is held against the oracle by the other files).  Then the context is closed, a second one opened on the same device,
and it answers alike.  The range is the traced lossy ping-pong of tests/test_campaign_groups_gpu.py; the resolving step uses the workload and
limits of tests/test_campaign_resolve_gpu.py's test_everything_overflows_and_one_round_settles_all."""
import numpy as np
import pytest

from madsim_amd import _abi as A
from madsim_amd import workload as W
from tests import groups_ref as G
from tests import stats_ref as R
from tests.test_campaign_groups_gpu import REPORT_FIELDS, SEED0, TOTAL

pytestmark = pytest.mark.gpu

ACCOUNT_FIELDS = ("n_first_pass", "n_resolved", "n_unresolved", "batches_resolved", "rounds", "reserved")


def report(rep):
    return {f: int(getattr(rep, f)) for f in REPORT_FIELDS}


def trace(t):
    return (t.seed, bytes(t.result), t.observations, t.n_observations, t.log, t.log_len)


def divergence(d):
    return tuple(bytes(v) if isinstance(v, A.Result) else v for v in (getattr(d, name) for name in type(d).__slots__))


def diff(out):
    rep_a, rep_b, d = out
    return (report(rep_a), report(rep_b), d.records.tobytes(), d.n_compared, d.n_incomparable, d.n_differ, d.n_by_field.tobytes(), d.transitions.tobytes())


def test_one_context_through_every_form_then_a_second_one(hip):
    w, cfg, _ = G.traced_pingpong()
    c = hip.Context(0)
    try:
        # 1. the plain campaign: small batches, more and larger ones, then small ones on buffers that stay large
        for batch, in_flight in ((64, 1), (1000, 3), (4096, 5), (64, 2)):
            assert report(c.run_campaign(w, SEED0, TOTAL, batch, in_flight, False, cfg)) == report(hip.run_campaign(w, SEED0, TOTAL, batch, in_flight, False, cfg))
        # 2. collecting: a short list, then a longer one
        for cap in (4, 64):
            got, want = c.run_campaign(w, SEED0, TOTAL, 1000, 3, False, cfg, collect=cap), hip.run_campaign(w, SEED0, TOTAL, 1000, 3, False, cfg, collect=cap)
            assert report(got[0]) == report(want[0]) and got[1].tobytes() == want[1].tobytes() and len(got[1]) == cap and (got[2] == want[2]).all()
        # 3. statistics: without extreme seeds, then with them
        for top_k in (0, 16):
            got = c.run_campaign_stats(w, SEED0, TOTAL, 1000, 3, False, cfg, include=(A.PASS, A.DEADLOCK), top_k=top_k)
            want = hip.run_campaign_stats(w, SEED0, TOTAL, 1000, 3, False, cfg, include=(A.PASS, A.DEADLOCK), top_k=top_k)
            assert report(got[0]) == report(want[0]) and R.same(R.of_stats(got[1]), R.of_stats(want[1])) and got[1].n > 0
        # 4. grouping: a table for batches of 1 000, then one for 4 096
        for batch in (1000, 4096):
            got, want = c.run_campaign_groups(w, SEED0, TOTAL, batch, 3, False, cfg, max_groups=8), hip.run_campaign_groups(w, SEED0, TOTAL, batch, 3, False, cfg, max_groups=8)
            assert report(got[0]) == report(want[0]) and got[1].groups.tobytes() == want[1].groups.tobytes() and len(got[1]) == 3
            assert (got[1].n_grouped, got[1].n_ungrouped) == (want[1].n_grouped, want[1].n_ungrouped)
        # 5. differential, both sides the same
        for batch in (1000, 4096):
            got = diff(c.run_campaign_diff(w, SEED0, TOTAL, config=cfg, max_listed=16, batch=batch, in_flight=3))
            assert got == diff(hip.run_campaign_diff(w, SEED0, TOTAL, config=cfg, max_listed=16, batch=batch, in_flight=3))
            assert got[3:6] == (TOTAL, 0, 0)
        # 6. a resolving list campaign: every listed seed overflows the first pass and one round settles it
        wo = W.pingpong(4, 16)
        lim = A.Limits(); lim.heap_lds_slots, lim.heap_spill_slots = 2, 0
        seeds = np.arange(50, dtype=np.uint64) * 241 + np.arange(50, dtype=np.uint64) % 7
        got = c.run_campaign_seeds(wo, seeds, 16, 2, False, None, lim, collect=50, list_runner=True, resolve=True)
        acct = c.campaign_resolved()
        want = hip.run_campaign_seeds(wo, seeds, 16, 2, False, None, lim, collect=50, list_runner=True, resolve=True)
        assert report(got[0]) == report(want[0]) and got[1].tobytes() == want[1].tobytes() and (got[2] == want[2]).all()
        assert [getattr(acct, f) for f in ACCOUNT_FIELDS] == [getattr(hip.campaign_resolved(), f) for f in ACCOUNT_FIELDS]
        assert list(acct.n_by_round) == list(hip.campaign_resolved().n_by_round)
        assert (acct.n_first_pass, acct.n_resolved, got[0].n_runner, int(got[2][A.PASS])) == (50, 50, 0, 50)
        # 7. traces: one seed with small rows, then eight with larger ones; 8. where the two (equal) sides of those eight part
        one, eight = [SEED0 + 3], [SEED0 + 1000 * i + i for i in range(8)]
        for listed, obs_cap, log_cap in ((one, 1, 16), (eight, 8, 4096)):
            got = c.trace_seeds(w, listed, cfg, obs_cap=obs_cap, log_cap=log_cap, resolve=None)
            want = hip.trace_seeds(w, listed, cfg, obs_cap=obs_cap, log_cap=log_cap, resolve=None)
            assert [trace(t) for t in got] == [trace(t) for t in want] and all(t.log_len > 0 for t in got)
        got, want = c.diverge_seeds(w, eight, config=cfg, log_cap=4096, obs_cap=8, resolve=None), hip.diverge_seeds(w, eight, config=cfg, log_cap=4096, obs_cap=8, resolve=None)
        assert [divergence(d) for d in got] == [divergence(d) for d in want] and all(d.log_status in (A.DIVERGE_SAME, A.DIVERGE_BEYOND_CAP) for d in got)
        # 9. per-seed results of 98 305 + 1 seeds: beyond the one-launch limit (98 304), so through the flights' page-locked staging
        count = 98_305 + 1
        (got, gs), (want, ws) = c.run_batch(w, SEED0, count, cfg), hip.run_batch(w, SEED0, count, cfg)
        assert got.tobytes() == want.tobytes()
        assert all(getattr(gs, f) == getattr(ws, f) for f in ("first_failing_seed", "n_failed", "total_steps", "total_clock_ns")) and gs.n_failed > 0
    finally:
        c.close()
    with hip.Context(0) as c2:                                   # everything was released with the first one: a second one starts from nothing
        assert report(c2.run_campaign(w, SEED0, TOTAL, 1000, 3, False, cfg)) == report(hip.run_campaign(w, SEED0, TOTAL, 1000, 3, False, cfg))
