"""The device AT and OVER the ceilings of its workload model, and at the top of its largest state region (MI355X).

Every comparison is on all 48 bytes of every seed against tests/parity.py `expected()`: the oracle run with the model's ceilings OFF, the
verdict derived from the event mask.  No seed is left out, no tolerance applies.
 1. at the limit — every directed workload of tests/lifecycle_workloads.py that stands AT a ceiling (the oracle's bytes, no runner verdict)
    and one OVER it (MADSIM_UNSUPPORTED, every other field 0, the same after run_batch_auto), under the workload's own limits, in the LDS
    layout where the geometry admits it and in global state;
 2. the seam — the same workloads from the default limits, so that run_batch_auto climbs from MADSIM_OVERFLOW to the ceiling and the verdict
    changes its kind there (or the seed settles just below);
 3. the base-op mailbox, whose 128th message stays a capacity verdict at every capacity;
 4. a batch in which every second lane leaves the model, through every campaign form;
 5. the top of the 4 GiB global-state region: the largest per-seed block at the largest lane count the library admits.
Left out on purpose: the heap-spill region.  It has the same 4 GiB rule, but reaching its top slots needs thousands of live timers per seed on
65 536 lanes, and no workload in the tree does that in seconds."""
import copy
import functools

import numpy as np
import pytest

from madsim_amd import _abi as A
from tests import lifecycle_workloads as LW
from tests import parity
from tests import sweep_ref
from tests.test_campaign_diff_gpu import check as check_diff
from tests.test_campaign_resolve_gpu import account, account_truth, ladder, plain_truth
from tests.test_campaign_resolve_gpu import report as plain_report
from tests.test_campaign_sweep_gpu import check as check_sweep
from tests.test_collect_gpu import check as check_collect
from tests.test_collect_gpu import listed
from tests.test_oracle_model_limits import two_ctrl_c_waiters

pytestmark = pytest.mark.gpu

NONE = (1 << 64) - 1
SEED0, COUNT = 7_000, 96                                   # a wave and a half, from a non-zero seed

PAIRS = LW.model_edge_pairs()
BASE_AT, BASE_OVER, BASE_LIM = LW.base_op_mailbox_pair()
AT = LW.model_at_ceiling_workloads() + [(name + "_at", w_at, lim, 0) for name, w_at, _, lim, _ in PAIRS] + [("base_op_mailbox_127", BASE_AT, BASE_LIM, 0)]
OVER = LW.model_ceiling_workloads() + LW.model_exactly_one_over_workloads() + [(name + "_over", w_over, lim, bit) for name, _, w_over, lim, bit in PAIRS] + [two_ctrl_c_waiters()]
# the ceilings of max_tasks, mbox_regs, mbox_msgs and chan_queue: from the defaults the first pass must be a capacity verdict on every seed
CLIMBS = {"spawn_storm_254_tasks", "spawn_storm_255_tasks", "registrations_255", "registrations_256", "rxseq_128_receives",
          "rxseq_wraps_onto_dead_registration", "queued_messages_255", "queued_messages_256", "fifteen_queued_payloads", "sixteenth_queued_payload",
          "spawn_storm_exactly_255_tasks", "registrations_exactly_256", "base_op_mailbox_127"}


def with_state(lim, state_mem):
    g = copy.copy(lim) if lim is not None else A.Limits()
    g.state_mem, g.lanes_per_wave = state_mem, 0
    return g


def layouts(hip, w, lim):
    """The workload's own limits in the LDS layout — where the geometry admits it: the refusal must be the one about LDS — and in global state."""
    out = []
    try:
        hip.geometry(w, with_state(lim, A.STATE_LDS))
        out.append(("lds", with_state(lim, A.STATE_LDS)))
    except hip.MadsimHipError as e:
        assert "LDS" in str(e), e
    out.append(("global", with_state(lim, A.STATE_GLOBAL)))
    return out


@functools.lru_cache(maxsize=None)
def expected(name):
    """The oracle's answer for the case `name` over the test's seeds, computed once (it does not depend on the capacities)."""
    _, w, lim, _ = next(c for c in AT + OVER if c[0] == name)
    want = parity.expected(w, SEED0, COUNT, None, lim or A.Limits())
    want.setflags(write=False)
    return want


@pytest.mark.parametrize("case", AT, ids=lambda c: c[0])
def test_at_the_ceiling_the_device_gives_the_oracles_bytes(hip, case):
    name, w, lim, _ = case
    want = expected(name)
    assert (want["verdict"] == A.PASS).all()
    for layout, l in layouts(hip, w, lim):
        got, _ = hip.run_batch(w, SEED0, COUNT, None, l)
        print(name, layout, "verdicts", np.bincount(got["verdict"], minlength=8).tolist())
        assert not (got["verdict"] >= A.OVERFLOW).any(), (name, layout, got[got["verdict"] >= A.OVERFLOW][0])
        assert (got == want).all(), (name, layout, got[got != want][0], want[got != want][0])


@pytest.mark.parametrize("case", OVER, ids=lambda c: c[0])
def test_one_over_the_ceiling_is_unsupported_and_stays_so(hip, case):
    name, w, lim, _ = case
    want = expected(name)
    assert (want["verdict"] == A.UNSUPPORTED).all() and not any(want[f].any() for f in want.dtype.names[1:])      # every other field 0
    for layout, l in layouts(hip, w, lim):
        got, _ = hip.run_batch(w, SEED0, COUNT, None, l)
        print(name, layout, "verdicts", np.bincount(got["verdict"], minlength=8).tolist())
        assert not (got["verdict"] == A.INTERNAL).any()
        assert (got == want).all(), (name, layout, got[got != want][0])
        auto, _ = hip.run_batch_auto(w, SEED0, COUNT, None, l, max_rounds=8)
        assert (auto == want).all(), (name, layout, "after run_batch_auto", auto[auto != want][0])


@pytest.mark.parametrize("case", AT + OVER, ids=lambda c: c[0])
def test_the_seam_from_the_default_limits(hip, case):
    """From madsim_limits_t's defaults run_batch_auto doubles the capacities up to their ceilings: a seed AT a ceiling settles there with the
    oracle's bytes, a seed one OVER it changes from MADSIM_OVERFLOW to MADSIM_UNSUPPORTED at the last rung."""
    name, w, _, _ = case
    want = expected(name)
    for state_mem in (A.STATE_AUTO, A.STATE_GLOBAL):
        lim = with_state(None, state_mem)
        first, _ = hip.run_batch(w, SEED0, COUNT, None, lim)
        n_ovf = int((first["verdict"] == A.OVERFLOW).sum())
        print(name, "state_mem", state_mem, "first-pass MADSIM_OVERFLOW", n_ovf, "of", COUNT)
        assert not (first["verdict"] == A.INTERNAL).any()
        if name in CLIMBS:
            assert n_ovf == COUNT, (name, state_mem, "the seam was not walked", np.bincount(first["verdict"], minlength=8))
        final, want2 = parity.gpu_compare(hip, w, SEED0, COUNT, None, lim, what=(name, state_mem))
        assert (want2 == want).all() and (final == want).all()


def test_base_op_mailbox_128th_message_stays_a_capacity_verdict(hip):
    """A workload without extended ops keeps 7 bits of queued messages per mailbox: 127 datagrams pass with the oracle's bytes, the 128th is
    MADSIM_OVERFLOW at every capacity and after run_batch_auto (include/madsim_hip.h) — never a wrong result, never MADSIM_UNSUPPORTED, never
    a failed call.  Not through parity.compare: its "beyond the ceilings" rule does not know this capacity.  (The 127 workload also goes
    through the at-the-ceiling and seam tests above.)"""
    w_at, w_over, own = BASE_AT, BASE_OVER, BASE_LIM
    assert hip.geometry(w_at, own).variant >> 8 & 0x1f == 0 == hip.geometry(w_over, own).variant >> 8 & 0x1f      # base ops only
    largest = hip.grown_limits(w_over, None, 8)             # every capacity at its ceiling — this workload's mailboxes: 127, no build has more
    assert (largest.mbox_msgs, largest.mbox_regs, largest.max_tasks, own.mbox_msgs) == (127, 255, 254, 127)
    want_at, want_over = (parity.expected(w, SEED0, COUNT, None, own) for w in (w_at, w_over))
    assert (want_at["verdict"] == A.PASS).all() and (want_over["verdict"] == A.PASS).all()      # the oracle passes both
    for what, lim in (("default", A.Limits()), ("own", own), ("largest", largest)):
        auto, _ = hip.run_batch_auto(w_at, SEED0, COUNT, None, lim, max_rounds=8)
        assert (auto == want_at).all(), (what, auto[auto != want_at][0], want_at[auto != want_at][0])
    capacities = [("default", A.Limits())] + [(f"round {r}", hip.grown_limits(w_over, None, r)) for r in range(1, 8)] + [("own", own), ("largest", largest)]
    assert [lim.mbox_msgs for _, lim in capacities] == [0, 4, 8, 16, 32, 64, 127, 127, 127, 127]
    for what, lim in capacities:
        got, _ = hip.run_batch(w_over, SEED0, COUNT, None, lim)
        print("128 datagrams,", what, "verdicts", np.bincount(got["verdict"], minlength=8).tolist())
        assert (got["verdict"] == A.OVERFLOW).all(), (what, np.bincount(got["verdict"], minlength=8))
    for what, lim in (("default", A.Limits()), ("own", own), ("largest", largest)):
        auto, _ = hip.run_batch_auto(w_over, SEED0, COUNT, None, lim, max_rounds=8)
        assert (auto["verdict"] == A.OVERFLOW).all(), (what, np.bincount(auto["verdict"], minlength=8))
    # ... and through a resolving campaign of 8 rounds: every seed re-run in every round, none settled, the call does not fail
    rep = hip.run_campaign(w_over, SEED0, COUNT, 0, 0, False, None, A.Limits(), resolve=8)
    acct = hip.campaign_resolved()
    assert (rep.seeds_run, rep.n_runner, rep.n_failed) == (COUNT, COUNT, 0) and (acct.n_first_pass, acct.n_resolved, acct.n_unresolved) == (COUNT, 0, COUNT)
    rep = hip.run_campaign(w_at, SEED0, COUNT, 0, 0, False, None, A.Limits(), resolve=8)
    assert (rep.seeds_run, rep.n_runner, rep.n_failed) == (COUNT, 0, 0) and hip.campaign_resolved().n_resolved == COUNT


# ---- a batch in which about every second lane leaves the model, through the campaign forms ------------------------------------------------

MIX_TOTAL, ROUNDS = 1024, 8                                # (8 rounds: mbox_msgs climbs 2 -> 255 in seven)


@functools.lru_cache(maxsize=None)
def mix():
    w, cfg, lim = LW.model_mix_workload()
    want = parity.expected(w, 0, MIX_TOTAL, cfg, lim)
    want.setflags(write=False)
    n = np.bincount(want["verdict"], minlength=8)
    assert n[A.PASS] >= 256 and n[A.UNSUPPORTED] >= 256 and n[A.PASS] + n[A.UNSUPPORTED] == MIX_TOTAL
    return w, cfg, lim, want


def grown_by_parity(w, lim, rounds):
    for _ in range(rounds):
        lim = parity.grow(lim, w.struct.n_progs)
    return lim


@pytest.mark.parametrize("batch", [1024, 256])
@pytest.mark.parametrize("from_defaults", [False, True], ids=["own-limits", "defaults-resolve"])
def test_the_mix_through_plain_and_collecting_campaigns(hip, batch, from_defaults):
    """MADSIM_UNSUPPORTED is a runner verdict (include/madsim_hip.h): the plain report counts it in n_runner, has no genuine failure and no
    first failing seed; the collecting form counts it in n_by_verdict[6] and lists it only with MADSIM_CAMPAIGN_LIST_RUNNER — then exactly
    those seeds, ascending, with all-zero results."""
    w, cfg, own, want = mix()
    lim, resolve = (A.Limits(), ROUNDS) if from_defaults else (own, None)
    n_uns = int((want["verdict"] == A.UNSUPPORTED).sum())
    uns = np.nonzero(want["verdict"] == A.UNSUPPORTED)[0].astype(np.uint64)
    rep = hip.run_campaign(w, 0, MIX_TOTAL, batch, 0, False, cfg, lim, resolve=resolve)
    assert plain_report(rep) == plain_truth(want, 0, batch), (plain_report(rep), plain_truth(want, 0, batch))
    assert (rep.n_failed, rep.n_runner, rep.first_failing_seed) == (0, n_uns, NONE)
    if from_defaults:                                       # the account, from the per-seed ladder under parity.grow
        resolved, k, rungs = ladder(hip.run_batch, grown_by_parity, w, 0, MIX_TOTAL, cfg, lim, ROUNDS)
        assert (resolved == want).all(), (resolved[resolved != want][0], want[resolved != want][0])
        truth = account_truth(k, rungs, resolved, lim, ROUNDS, batch)
        print("account", account(hip.campaign_resolved()), truth)
        assert account(hip.campaign_resolved()) == truth
        assert (truth["n_first_pass"], truth["n_resolved"], truth["n_unresolved"]) == (MIX_TOTAL, MIX_TOTAL - n_uns, n_uns)
    for list_runner in (True, False):
        got = hip.run_campaign(w, 0, MIX_TOTAL, batch, 0, False, cfg, lim, collect=MIX_TOTAL, list_runner=list_runner, resolve=resolve)
        check_collect(got, want, 0, MIX_TOTAL, list_runner, plain=rep, what=(batch, from_defaults, list_runner))
        _, fails, hist = got
        assert (hist == np.bincount(want["verdict"], minlength=8)).all() and hist[A.UNSUPPORTED] == n_uns
        if list_runner:
            assert (fails["seed"] == uns).all() and fails["seed"][0] == uns[0] and (fails["verdict"] == A.UNSUPPORTED).all()
            assert not any(fails[f].any() for f in want.dtype.names[1:])
            assert fails.tobytes() == listed(want, 0, MIX_TOTAL, True).tobytes()
        else:
            assert len(fails) == 0
        if from_defaults:
            assert account(hip.campaign_resolved()) == truth


@pytest.mark.parametrize("batch", [1024, 256])
@pytest.mark.parametrize("from_defaults", [False, True], ids=["own-limits", "defaults-resolve"])
def test_the_mix_through_differential_and_sweep_campaigns(hip, batch, from_defaults):
    """The workload against itself at loss 0, where every seed queues all 256 datagrams: a seed that is MADSIM_UNSUPPORTED on either side is
    incomparable, and row and column 6 of the transition matrix are the two sides' counts; the sweep's runner counts per variant likewise."""
    w, cfg, own, a = mix()
    b = parity.expected(w, 0, MIX_TOTAL, None, own)
    assert (b["verdict"] == A.UNSUPPORTED).all()
    lim, resolve = (A.Limits(), ROUNDS) if from_defaults else (own, None)
    got = hip.run_campaign_diff_resolved(w, 0, MIX_TOTAL, resolve, config=cfg, other_config=A.Config.default(), limits=lim, other_limits=lim,
                                         max_listed=16, batch=batch)
    check_diff(got, a, b, 0, A.DIFF_ALL, 16, ("diff", batch, from_defaults))
    d = got[2]
    either = (a["verdict"] == A.UNSUPPORTED) | (b["verdict"] == A.UNSUPPORTED)
    assert d.n_incomparable == int(either.sum()) and d.n_compared == MIX_TOTAL - int(either.sum()) and d.n_differ == 0 and len(d) == 0
    t = d.transitions.astype(np.int64)
    assert t[A.UNSUPPORTED, :].sum() == np.bincount(a["verdict"], minlength=8)[A.UNSUPPORTED]
    assert t[:, A.UNSUPPORTED].sum() == np.bincount(b["verdict"], minlength=8)[A.UNSUPPORTED] == MIX_TOTAL
    # side B against side A: the matrix transposed, the same seeds incomparable
    back = hip.run_campaign_diff_resolved(w, 0, MIX_TOTAL, resolve, config=A.Config.default(), other_config=cfg, limits=lim, other_limits=lim,
                                          max_listed=16, batch=batch)
    check_diff(back, b, a, 0, A.DIFF_ALL, 16, ("diff, sides swapped", batch, from_defaults))
    assert (back[2].transitions == d.transitions.T).all()
    # the sweep: the two variants; then — so that settled seeds exist and records are listed — the lossy one twice beside a lossier third
    variants = [(w, cfg, lim), (w, A.Config.default(), lim)]
    got = hip.run_campaign_sweep(variants, 0, MIX_TOTAL, fields=A.DIFF_ALL, list_rule="differing", max_listed=MIX_TOTAL, batch=batch, resolve=resolve)
    check_sweep(got, [a, b], 0, A.DIFF_ALL, sweep_ref.DIFFERING, MIX_TOTAL, ("sweep", batch, from_defaults))
    reps, sw = got
    assert int(sw.n_runner_by_variant[0]) == int(reps[0].n_runner) == int((a["verdict"] == A.UNSUPPORTED).sum())
    assert int(sw.n_runner_by_variant[1]) == MIX_TOTAL == sw.n_incomparable and len(sw) == 0
    cfg3 = A.Config.default(packet_loss_rate=0.006)
    c = parity.expected(w, 0, MIX_TOTAL, cfg3, own)
    fail, runner, differ = sweep_ref.classify([a, a, c], A.DIFF_ALL)
    assert ((runner != 0) & (runner != 7)).any() and (differ != 0).any()      # seeds that leave the model under one rate only; settled seeds that differ
    got = hip.run_campaign_sweep([(w, cfg, lim), (w, cfg, lim), (w, cfg3, lim)], 0, MIX_TOTAL, fields=A.DIFF_ALL, list_rule="differing",
                                 max_listed=MIX_TOTAL, batch=batch, resolve=resolve)
    check_sweep(got, [a, a, c], 0, A.DIFF_ALL, sweep_ref.DIFFERING, MIX_TOTAL, ("sweep of three", batch, from_defaults))
    assert len(got[1]) == int((differ != 0).sum()) > 0


# ---- the top of the 4 GiB global-state region -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("narrow", [False, True], ids=["wide-heap", "narrow-heap"])
def test_the_top_of_the_global_state_region(hip, narrow):
    """The per-lane state blocks of a launch form one region addressed with 32-bit buffer offsets, `at * total_lanes + lane * k`
    (k_state.h gs_addr_*, k_timer.h pool_addr), and the host keeps it below 4 GiB (madsim_hip.cpp ensure_scratch).  The largest block the
    limits admit — 60 addresses, every capacity at its ceiling — puts that edge at about 17 290 lanes; the workload runs one exchange through
    the first two sockets and one through the last two, whose planes are the highest words of the block.  With MADSIM_STATE_NARROW_HEAP the
    geometry selects the 8-byte-entry build for this workload (asserted), and a datagram delivery then writes the record pool, which lies
    behind the planes at the very top.  A wrong offset reads zeros, drops a store (buffer resources clamp) or aliases another lane: a mismatch
    with the oracle in some lane, never a fault."""
    w, lim = LW.top_of_state_region()
    if narrow:
        lim.state_mem |= A.STATE_NARROW_HEAP
    geo = hip.geometry(w, lim)
    B = geo.global_bytes_per_seed
    assert geo.variant & 16 and geo.lanes_per_wave == 64 and bool(geo.variant >> 8 & 0x80) == narrow and (geo.variant >> 8 & 0xf) == 0xf, hex(geo.variant)      # global state, full waves, every op class
    assert 200_000 < B < 1 << 24                            # (__umul24 takes the block's offsets)
    with hip.Context(0) as ctx:                             # a context of its own: its 4 GiB of scratch goes when it closes
        def runs(k):
            try:
                return ctx.run_batch(w, SEED0, 256 * k, None, lim)[0], None
            except hip.MadsimHipError as e:
                if not str(e).startswith("limits do not fit the device"):      # only MADSIM_E_LIMITS is a refusal; a failed allocation is its own error
                    raise
                return None, str(e)
        lo, hi = 1, 2 * ((1 << 32) // (256 * B) + 1)        # lo runs (asserted), hi is refused (asserted); at most 8 probes between
        got, why = runs(lo)
        assert got is not None, why
        refused, why_hi = runs(hi)
        assert refused is None
        n_refused = 1
        while hi - lo > 1:
            mid = (lo + hi) // 2
            r, why = runs(mid)
            if r is None:
                hi, why_hi, n_refused = mid, why, n_refused + 1
            else:
                lo, got = mid, r
        assert n_refused <= 12
    accepted, refused = 256 * lo, 256 * hi
    print("B", B, "accepted", accepted, "lanes:", B * accepted, "refused", refused, "lanes:", B * refused, "2^32 =", 1 << 32)
    assert why_hi.startswith("limits do not fit the device") and "global state region exceeds 4 GiB" in why_hi, why_hi      # MADSIM_E_LIMITS
    assert B * accepted < 1 << 32 <= B * refused
    assert (1 << 32) - B * accepted <= B * 256               # within one workgroup's share of the edge
    want = parity.expected(w, SEED0, accepted, None, lim)
    assert (want["verdict"] == A.PASS).all() and len(got) == accepted
    bad = np.nonzero(got != want)[0]
    assert len(bad) == 0, (len(bad), "first lane", int(bad[0]), "last lane", int(bad[-1]), got[bad[0]], want[bad[0]])
