"""Divergence reports on the MI355X: madsim_hip_diverge_seeds / madsim_hip_ctx_diverge_seeds and runtime.diverge_seeds against the CPU oracle's
logs and observation lists put through tests/diverge_ref.py — every record byte and every context word, exactly; the results by
tests/parity.py's expected() convention.  The blocks, and the proof from the oracle alone that they hold the statuses they are there for,
are tests/test_diverge.py's (which runs without a GPU)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import oracle
from madsim_amd import _abi as A
from tests import diverge_ref as R
from tests import groups_ref as G
from tests import test_diverge as D
from tests import test_observe as T

pytestmark = pytest.mark.gpu

ROUNDS = A.RESOLVE_MAX_ROUNDS


def raw(hip, wa, ca, la, wb, cb, lb, seeds, log_cap, obs_cap, win, ctx=None):
    """The C entry itself (the default context's, or `ctx`'s): (records ndarray[A.DIVERGENCE_DTYPE], context rows uint64[n, 3 * win]), from
    host buffers that hold a pattern before the call."""
    n = len(seeds)
    s = np.array(seeds, dtype=np.uint64)
    recs = np.full(n * 184, 0xAA, dtype=np.uint8)
    rows = np.full((n, 3 * win), 0xAAAAAAAAAAAAAAAA, dtype=np.uint64)
    args = [wa.ref(), C.byref(ca), C.byref(la), wb.ref(), C.byref(cb), C.byref(lb), s.ctypes.data_as(C.POINTER(C.c_uint64)), n, log_cap, obs_cap, win,
            recs.ctypes.data_as(C.c_void_p), rows.ctypes.data_as(C.c_void_p) if win else None]
    L = hip.lib()
    rc = L.madsim_hip_ctx_diverge_seeds(ctx._h, *args) if ctx is not None else L.madsim_hip_diverge_seeds(*args)
    assert rc == 0, (rc, L.madsim_hip_last_error().decode())
    return recs.view(A.DIVERGENCE_DTYPE).copy(), rows


def same_bytes(got, want, what):
    recs, rows = got
    wrecs, wrows = want
    if recs.tobytes() != wrecs.tobytes():
        bad = [i for i in range(len(recs)) if recs[i].tobytes() != wrecs[i].tobytes()]
        raise AssertionError((what, "records", bad[:8], recs[bad[0]], wrecs[bad[0]]))
    assert rows.tobytes() == wrows.tobytes(), (what, "context rows", np.nonzero((rows != wrows).any(axis=1))[0][:8].tolist())


def pick(truth, idx):
    recs, rows = truth
    return recs[idx], rows[idx]


# ---- 1. the blocks, on both state layouts ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mem", [A.STATE_LDS, A.STATE_GLOBAL])
@pytest.mark.parametrize("name", ["loss", "bodies", "small_caps", "steps"])
def test_blocks_equal_the_oracle(hip, name, mem):
    wa, ca, la, wb, cb, lb, seed0, n, log_cap, obs_cap = D.blocks()[name]
    la, lb = D.limits_like(la, state_mem=mem), D.limits_like(lb, state_mem=mem)
    got = raw(hip, wa, ca, la, wb, cb, lb, range(seed0, seed0 + n), log_cap, obs_cap, D.WINDOW)
    print(name, mem, np.bincount(got[0]["log_status"], minlength=5), np.bincount(got[0]["obs_status"], minlength=5))
    same_bytes(got, D.block_truth(name), (name, mem))


def test_the_wrapper_reports_what_the_records_hold(hip):
    """runtime.diverge_seeds: the record fields as Python ints, the context row cut into shared / next_a / next_b at the true counts."""
    wa, ca, la, wb, cb, lb, seed0, n, log_cap, obs_cap = D.blocks()["bodies"]
    recs, rows = D.block_truth("bodies")
    seeds = list(range(seed0, seed0 + 65))
    out = hip.diverge_seeds(wa, seeds, other=wb, config=ca, other_config=cb, limits=la, other_limits=lb, log_cap=log_cap, obs_cap=obs_cap,
                            window=D.WINDOW, resolve=None)
    assert [d.seed for d in out] == seeds
    w = D.WINDOW
    for i, d in enumerate(out):
        x = recs[i]
        for f in ("log_status", "obs_status", "log_at", "obs_at", "log_len_a", "log_len_b", "obs_len_a", "obs_len_b", "obs_a", "obs_b", "log_a", "log_b"):
            assert getattr(d, f) == int(x[f]), (i, f)
        assert d.a.astuple() == tuple(int(v) for v in x["a"]) and d.b.astuple() == tuple(int(v) for v in x["b"])
        vals_a, vals_b = oracle.observe_seed(wa, seeds[i], ca, la)[0], oracle.observe_seed(wb, seeds[i], cb, lb)[0]
        at = d.obs_at
        assert d.shared == vals_a[max(at - w, 0):at] == vals_b[max(at - w, 0):at], (i, d)
        assert d.next_a == vals_a[at:at + w][:max(obs_cap - at, 0)] and d.next_b == vals_b[at:at + w][:max(obs_cap - at, 0)], (i, d)
        assert d.shared == [int(v) for v in rows[i, w - len(d.shared):w]]
    # None on the B side means A's: a run against itself
    me = hip.diverge_seeds(wa, seeds[:3], config=ca, log_cap=4096, obs_cap=4, window=2, resolve=None)
    assert all(d.log_status == d.obs_status == A.DIVERGE_SAME and d.a.astuple() == d.b.astuple() for d in me)


# ---- 2. runs that must not part ----------------------------------------------------------------------------------------------------------
def test_one_workload_under_two_layouts_or_limits_is_the_same_run(hip):
    """The state layout and the capacities are the runner's business: every seed SAME on both channels, the two results equal."""
    w, cfg, _ = G.traced_pingpong()
    cfg = A.Config.default(packet_loss_rate=D.LOSS)
    seeds = range(G.SEED0, G.SEED0 + 257)
    pairs = [(D.limits_like(state_mem=A.STATE_LDS), D.limits_like(state_mem=A.STATE_GLOBAL)),
             (A.Limits(), D.limits_like(heap_spill_slots=128, mbox_regs=8, mbox_msgs=4, lanes_per_wave=32))]
    for la, lb in pairs:
        recs, rows = raw(hip, w, cfg, la, w, cfg, lb, seeds, 1024, 8, 4)
        assert (recs["log_status"] == A.DIVERGE_SAME).all() and (recs["obs_status"] == A.DIVERGE_SAME).all()
        assert recs["a"].tobytes() == recs["b"].tobytes() and (recs["log_at"] == recs["log_len_a"]).all() and (recs["log_len_a"] == recs["log_len_b"]).all()
        assert not recs["obs_a"].any() and not recs["log_a"].any() and not rows[:, 4:].any()
        assert set(recs["a"]["verdict"].tolist()) == {A.PASS, A.DEADLOCK}


def test_the_same_arguments_on_both_sides(hip):
    """The reference's determinism check, many seeds at once: the same run twice is the same run."""
    for name in ("lossy_pingpong", "raft_ticker", "lossy_select"):
        w, cfg, lim = T.directed()[name]
        recs, rows = raw(hip, w, cfg, lim, w, cfg, lim, range(100), 4096, 1024, 8)
        assert (recs["log_status"] == A.DIVERGE_SAME).all() and (recs["obs_status"] == A.DIVERGE_SAME).all(), name
        assert recs["a"].tobytes() == recs["b"].tobytes() and (recs["log_at"] == recs["log_len_a"]).all() and (recs["obs_at"] == recs["obs_len_a"]).all()
        assert (recs["a"]["verdict"] < A.OVERFLOW).all() and recs["log_len_a"].min() > 0


# ---- 3. lists ----------------------------------------------------------------------------------------------------------------------------
def test_lists_in_any_order_with_duplicates_and_of_several_lengths(hip):
    wa, ca, la, wb, cb, lb, seed0, n, log_cap, obs_cap = D.blocks()["loss"]
    truth = D.block_truth("loss")
    idx = list(range(199, -1, -1)) + [7, 7, 199]                                    # descending, then duplicates
    got = raw(hip, wa, ca, la, wb, cb, lb, [seed0 + i for i in idx], log_cap, obs_cap, D.WINDOW)
    same_bytes(got, pick(truth, idx), "descending with duplicates")
    for m in (1, 63, 65, 257):
        idx = [(i * 37 + 5) % n for i in range(m)]
        got = raw(hip, wa, ca, la, wb, cb, lb, [seed0 + i for i in idx], log_cap, obs_cap, D.WINDOW)
        same_bytes(got, pick(truth, idx), ("n", m))
    # no window: the records alone
    got = raw(hip, wa, ca, la, wb, cb, lb, range(seed0, seed0 + 65), log_cap, obs_cap, 0)
    assert got[0].tobytes() == truth[0][:65].tobytes() and got[1].shape == (65, 0)


def test_a_second_context_gives_the_same_bytes(hip):
    wa, ca, la, wb, cb, lb, seed0, n, log_cap, obs_cap = D.blocks()["bodies"]
    seeds = range(seed0, seed0 + 130)
    want = raw(hip, wa, ca, la, wb, cb, lb, seeds, log_cap, obs_cap, D.WINDOW)
    with hip.Context(0) as ctx:
        got = raw(hip, wa, ca, la, wb, cb, lb, seeds, log_cap, obs_cap, D.WINDOW, ctx)
        again = raw(hip, wa, ca, la, wb, cb, lb, seeds, log_cap, obs_cap, D.WINDOW, ctx)      # ... and its buffers, used a second time
        out = ctx.diverge_seeds(wa, list(seeds)[:5], other=wb, config=ca, other_config=cb, limits=la, other_limits=lb, log_cap=log_cap, obs_cap=obs_cap,
                                window=D.WINDOW, resolve=None)
    same_bytes(got, want, "second context")
    same_bytes(again, want, "second call")
    same_bytes(want, pick(D.block_truth("bodies"), slice(0, 130)), "the oracle")
    assert [d.log_at for d in out] == want[0]["log_at"][:5].tolist()


# ---- 4. resolve --------------------------------------------------------------------------------------------------------------------------
def test_resolve_replays_the_incomparable_seeds_under_grown_limits(hip):
    wa, ca, la, wb, cb, lb, seed0, n, log_cap, obs_cap = D.blocks()["steps"]
    seeds = list(range(seed0, seed0 + 100))
    capped, _ = D.block_truth("steps")
    grown, grows = D.block_truth("steps", True)
    kw = dict(other=wb, config=ca, other_config=cb, limits=la, other_limits=lb, log_cap=log_cap, obs_cap=obs_cap, window=D.WINDOW)
    left = hip.diverge_seeds(wa, seeds, resolve=None, **kw)
    assert [d.log_status for d in left] == capped["log_status"][:100].tolist() and sum(d.log_status == A.DIVERGE_INCOMPARABLE for d in left) >= 3
    assert all(d.b.verdict == A.STEP_LIMIT and not d.shared and not d.next_a and not d.next_b for d in left if d.log_status == A.DIVERGE_INCOMPARABLE)
    done = hip.diverge_seeds(wa, seeds, resolve=True, **kw)
    for i, d in enumerate(done):
        x = grown[i]
        assert (d.log_status, d.obs_status, d.log_at, d.obs_at, d.log_a, d.log_b, d.obs_a, d.obs_b) == \
               tuple(int(x[f]) for f in ("log_status", "obs_status", "log_at", "obs_at", "log_a", "log_b", "obs_a", "obs_b")), (i, d)
        assert d.a.astuple() == tuple(int(v) for v in x["a"]) and d.b.astuple() == tuple(int(v) for v in x["b"]), (i, d)
        assert d.log_status != A.DIVERGE_INCOMPARABLE and d.shared == [int(v) for v in grows[i, D.WINDOW - len(d.shared):D.WINDOW]]


# ---- 5. trace_seeds is what it was -------------------------------------------------------------------------------------------------------
def test_trace_seeds_still_returns_its_bytes_and_its_rows_give_the_records(hip):
    """A diverge call in between leaves trace_seeds' answers alone (they share side A's buffers), and the divergence records are what
    tests/diverge_ref.py makes of the rows the two trace_seeds calls copy back — the route this call replaces."""
    wa, ca, la, wb, cb, lb, seed0, n, log_cap, obs_cap = D.blocks()["bodies"]
    seeds = [seed0 + i for i in (5, 0, 99, 5, 64)]
    before = hip.trace_seeds(wa, seeds, ca, la, obs_cap=obs_cap, log_cap=log_cap, resolve=None)
    got = raw(hip, wa, ca, la, wb, cb, lb, seeds, log_cap, obs_cap, D.WINDOW)
    after = hip.trace_seeds(wa, seeds, ca, la, obs_cap=obs_cap, log_cap=log_cap, resolve=None)
    other = hip.trace_seeds(wb, seeds, cb, lb, obs_cap=obs_cap, log_cap=log_cap, resolve=None)
    for x, y, s in zip(before, after, seeds):
        log, res = oracle.trace_seed(wa, s, ca, la)
        assert (x.result.astuple(), x.observations, x.n_observations, x.log, x.log_len) == (y.result.astuple(), y.observations, y.n_observations, y.log, y.log_len)
        assert (x.log, x.log_len, x.result.astuple()) == (log[:log_cap], len(log), res.astuple()), s
    def side(traces):
        logs, _ = R.rows_of([t.log for t in traces], log_cap, np.uint8)
        obs, _ = R.rows_of([t.observations for t in traces], obs_cap, np.uint64)
        res = np.array([t.result.astuple() for t in traces], dtype=A.RESULT_DTYPE)
        return logs, np.array([t.log_len for t in traces], dtype=np.uint64), obs, np.array([t.n_observations for t in traces], dtype=np.uint64), res
    a, b = side(after), side(other)
    want = R.records(seeds, a[0], b[0], a[1], b[1], a[2], b[2], a[3], b[3], a[4], b[4], D.WINDOW)
    same_bytes(got, want, "from trace_seeds' rows")
    # trace_seed (n = 1) too
    log, res = hip.trace_seed(wa, seeds[0], ca, la)
    assert (log, res.astuple()) == (oracle.trace_seed(wa, seeds[0], ca, la)[0], before[0].result.astuple())


# ---- 6. the example ----------------------------------------------------------------------------------------------------------------------
def test_diverge_example(hip):
    """examples/diverge_test.cpp (C++ Builder mirror) prints, per seed the fix changed, what runtime.diverge_seeds reports for it."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "examples", "diverge_test")
    assert os.path.exists(exe), "examples/diverge_test is not built (run __graft_entry__.build())"
    w, cfg, _ = G.traced_pingpong()
    fixed, fixed_lim = T.fixed_pingpong()
    total = T.CAMPAIGN_TOTAL
    hip.shutdown()
    try:
        p = subprocess.run([exe], env=dict(os.environ, MADSIM_TEST_SEED=str(G.SEED0), MADSIM_TEST_NUM=str(total)), capture_output=True, text=True, timeout=120)
    finally:
        hip.init(0)
    assert p.returncode == 0, (p.returncode, p.stdout, p.stderr)
    lim = D.limits_like(heap_spill_slots=128, mbox_regs=8, mbox_msgs=4)             # the example's capacities, both sides
    ra, rb, d = hip.run_campaign_diff_resolved(w, G.SEED0, total, None, other=fixed, config=cfg, limits=lim, other_limits=lim, fields=A.DIFF_VERDICT,
                                               max_listed=8, batch=1024, in_flight=2)
    seeds = [int(x["seed"]) for x in d.records]
    assert len(seeds) == 8 and f"{total} seeds from {G.SEED0}, the fix changes {d.n_differ}, 8 listed" in p.stdout, p.stdout
    parts = hip.diverge_seeds(w, seeds, other=fixed, config=cfg, limits=lim, log_cap=4096, obs_cap=8, window=4, resolve=None)
    for x in parts:
        line = (f"  seed {x.seed}: log {A.DIVERGE_NAMES[x.log_status]} at draw {x.log_at} of {x.log_len_a} / {x.log_len_b} (byte {x.log_a} / {x.log_b}); "
                f"observations {A.DIVERGE_NAMES[x.obs_status]} at {x.obs_at}: shared {x.shared}, then old {x.next_a}, new {x.next_b}")
        assert line in p.stdout, (line, p.stdout)
        assert x.log_status in (A.DIVERGE_DIFFER, A.DIVERGE_PREFIX) and x.a.verdict == A.DEADLOCK and x.b.verdict == A.PASS
