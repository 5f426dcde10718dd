"""Observation logs on the MI355X: madsim_hip_trace_seeds / madsim_hip_observe_seed through runtime.trace_seeds, observe_seed and the
`observe=` option of the campaigns, against the CPU oracle's observe_seed / trace_seed — values, counts, log bytes and all 48 result bytes,
every comparison exact.  The workloads, the fuzz blocks and the proof that every seed of theirs is inside the workload model are
tests/test_observe.py's (which runs without a GPU); no seed is left out here: a first-pass runner verdict is replayed by trace_seeds' own
ladder (resolve=) and then compared, and one that is still a runner verdict differs from the oracle and fails."""
import functools
import os
import subprocess

import numpy as np
import pytest

import oracle
from madsim_amd import _abi as A
from tests import groups_ref as G
from tests import test_observe as T

pytestmark = pytest.mark.gpu

U64_MAX = (1 << 64) - 1
ROUNDS = A.RESOLVE_MAX_ROUNDS


@functools.lru_cache(maxsize=None)
def truth(name, seed):
    """(observations, Result, log bytes) of one seed of a directed workload, by the oracle; computed once."""
    w, cfg, lim = DIRECTED[name]
    vals, res = oracle.observe_seed(w, seed, cfg, lim)
    log, res2 = oracle.trace_seed(w, seed, cfg, lim)
    assert res.astuple() == res2.astuple() and res.verdict < A.OVERFLOW
    return vals, res, log


DIRECTED = T.directed()


def same(trace, want, obs_cap, log_cap, what):
    vals, res, log = want
    assert trace.result.astuple() == res.astuple(), (what, trace.result.astuple(), res.astuple())
    assert trace.n_observations == len(vals) and trace.observations == vals[:obs_cap], (what, trace.n_observations, trace.observations, vals)
    assert trace.log_len == len(log) and trace.log == log[:log_cap], (what, trace.log_len, len(log))


# ---- 1. a single seed --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(DIRECTED))
def test_single_seed_equals_the_oracle(hip, name):
    w, cfg, lim = DIRECTED[name]
    for seed in T.DIRECTED_SEEDS:
        vals, res, _ = truth(name, seed)
        got, gres = hip.observe_seed(w, seed, cfg, lim, resolve=ROUNDS)
        assert got == vals and len(got) == len(vals), (name, seed, got, vals)
        assert gres.astuple() == res.astuple() and bytes(gres) == bytes(res), (name, seed)
        assert hip.fold_observations(got) == gres.obs_hash, (name, seed)


# ---- 2. a list in one launch -------------------------------------------------------------------------------------------------------------
POOL = [(i * 2654435761 + 12345) % 100_003 for i in range(300)]            # distinct, unsorted


def seed_list(n):
    """n seeds: unsorted, 2^64 - 1 among them, and (from three on) one duplicate pair, first and last."""
    if n == 1:
        return [U64_MAX]
    seeds = POOL[:n]
    seeds[n // 2] = U64_MAX
    if n >= 3:
        seeds[n - 1] = seeds[0]
    return seeds


@pytest.mark.parametrize("lanes", [0, 8, 16, 32, 64])
def test_a_list_in_one_launch(hip, lanes):
    assert len(set(POOL)) == len(POOL) and POOL != sorted(POOL)
    w, cfg, _ = DIRECTED["lossy_pingpong"]
    lim = A.Limits(); lim.lanes_per_wave = lanes
    for n in (1, 63, 64, 65, 257):
        seeds = seed_list(n)
        traces = hip.trace_seeds(w, seeds, cfg, lim, obs_cap=8, log_cap=1024, resolve=ROUNDS)
        assert [t.seed for t in traces] == seeds
        verdicts = set()
        for i, t in enumerate(traces):
            same(t, truth("lossy_pingpong", seeds[i]), 8, 1024, (lanes, n, i, seeds[i]))
            verdicts.add(t.result.verdict)
        if n >= 63:
            assert verdicts == {A.PASS, A.DEADLOCK}, verdicts
            a, b = traces[0], traces[n - 1]
            assert seeds[0] == seeds[n - 1] and (a.result.astuple(), a.observations, a.log) == (b.result.astuple(), b.observations, b.log)
    # n = 1 is trace_seed: the same bytes
    for seed in (U64_MAX, 3):
        log, res = hip.trace_seed(w, seed, cfg, lim)
        t = hip.trace_seeds(w, [seed], cfg, lim, obs_cap=0, log_cap=1 << 20, resolve=None)[0]
        assert (t.log, t.log_len, t.result.astuple()) == (log, len(log), res.astuple()) and log == truth("lossy_pingpong", seed)[2]


# ---- 3. caps -----------------------------------------------------------------------------------------------------------------------------
def test_caps(hip):
    """A store past a cap lands in the next row: the middle seed's caps are walked around its lengths through the C entry itself, into
    host buffers that hold a pattern before the call.  Every row of both arrays is the oracle's first min(len, cap) entries and zeros
    behind them, the lengths the true ones every time; the mirror, which trims a row to its entries, is held to the same prefixes."""
    import ctypes as C
    w, cfg, lim = DIRECTED[T.CAPS_WORKLOAD]
    seeds = list(T.CAPS_SEEDS)
    want = [truth(T.CAPS_WORKLOAD, s) for s in seeds]
    m, l = len(want[1][0]), len(want[1][2])
    s3 = (C.c_uint64 * 3)(*seeds)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p) if a.size else None                      # noqa: E731
    for obs_cap, log_cap in [(c, l) for c in (0, 1, m - 1, m, m + 1)] + [(m, c) for c in (0, 1, l - 1, l, l + 1)]:
        obs, logs = np.full((3, obs_cap), 0xAAAAAAAAAAAAAAAA, dtype=np.uint64), np.full((3, log_cap), 0xAA, dtype=np.uint8)
        olen, llen = np.full(3, 0xAAAAAAAAAAAAAAAA, dtype=np.uint64), np.full(3, 0xAAAAAAAAAAAAAAAA, dtype=np.uint64)
        res = np.zeros(3, dtype=A.RESULT_DTYPE)
        rc = hip.lib().madsim_hip_trace_seeds(w.ref(), C.byref(cfg), s3, 3, C.byref(lim), ptr(logs), log_cap, ptr(obs), obs_cap, ptr(llen), ptr(olen),
                                              ptr(res))
        assert rc == 0, (obs_cap, log_cap)
        for i, (vals, r, log) in enumerate(want):
            what = (obs_cap, log_cap, seeds[i])
            assert (int(olen[i]), int(llen[i])) == (len(vals), len(log)), what
            assert obs[i].tolist() == (vals + [0] * obs_cap)[:obs_cap], (what, obs[i].tolist(), vals)
            assert logs[i].tobytes() == (log + bytes(log_cap))[:log_cap], (what, "log row")
            assert tuple(int(x) for x in res[i]) == r.astuple(), what
        assert (int(olen[1]), int(llen[1])) == (m, l)
        traces = hip.trace_seeds(w, seeds, cfg, lim, obs_cap=obs_cap, log_cap=log_cap, resolve=None)
        for t, wt in zip(traces, want):
            same(t, wt, obs_cap, log_cap, (obs_cap, log_cap, t.seed))


# ---- 4. fuzz parity ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(T.BLOCKS))
def test_fuzz_parity(hip, name):
    """One trace_seeds call per program of the block (its ladder replays what the first pass leaves with a runner verdict); every row is
    the oracle's list and result.  The blocks are fixed: a failure names the generator call that rebuilds the program, and the seed."""
    n = 0
    for k, w, cfg, lim, desc, seeds, want in T.block_truth(name):
        what = f"block {name!r} program {k}: {desc}, limits time_limit_ns={lim.time_limit_ns} state_mem={lim.state_mem}"
        traces = hip.trace_seeds(w, seeds, cfg, lim, obs_cap=64, log_cap=0, resolve=ROUNDS)
        for t, (vals, res) in zip(traces, want):
            assert len(vals) <= 64
            assert t.result.astuple() == res.astuple(), (what, t.seed, t.result.astuple(), res.astuple())
            assert (t.n_observations, t.observations) == (len(vals), vals), (what, t.seed, t.observations, vals)
            n += 1
    assert n == T.N_PROGRAMS * T.N_SEEDS


# ---- 5. the campaigns --------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def campaign_truth(seed):
    w, cfg, _ = G.traced_pingpong()
    return oracle.observe_seed(w, seed, cfg)


def test_groups_spell_out_their_keys(hip):
    w, cfg, want = G.traced_pingpong()
    rep, groups = hip.run_campaign_groups(w, G.SEED0, T.CAMPAIGN_TOTAL, 1024, 2, config=cfg, observe=8)
    assert G.of_report(groups) == G.groups_truth(want[:T.CAMPAIGN_TOTAL], G.SEED0, G.FAILURES, 0, 32) and len(groups) >= 3
    assert len(groups.observations) == len(groups)
    for (verdict, key, count, first_seed), vals, n in zip(groups, groups.observations, groups.n_observations):
        assert hip.fold_observations(vals) == key and n == len(vals), (first_seed, vals, hex(key))
        assert vals == campaign_truth(first_seed)[0], (first_seed, vals)
    assert len({tuple(v) for v in groups.observations}) == len(groups)              # two different groups never hold the same list
    # the collecting form: the same lists for the listed seeds, the other returns as they were
    rep, fails, hist, lists = hip.run_campaign(w, G.SEED0, T.CAMPAIGN_TOTAL, 1024, 2, config=cfg, collect=8, observe=8)
    plain = hip.run_campaign(w, G.SEED0, T.CAMPAIGN_TOTAL, 1024, 2, config=cfg, collect=8)
    assert len(fails) == 8 == len(lists) and fails.tobytes() == plain[1].tobytes() and (hist == plain[2]).all()
    for f, vals in zip(fails, lists):
        vals_want, res = campaign_truth(int(f["seed"]))
        assert vals == vals_want and tuple(int(x) for x in f)[1:] == res.astuple(), int(f["seed"])
    by_seed = {int(g["first_seed"]): v for g, v in zip(groups.groups, groups.observations)}
    for f, vals in zip(fails, lists):
        if int(f["seed"]) in by_seed:
            assert by_seed[int(f["seed"])] == vals
    # observe=0, the default, is the call it was
    assert hip.run_campaign_groups(w, G.SEED0, T.CAMPAIGN_TOTAL, 1024, 2, config=cfg)[1].observations is None


def test_diff_lists_both_sides(hip):
    """The lossy ping-pong against its timeout-and-resend fix: the seeds the fix changed, with what each side traced."""
    w, cfg, _ = G.traced_pingpong()
    fixed, fixed_lim = T.fixed_pingpong()
    ra, rb, d = hip.run_campaign_diff_resolved(w, G.SEED0, T.CAMPAIGN_TOTAL, None, other=fixed, config=cfg, limits=A.Limits(), other_limits=fixed_lim,
                                               fields=A.DIFF_VERDICT, max_listed=4, observe=8, batch=1024, in_flight=2)
    assert len(d) == 4 == len(d.observations_a) == len(d.observations_b)
    for rec, la, lb in zip(d.records, d.observations_a, d.observations_b):
        seed = int(rec["seed"])
        va, res_a = campaign_truth(seed)
        vb, res_b = oracle.observe_seed(fixed, seed, cfg, fixed_lim)
        assert (la, tuple(int(x) for x in rec["a"])) == (va, res_a.astuple()), seed
        assert (lb, tuple(int(x) for x in rec["b"])) == (vb, res_b.astuple()), seed
        assert res_a.verdict == A.DEADLOCK and res_b.verdict == A.PASS and sorted(lb) == [0, 1] and len(la) < 2, (seed, la, lb)


def test_resolving_campaign_lists_under_the_grown_limits(hip):
    """Limits nobody fits: the first pass answers every seed with MADSIM_OVERFLOW, one round settles all.  The lists come from the replay
    under the grown limits, the check of the replayed 48 bytes against the listed ones passes, and the lists are the oracle's pure-run
    lists."""
    w, cfg, want = G.traced_pingpong()
    lim = A.Limits(); lim.heap_lds_slots, lim.heap_spill_slots = 2, 0
    first, _ = hip.run_batch(w, G.SEED0, 64, cfg, lim)
    assert (first["verdict"] == A.OVERFLOW).all()
    rep, fails, hist, lists = hip.run_campaign(w, G.SEED0, T.CAMPAIGN_TOTAL, 1024, 2, config=cfg, limits=lim, collect=8, resolve=True, observe=8)
    assert hip.campaign_resolved().n_first_pass == T.CAMPAIGN_TOTAL and rep.n_runner == 0 and len(fails) == 8
    for f, vals in zip(fails, lists):
        vals_want, res = campaign_truth(int(f["seed"]))
        assert vals == vals_want and tuple(int(x) for x in f)[1:] == res.astuple(), int(f["seed"])
    rep, groups = hip.run_campaign_groups(w, G.SEED0, T.CAMPAIGN_TOTAL, 1024, 2, config=cfg, limits=lim, resolve=True, observe=8)
    assert G.of_report(groups) == G.groups_truth(want[:T.CAMPAIGN_TOTAL], G.SEED0, G.FAILURES, 0, 32)
    assert [hip.fold_observations(v) for v in groups.observations] == [key for _, key, _, _ in groups]
    assert hip.trace_seeds(w, [G.SEED0], cfg, lim, resolve=True)[0].result.astuple() == campaign_truth(G.SEED0)[1].astuple()


# ---- 6. contexts -------------------------------------------------------------------------------------------------------------------------
def test_a_second_context_gives_the_same_bytes(hip):
    w, cfg, lim = DIRECTED["raft_ticker"]
    seeds = [5, 0, U64_MAX, 5, 77]
    want = hip.trace_seeds(w, seeds, cfg, lim, obs_cap=64, log_cap=4096)
    with hip.Context(0) as ctx:
        got = ctx.trace_seeds(w, seeds, cfg, lim, obs_cap=64, log_cap=4096)
        vals, res = ctx.observe_seed(w, 0, cfg, lim)
    for a, b in zip(got, want):
        assert (a.seed, a.result.astuple(), a.observations, a.n_observations, a.log, a.log_len) == \
               (b.seed, b.result.astuple(), b.observations, b.n_observations, b.log, b.log_len)
    assert (vals, res.astuple()) == (truth("raft_ticker", 0)[0], truth("raft_ticker", 0)[1].astuple())
    assert want[1].log == truth("raft_ticker", 0)[2][:4096]


# ---- 7. the example ----------------------------------------------------------------------------------------------------------------------
def test_explain_example(hip):
    """examples/explain_test.cpp (C++ Builder mirror): every way the lossy ping-pong deadlocks, with the seed to replay and the values it traced."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "examples", "explain_test")
    assert os.path.exists(exe), "examples/explain_test is not built (run __graft_entry__.build())"
    w, cfg, want = G.traced_pingpong()
    modes = G.groups_truth(want[:T.CAMPAIGN_TOTAL], G.SEED0, G.FAILURES, 0, 8)["groups"]
    hip.shutdown()
    try:
        p = subprocess.run([exe], env=dict(os.environ, MADSIM_TEST_SEED=str(G.SEED0), MADSIM_TEST_NUM=str(T.CAMPAIGN_TOTAL)), capture_output=True, text=True,
                           timeout=120)
    finally:
        hip.init(0)
    assert p.returncode == 0, (p.returncode, p.stdout, p.stderr)
    assert f"{T.CAMPAIGN_TOTAL} seeds from {G.SEED0}" in p.stdout and f"in {len(modes)} different ways" in p.stdout, p.stdout
    for verdict, key, count, first_seed in modes:
        vals = campaign_truth(first_seed)[0]
        line = f"deadlock, {count} seeds, replay with MADSIM_TEST_SEED={first_seed}: traced [{', '.join(str(v) for v in vals)}]"
        assert line in p.stdout, (line, p.stdout)
    assert "both pairs stuck" in p.stdout or "pair 0 stuck" in p.stdout or "pair 1 stuck" in p.stdout
