"""Task post-mortems and the stall-site census through the public calls on the device.  The truth is never the code under test:
  - the traced lossy ping-pong, first 4 096 seeds of tests/groups_ref.py's range: every seed's table from the oracle's result and what the
    oracle observed of an instrumented twin (tests/test_stall.py pingpong_truth), loop registers included; the census over the range, a
    sparse list, every chunk size and a second context against the numpy fold of those tables, byte for byte;
  - directed workloads whose table is written by hand from the program text (tests/stall_workloads.py), 65 seeds each so that a second
    wave takes part: a leaked task, a panic, an abort, a failing assert behind an await, one task parked in every awaiting op of each of
    the five trace builds under a time limit, and crowds of 63 / 64 / 65 parked children around a task_cap of 64;
  - the conventions of madsim_hip_task_states against madsim_hip_trace_seeds;
  - a block of every fuzz generator, checking what follows from the program table and the oracle's 48 bytes alone;
  - the paths the feature must leave alone, against the oracle-derived truths their own tests use, run BEHIND a task-log launch on the
    same context."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from madsim_amd import _abi as A
from madsim_amd import runtime
from tests import stall_ref as R
from tests import stall_workloads as SW
from tests import test_census as TC
from tests import test_observe as TO
from tests import test_probe_order as TPO
from tests import test_probe_sets as TPS
from tests import test_stall as T

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAILING = (A.PANIC, A.DEADLOCK, A.TIME_LIMIT)


def same(got, want, tag):
    assert got.n_counted == want.n_counted and got.n_idle == want.n_idle, (tag, got.n_counted, want.n_counted, got.n_idle, want.n_idle)
    assert (got.n_truncated, got.n_tasks, got.n_runner) == (want.n_truncated, want.n_tasks, want.n_runner), tag
    assert [int(s) for s in got.runner_seeds] == list(want.runner_seeds), tag
    assert got.sites.tobytes() == want.sites.tobytes(), (tag, got.sites, want.sites)
    assert got.shapes.tobytes() == want.shapes.tobytes(), (tag, got.shapes, want.shapes)
    assert got.tobytes() == want.tobytes(), tag
    assert int(got.sites["n_total"].sum()) == got.n_tasks, tag


# ---- 1. the lossy ping-pong: every seed's table, then the census --------------------------------------------------------------------------------
def test_pingpong_every_seed_ends_with_the_table_the_oracle_implies(hip):
    w, cfg, seeds, tables, verdicts, results, _ = T.pingpong_truth()
    got = hip.post_mortem(w, seeds, task_cap=32, config=cfg, lengths=True)
    assert len(got) == len(seeds)
    n_dead = 0
    for s, (res, recs, true_len), rows, want in zip(seeds, got, tables, results):
        assert res.astuple() == want.astuple(), (s, res.astuple(), want.astuple())
        exact = [R.word(st, prog, pc, c0, 0) for st, prog, pc, c0 in rows]
        assert true_len == len(rows) and [int(x) for x in recs] == exact, (s, [runtime.task_fields(x) for x in recs], rows)
        assert sorted(R.site(x) for x in recs) == sorted(R.site(x) for x in exact)      # (as sorted multisets of sites, as the issue words it)
        n_dead += res.verdict == A.DEADLOCK
    assert n_dead == verdicts.count(A.DEADLOCK) > 400


@pytest.mark.parametrize("chunk", [1000, 0, 1])
def test_pingpong_census_whatever_the_chunk(hip, chunk):
    w, cfg, seeds, _, _, _, _ = T.pingpong_truth()
    same(hip.stall_census(w, seeds[0], len(seeds), config=cfg, chunk=chunk), T.pingpong_ref(), chunk)      # (chunk 1: 4 096 launches of one seed)


def test_pingpong_census_forms_contexts_masks_and_what_it_says(hip):
    w, cfg, seeds, tables, verdicts, _, _ = T.pingpong_truth()
    want = T.pingpong_ref()
    whole = hip.stall_census(w, seeds[0], len(seeds), config=cfg)
    same(whole, want, "range")
    pick = sorted(set(range(0, len(seeds), 7)) | {1, 2, 3, len(seeds) - 1})
    for chunk in (0, 33):
        same(hip.stall_census(w, seeds=[seeds[i] for i in pick], config=cfg, chunk=chunk), T.pingpong_ref(pick=pick), ("sparse", chunk))
    with runtime.Context(0) as ctx:
        a = ctx.stall_census(w, seeds[0], len(seeds), config=cfg, chunk=700)
        b = ctx.stall_census(w, seeds=seeds, config=cfg)
        assert a.tobytes() == b.tobytes() == whole.tobytes() == want.tobytes()
    with pytest.raises(runtime.MadsimHipError, match="numpy.unique"):
        hip.stall_census(w, seeds=[5, 4], config=cfg)
    # every verdict counted: the passes are idle, the sites are the deadlocks' alone
    every = hip.stall_census(w, seeds[0], len(seeds), include=(A.PASS,) + FAILING, config=cfg)
    same(every, T.pingpong_ref(include=0xf), "all verdicts")
    assert every.n_idle[A.PASS] == every.n_counted[A.PASS] == verdicts.count(A.PASS) and every.sites.tobytes() == whole.sites.tobytes()
    # the shapes: six by the oracle (tests/test_stall.py says why not three), the three most frequent the three modes with both ends waiting
    dead = hip.stall_census(w, seeds[0], len(seeds), include=(A.DEADLOCK,), config=cfg)
    assert len(dead.shapes) == 6 and [n for _, n, _ in dead.shapes_of(A.DEADLOCK)] == [230, 184, 20, 10, 3, 1]
    _, at = T.pingpong_labels()
    for shape, n, first in dead.shapes_of(A.DEADLOCK):
        i = seeds.index(first)                                                      # the seed to replay has that shape
        (res, recs), = hip.post_mortem(w, [first], config=cfg)
        assert runtime.stall_shape(recs) == shape == R.shape(T.pingpong_sites(tables[i])) and res.verdict == A.DEADLOCK
    # "which task is waiting, and on what": every deadlock has its main in a join, and a client in its recv_from
    assert sum(int(r["n_seeds"][A.DEADLOCK]) for k in range(4) for r in dead.at(0, at[("join", k)], A.TASK_PARKED)) == dead.n_counted[A.DEADLOCK]
    c0 = dead.at(1, at[("recv", 1)], A.TASK_PARKED)
    assert len(c0) == 1 and dead.share(int(c0[0]["value"]), A.DEADLOCK) == runtime.Fraction(230 + 20 + 3 + 1, 448)
    assert " RECV " in dead.describe(w)[int(c0[0]["value"])]
    # no shapes pass: the same sites and totals
    bare = hip.stall_census(w, seeds[0], len(seeds), config=cfg, max_shapes=0)
    assert len(bare.shapes) == 0 and bare.sites.tobytes() == whole.sites.tobytes() and bare.n_counted == whole.n_counted
    # one site, or one shape, more than the cap: nothing is reported
    for kw in (dict(max_sites=len(want.sites) - 1), dict(max_shapes=len(want.shapes) - 1)):
        with pytest.raises(runtime.MadsimHipError, match="max_sites / max_shapes"):
            hip.stall_census(w, seeds[0], len(seeds), config=cfg, **kw)
    same(hip.stall_census(w, seeds[0], len(seeds), config=cfg, max_sites=len(want.sites), max_shapes=len(want.shapes)), want, "caps exactly met")


# ---- 2. directed workloads: every seed gives the hand-written table ------------------------------------------------------------------------------
N = 65


def run_case(hip, case, seeds, task_cap=32):
    w, lim, verdict, want = case
    got = hip.post_mortem(w, seeds, task_cap=task_cap, limits=lim, resolve=False, lengths=True)
    for s, (res, recs, true_len) in zip(seeds, got):
        assert res.verdict == verdict, (s, res.astuple())
        assert true_len == len(want) and [int(x) for x in recs] == want[:task_cap], (s, [runtime.task_fields(x) for x in recs], [runtime.task_fields(x) for x in want])
    import oracle
    ref, _ = oracle.run_batch(w, seeds[0], len(seeds), limits=lim)
    assert [r.astuple() for r, _, _ in got] == [tuple(int(x) for x in ref[i]) for i in range(len(seeds))]


@pytest.mark.parametrize("name", ["leak", "panic", "abort", "fused_assert", "assert_alone"])
def test_directed_small(hip, name):
    case = {"leak": SW.leak, "panic": SW.panic, "abort": SW.abort, "fused_assert": SW.fused_assert, "assert_alone": lambda: SW.fused_assert(True)}[name]()
    run_case(hip, case, list(range(1, N + 1)))


@pytest.mark.parametrize("tier", SW.TIERS)
def test_one_task_parked_in_every_awaiting_op_under_a_time_limit(hip, tier):
    """The test that pins what `pc` holds: every awaiting op of the tier's trace build, each PARKED at its own instruction; the alarm QUEUED."""
    case = SW.time_limit(tier)
    w, lim, _, want = case
    seeds = SW.time_limit_seeds(w, lim, N)
    got = hip.post_mortem(w, seeds, task_cap=32, limits=lim, resolve=False, lengths=True)
    import oracle
    for s, (res, recs, true_len) in zip(seeds, got):
        assert res.astuple() == tuple(int(x) for x in oracle.run_batch(w, s, 1, limits=lim)[0][0]), s
        assert res.verdict == A.TIME_LIMIT and true_len == len(want) and [int(x) for x in recs] == want, \
            (tier, s, [runtime.describe(w, x) for x in recs], [runtime.describe(w, x) for x in want])
    sc = hip.stall_census(w, seeds=sorted(seeds), limits=lim, include=(A.TIME_LIMIT,))
    assert len(sc.shapes) == 1 and len(sc.sites) == len(want) and (sc.sites["n_seeds"][:, A.TIME_LIMIT] == N).all()
    assert len(sc.at(len(want) - 1, R.pc(want[-1]), A.TASK_QUEUED)) == 1            # the alarm


@pytest.mark.parametrize("children", [63, 64, 65])
def test_crowds_around_a_task_cap_of_64(hip, children):
    case = SW.crowd(children)
    w, lim, _, want = case
    seeds = list(range(1, N + 1))
    run_case(hip, case, seeds, task_cap=64)
    run_case(hip, case, seeds, task_cap=254)
    for cap in (64, 254):
        sc = hip.stall_census(w, 1, N, task_cap=cap, limits=lim, resolve=False)
        ref = R.census_of_lists([want] * N, [A.PANIC] * N, seeds, 0xe, cap)
        same(sc, ref, (children, cap))
        assert sc.n_truncated == (N if len(want) > cap else 0) and sc.n_tasks == N * min(len(want), cap) and len(sc.shapes) == 1
        parked = sc.at(1, R.pc(want[1]), A.TASK_PARKED)[0]
        assert int(parked["max_per_seed"]) == min(children, cap - 1) and int(parked["n_seeds"][A.PANIC]) == N


# ---- 3. the conventions of task_states ---------------------------------------------------------------------------------------------------------
def test_task_states_conventions(hip):
    w, cfg, seeds, tables, verdicts, results, _ = T.pingpong_truth()
    L = runtime.lib()
    dead = [i for i, v in enumerate(verdicts) if v == A.DEADLOCK]
    five = next(i for i in dead if len(tables[i]) == 5)
    idx = [dead[0], 0, five, dead[0], dead[1], five, 1]                            # any order, duplicates
    s = np.array([seeds[i] for i in idx], dtype=np.uint64)
    n, lim = len(idx), A.Limits()
    sp = s.ctypes.data_as(C.POINTER(C.c_uint64))
    p = lambda a: a.ctypes.data_as(C.c_void_p)                                      # noqa: E731
    for cap in (8, 3, 1):                                                           # a cap below some rows: the prefix, the true length, zeros behind
        rows, lens, out = np.full((n, cap), 0xA5A5, dtype=np.uint64), np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=A.RESULT_DTYPE)
        assert L.madsim_hip_task_states(w.ref(), C.byref(cfg), sp, n, C.byref(lim), p(rows), cap, p(lens), p(out)) == 0
        for j, i in enumerate(idx):
            want = [R.word(*r) for r in tables[i]]
            assert int(lens[j]) == len(want) and [int(x) for x in rows[j]] == (want + [0] * cap)[:cap], (cap, j)
            assert tuple(int(x) for x in out[j]) == results[i].astuple()
    lens2, out2 = np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=A.RESULT_DTYPE)      # cap 0 with NULL: the counts alone
    assert L.madsim_hip_task_states(w.ref(), C.byref(cfg), sp, n, C.byref(lim), None, 0, p(lens2), p(out2)) == 0
    assert lens2.tobytes() == lens.tobytes() and out2.tobytes() == out.tobytes()
    assert L.madsim_hip_task_states(w.ref(), C.byref(cfg), sp, n, C.byref(lim), None, 0, None, None) == 0
    # `out` is what trace_seeds gives for the same seeds, trace_hash included; and under no_trace_hash both zero it
    for no_hash in (0, 1):
        lim2 = A.Limits(); lim2.no_trace_hash = no_hash
        out3, out4 = np.zeros(n, dtype=A.RESULT_DTYPE), np.zeros(n, dtype=A.RESULT_DTYPE)
        assert L.madsim_hip_trace_seeds(w.ref(), C.byref(cfg), sp, n, C.byref(lim2), None, 0, None, 0, None, None, p(out3)) == 0
        assert L.madsim_hip_task_states(w.ref(), C.byref(cfg), sp, n, C.byref(lim2), None, 0, p(lens2), p(out4)) == 0
        assert out3.tobytes() == out4.tobytes() and bool((out4["trace_hash"] == 0).all()) == bool(no_hash)
    # a runner verdict: an empty row, and the verdict is the whole answer; the resolve rounds settle it
    tight = A.Limits()
    tight.heap_lds_slots, tight.heap_spill_slots = 2, 0
    got = hip.post_mortem(w, [seeds[i] for i in idx], config=cfg, limits=tight, resolve=False, lengths=True)
    assert all(r.verdict == A.OVERFLOW and len(t) == 0 and ln == 0 for r, t, ln in got), [(r.verdict, ln) for r, _, ln in got]
    got = hip.post_mortem(w, [seeds[i] for i in idx], config=cfg, limits=tight, resolve=True)
    for (r, t), i in zip(got, idx):
        assert r.astuple() == results[i].astuple() and [int(x) for x in t] == [R.word(*x) for x in tables[i]]
    raw = hip.stall_census(w, seeds[0], 300, config=cfg, limits=tight, chunk=128, resolve=False)
    assert raw.n_runner == 300 and [int(x) for x in raw.runner_seeds] == seeds[:300] and len(raw.sites) == len(raw.shapes) == 0 and raw.n_counted == (0, 0, 0, 0)
    same(hip.stall_census(w, seeds[0], 300, config=cfg, limits=tight, chunk=128, resolve=True), T.pingpong_ref(pick=range(300)), "resolved")
    with runtime.Context(0) as ctx:
        (r, t), = ctx.post_mortem(w, [seeds[five]], config=cfg)
        assert [int(x) for x in t] == [R.word(*x) for x in tables[five]]


# ---- 4. the fuzz blocks: what follows from the program table and the oracle's 48 bytes alone ----------------------------------------------------------
# The ops whose poll can return Pending, from the program text of k_poll.h — not from what the device reported.  The receive family, the sleeps, join,
# accept1, the channel receive, the typed call, tick, ctrl_c and the selects wait for an event; YIELD returns Pending once by definition; BIND, SEND,
# REPLY, CONNECT and RPC_REPLY begin with NetSim::rand_delay (net/mod.rs:287-292), a Sleep of its own during which the task stands at that op.
# (Under DEADLOCK no timer is left, so a task cannot in fact stand in a delay stage: the set is the issue's wider "can return Pending".)
PENDING_OPS = {A.OP[k] for k in ("SLEEP", "SLEEP_UNTIL", "SLEEP_RAND", "RECV", "RECV_TIMEOUT", "JOIN", "ACCEPT", "CRECV", "RPC_CALL", "YIELD", "BIND", "SEND",
                                 "REPLY", "CONNECT", "RPC_REPLY", "TICK", "RECV_OR_TICK", "RECV_TIMEOUT_AT", "CTRL_C", "RECV_OR_CTRL_C")}


def prog_of_pc(w):
    """pc -> the program whose body holds it (bodies are laid out one after another, in program order)."""
    entries = sorted((w.progs[i].entry, i) for i in range(w.struct.n_progs))
    out = {}
    for j, (e, i) in enumerate(entries):
        for pc in range(e, entries[j + 1][0] if j + 1 < len(entries) else w.struct.n_insns):
            out[pc] = i
    return out


@pytest.mark.parametrize("name", sorted(TO.BLOCKS))
def test_fuzz_blocks(hip, name):
    n = n_records = 0
    states = set()
    for k, w, cfg, lim, desc, seeds, want in TO.block_truth(name):
        what = f"block {name!r} program {k}: {desc}"
        inside = prog_of_pc(w)
        for s, (res, recs), (_, ref) in zip(seeds, hip.post_mortem(w, seeds, task_cap=64, config=cfg, limits=lim, resolve=True), want):
            assert res.astuple() == ref.astuple(), (what, s, res.astuple(), ref.astuple())
            fields = [runtime.task_fields(x) for x in recs]
            if A.is_runner_verdict(res.verdict):
                assert not fields, (what, s)
                continue
            for st, prog, pc, _, _ in fields:
                assert 1 <= st <= 4 and prog < w.struct.n_progs and inside.get(pc) == prog, (what, s, fields)
                states.add(st)
            n_panicked = sum(st == A.TASK_PANICKED for st, *_ in fields)
            assert n_panicked == (1 if res.verdict == A.PANIC else 0), (what, s, fields)
            if res.verdict == A.DEADLOCK:
                assert all(st != A.TASK_QUEUED for st, *_ in fields) and fields, (what, s, fields)
                assert all(w.insns[pc].op in PENDING_OPS for _, _, pc, _, _ in fields), (what, s, [runtime.describe(w, x) for x in recs])
            if res.verdict == A.PASS:
                assert all(prog != 0 for _, prog, *_ in fields), (what, s, fields)
            n += 1
            n_records += len(fields)
    assert n > 0 and n_records > 0 and A.TASK_PARKED in states, (name, n, n_records, states)


# ---- 5. the paths the feature leaves alone, behind a task-log launch on the same context ------------------------------------------------------------
def test_unchanged_paths_return_what_the_oracle_implies(hip):
    w, cfg, seeds, obs, verdicts = TC.truth("pingpong")
    hip.post_mortem(w, seeds[:100], config=cfg)                                     # the trace set now holds task rows
    traces = hip.trace_seeds(w, seeds[:300], cfg, obs_cap=8, log_cap=16)
    import oracle
    for t, s, o in zip(traces, seeds, obs):
        log, res = oracle.trace_seed(w, s, cfg)
        assert t.observations == list(o) and t.result.astuple() == res.astuple() and t.log == log[:16] and t.log_len == len(log), s
    assert hip.census(w, seeds[0], len(seeds), config=cfg).tobytes() == TC.ref_of("pingpong").tobytes()
    hip.stall_census(w, seeds[0], 200, config=cfg)
    assert hip.census(w, seeds[0], len(seeds), config=cfg, chunk=300).tobytes() == TC.ref_of("pingpong").tobytes()
    pw, pcfg, pseeds, _, _ = TPS.truth("probe")
    got = hip.probe_sets(pw, TPS.PROBE_VOCAB, pseeds[0], len(pseeds), config=pcfg)
    assert got.tobytes() == TPS.ref_of("probe", TPS.PROBE_VOCAB).tobytes()
    got = hip.probe_order(pw, TPO.PROBE_VOCAB, pseeds[0], len(pseeds), config=pcfg)
    assert got.tobytes() == TPO.ref_of("probe", TPO.PROBE_VOCAB).tobytes()


# ---- 6. the example agrees with the Python call ---------------------------------------------------------------------------------------------------
def test_the_example_agrees_with_the_python_call(hip):
    exe = os.path.join(ROOT, "examples", "stall_test")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", os.path.join(ROOT, "examples", "stall_test.cpp"), "-o", exe,
                           "-L" + os.path.join(ROOT, "madsim_amd"), "-lmadsim_hip", "-Wl,-rpath," + os.path.join(ROOT, "madsim_amd")])
    from tests import groups_ref as G
    n = 4096
    out = subprocess.run([exe], env=dict(os.environ, MADSIM_TEST_SEED=str(G.SEED0), MADSIM_TEST_NUM=str(n)), capture_output=True, text=True, timeout=120)
    assert out.returncode == 101, (out.returncode, out.stderr)                       # (deadlocks were found: cargo test's exit code for a failed test)
    w, cfg, seeds, _, _, _, _ = T.pingpong_truth()
    sc = hip.stall_census(w, G.SEED0, n, include=(A.DEADLOCK,), config=cfg)
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("shape ")]
    assert len(lines) == len(sc.shapes)
    for ln, (shape, cnt, first) in zip(lines, sc.shapes_of(A.DEADLOCK)):
        assert ln.split()[:7] == ["shape", f"{shape:016x}", "seeds", str(cnt), "replay", "seed", str(first)], (ln, shape, cnt, first)
    assert f"{sc.n_counted[A.DEADLOCK]} of {n} seeds deadlock" in out.stdout
