"""The probe-order census through the public calls (runtime.probe_order, Context.probe_order, madsim_hip_probe_order_range / _seeds, the
C++ example) on the device.  The truth is never the code under test: it is the oracle's observe_seed lists fed to tests/order_ref.py — the
directed inputs of tests/test_probe_order.py, which proves by the oracle alone that they are not vacuous — and every comparison is of whole
reports, byte for byte: the same bytes whatever the chunk size, the form (range or list), the context and the run."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from madsim_amd import _abi as A
from madsim_amd import runtime
from tests import test_probe_order as T

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def same(got, want, tag):
    assert (got.n_counted, got.n_none, got.n_truncated, got.n_runner) == (want.n_counted, want.n_none, want.n_truncated, want.n_runner), tag
    assert [int(s) for s in got.runner_seeds] == list(want.runner_seeds), tag
    assert got.pairs.tobytes() == want.pairs.tobytes(), (tag, got.pairs, want.pairs)
    assert got.tobytes() == want.tobytes(), tag


# ---- 1. the probe ping-pong: chunks, forms, contexts, lists ---------------------------------------------------------------------------------
@pytest.mark.parametrize("chunk", [0, 1, 64, 1000])
def test_probe_pingpong_whatever_the_chunk(hip, chunk):
    w, cfg, seeds, _, _ = T.truth("probe")
    n = 300 if chunk == 1 else len(seeds)                                          # (one seed per launch: the first 300)
    same(hip.probe_order(w, T.PROBE_VOCAB, seeds[0], n, config=cfg, chunk=chunk), T.ref_of("probe", T.PROBE_VOCAB, pick=range(n)), chunk)


def test_the_cells_of_the_issue_and_the_readers(hip):
    w, cfg, seeds, _, _ = T.truth("probe")
    got = hip.probe_order(w, T.PROBE_VOCAB, seeds[0], len(seeds), config=cfg)
    P, D = A.PASS, A.DEADLOCK
    assert (got.before(0x10, 0x11, P), got.before(0x10, 0x11, D), got.before(0x11, 0x10, P), got.before(0x11, 0x10, D)) == (266, 723, 305, 706)
    assert (got.before(0x20, 0x21), got.before(0x21, 0x20), got.before(0x20, 0x10), got.reached(0x30)) == (286, 285, 0, 0)
    assert got.witness(0x10, 0x11, P) == 16 and got.witness(0x21, 0x20, P) == 19 and got.witness(0x20, 0x10, P) is None
    assert got.always_before(0x10, 0x20) and not got.always_before(0x10, 0x11) and got.both(0x20, 0x21) == 571 == got.n_counted[P]
    assert got.without(0x20, 0x21) == 496 and got.without(0x21, 0x20) == 506
    assert got.precedence() == [(0x10, 0x20), (0x10, 0x21), (0x11, 0x20), (0x11, 0x21)] and got.discriminating() == []


def test_list_form_and_contexts_give_the_same_bytes(hip):
    w, cfg, seeds, _, _ = T.truth("probe")
    want = T.ref_of("probe", T.PROBE_VOCAB)
    dense = hip.probe_order(w, T.PROBE_VOCAB, seeds=np.array(seeds, dtype=np.uint64), config=cfg, chunk=100)
    same(dense, want, "dense list")
    with runtime.Context(0) as ctx:                                                # a fresh context
        a = ctx.probe_order(w, T.PROBE_VOCAB, seeds[0], len(seeds), config=cfg, chunk=300)
        b = ctx.probe_order(w, T.PROBE_VOCAB, seeds=seeds, config=cfg)
        assert a.tobytes() == b.tobytes() == dense.tobytes() == want.tobytes()
    with runtime.Context(0) as ctx:                                                # one that has just run a census and a probe-set census
        cen = ctx.census(w, seeds[0], len(seeds), config=cfg)
        ps = ctx.probe_sets(w, T.PROBE_VOCAB, seeds[0], len(seeds), config=cfg)
        c = ctx.probe_order(w, T.PROBE_VOCAB, seeds[0], len(seeds), config=cfg)
        assert c.tobytes() == want.tobytes()
        assert ctx.census(w, seeds[0], len(seeds), config=cfg).tobytes() == cen.tobytes()
        assert ctx.probe_sets(w, T.PROBE_VOCAB, seeds[0], len(seeds), config=cfg).tobytes() == ps.tobytes()
        for v in T.PROBE_VOCAB[:4]:                                                # the diagonal is the census's rows
            assert [c.reached(v, k) for k in range(4)] == [int(x) for x in cen.row(v)["n_seeds"]], hex(v)
    assert hip.probe_order(w, T.PROBE_VOCAB, seeds[0], len(seeds), config=cfg).tobytes() == want.tobytes()


def test_a_sparse_list_and_the_include_masks(hip):
    w, cfg, seeds, _, _ = T.truth("probe")
    pick = list(range(0, len(seeds), 3))                                           # every third seed
    for chunk in (0, 33):
        same(hip.probe_order(w, T.PROBE_VOCAB, seeds=[seeds[i] for i in pick], config=cfg, chunk=chunk), T.ref_of("probe", T.PROBE_VOCAB, pick=pick),
             ("sparse", chunk))
    with pytest.raises(runtime.MadsimHipError, match="numpy.unique"):
        hip.probe_order(w, T.PROBE_VOCAB, seeds=[5, 4], config=cfg)
    for include in ((A.PASS,), (A.PANIC, A.DEADLOCK), A.DEADLOCK):
        mask = sum(1 << v for v in ((include,) if isinstance(include, int) else include))
        same(hip.probe_order(w, T.PROBE_VOCAB, seeds[0], len(seeds), include=include, config=cfg, chunk=500),
             T.ref_of("probe", T.PROBE_VOCAB, include=mask), include)


# ---- 2. the looping workload: cut at 256, whole at 512 ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("obs_cap,chunk", [(256, 0), (256, 1), (256, 64), (512, 0), (512, 1000), (130, 64), (1, 0), (A.CENSUS_MAX_OBS_CAP, 0)])
def test_looping_workload(hip, obs_cap, chunk):
    w, cfg, seeds, _, _ = T.truth("loop")
    got = hip.probe_order(w, T.LOOP_VOCAB, seeds[0], len(seeds), obs_cap=obs_cap, config=cfg, chunk=chunk)
    same(got, T.ref_of("loop", T.LOOP_VOCAB, obs_cap=obs_cap), (obs_cap, chunk))
    assert got.n_truncated == (len(seeds) if obs_cap < 300 else 0)


def test_the_reports_at_256_and_512_differ_only_in_n_truncated(hip):
    w, cfg, seeds, _, _ = T.truth("loop")
    cut, whole = (hip.probe_order(w, T.LOOP_VOCAB, seeds=seeds, obs_cap=c, config=cfg) for c in (256, 512))
    assert cut.pairs.tobytes() == whole.pairs.tobytes() and (cut.n_counted, cut.n_none, cut.n_runner) == (whole.n_counted, whole.n_none, whole.n_runner)
    assert (cut.n_truncated, whole.n_truncated) == (len(seeds), 0) and cut.always_before(7, 249) and cut.reached(100) == 0


# ---- 3. runner verdicts -----------------------------------------------------------------------------------------------------------------------
def test_runner_verdicts_are_tallied_listed_and_settled(hip):
    """Limits nobody fits: the first pass answers every seed with MADSIM_OVERFLOW.  Without resolve rounds they are all tallied and listed,
    ascending, and nothing is counted; with them the report is the oracle's — and what the per-seed ladder (trace_seeds, which settles
    its seeds the same way) gives."""
    w, cfg, seeds, _, _ = T.truth("probe")
    n = 500
    lim = A.Limits()
    lim.heap_lds_slots, lim.heap_spill_slots = 2, 0
    first, _ = hip.run_batch(w, seeds[0], 64, cfg, lim)
    assert (first["verdict"] == A.OVERFLOW).all()
    raw = hip.probe_order(w, T.PROBE_VOCAB, seeds[0], n, config=cfg, limits=lim, chunk=128, resolve=None)
    assert raw.n_runner == n and [int(s) for s in raw.runner_seeds] == seeds[:n] and len(raw.pairs) == 0 and raw.n_counted == (0, 0, 0, 0)
    # the C call with room for ten: the ten smallest, ascending
    pairs, runner, vocab = np.zeros(25, dtype=A.PROBE_ORDER_PAIR_DTYPE), np.full(12, 0xA5A5, dtype=np.uint64), np.array(T.PROBE_VOCAB, dtype=np.uint64)
    po = A.ProbeOrder(include=T.ALL, obs_cap=16, n_vocab=len(vocab), cap=25, runner_cap=10)
    po.vocab, po.pairs = vocab.ctypes.data_as(C.POINTER(C.c_uint64)), pairs.ctypes.data_as(C.POINTER(A.ProbeOrderPair))
    po.runner_seeds = runner.ctypes.data_as(C.POINTER(C.c_uint64))
    assert runtime.lib().madsim_hip_probe_order_range(w.ref(), C.byref(cfg), seeds[0], n, 128, C.byref(lim), C.byref(po)) == 0
    assert (po.n_runner, po.n_runner_listed, po.n_pairs) == (n, 10, 0) and list(runner) == seeds[:10] + [0xA5A5, 0xA5A5]
    settled = hip.probe_order(w, T.PROBE_VOCAB, seeds[0], n, config=cfg, limits=lim, chunk=128, resolve=True)
    same(settled, T.ref_of("probe", T.PROBE_VOCAB, pick=range(n)), "resolved")
    from tests import order_ref as R
    traces = hip.trace_seeds(w, seeds[:n], cfg, lim, obs_cap=256, log_cap=0, resolve=True)
    ladder = R.probe_order_of_lists([list(t.observations) for t in traces], [int(t.result.verdict) for t in traces], seeds[:n], T.ALL, 256, T.PROBE_VOCAB)
    same(settled, ladder, "the per-seed ladder")


# ---- 4. vocabulary=None, merge ----------------------------------------------------------------------------------------------------------------
def test_no_vocabulary_takes_the_census_values(hip):
    w, cfg, seeds, _, _ = T.truth("probe")
    vocab = [0x10, 0x11, 0x20, 0x21]
    auto = hip.probe_order(w, None, seeds[0], len(seeds), config=cfg)
    assert auto.vocabulary == tuple(vocab) and auto.tobytes() == T.ref_of("probe", vocab).tobytes()
    assert hip.probe_order(w, seed0=seeds[0], total=len(seeds), config=cfg).tobytes() == auto.tobytes()
    with runtime.Context(0) as ctx:
        assert ctx.probe_order(w, seeds=seeds[::2], config=cfg).tobytes() == T.ref_of("probe", vocab, pick=range(0, len(seeds), 2)).tobytes()
    from tests import test_census as TC
    with pytest.raises(runtime.MadsimHipError, match="vocabulary of 1..32"):      # a traced random value is not a vocabulary
        hip.probe_order(TC.random_value_workload(), None, 0, 200)


def test_merge_of_two_halves_is_the_whole(hip):
    w, cfg, seeds, _, _ = T.truth("probe")
    half = len(seeds) // 2
    a = hip.probe_order(w, T.PROBE_VOCAB, seeds[0], half, config=cfg)
    b = hip.probe_order(w, T.PROBE_VOCAB, seeds[half], len(seeds) - half, config=cfg)
    assert a.merge(b).tobytes() == b.merge(a).tobytes() == T.ref_of("probe", T.PROBE_VOCAB).tobytes()
    assert a.tobytes() != b.tobytes()


# ---- 5. the example ----------------------------------------------------------------------------------------------------------------------------
def test_the_example_prints_the_matrix_and_the_lines(hip):
    """examples/probe_order_test.cpp (C++ Builder mirror): the matrix per verdict, "0x10 always before 0x20", and both orders of
    (0x10, 0x11), each with its witness seed."""
    env = dict(os.environ, MADSIM_TEST_SEED="0", MADSIM_TEST_NUM="2000")
    out = subprocess.run([os.path.join(ROOT, "examples", "probe_order_test")], env=env, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    want = T.ref_of("probe", T.PROBE_VOCAB)
    n = T.cells(want, T.PROBE_VOCAB)
    for k, name in ((0, "pass"), (2, "deadlock")):
        block = re.search(r"\(diagonal: reached\), %s:\n((?:    .*\n)+)" % name, out.stdout)
        assert block, out.stdout
        rows = [[int(x) for x in ln.split()[1:]] for ln in block.group(1).splitlines()[1:]]
        assert rows == [[n.get((a, b), [0] * 4)[k] for b in T.PROBE_VOCAB] for a in T.PROBE_VOCAB], (name, rows)
    assert "0x10 always before 0x20" in out.stdout
    got = re.findall(r"0x(1[01]) before 0x(1[01]): (\d+) pass, (\d+) panic, (\d+) deadlock, (\d+) time-limit seeds;(.*)", out.stdout)
    first = T.cells(want, T.PROBE_VOCAB, "first_seed")
    assert [(int(a, 16), int(b, 16), [int(x) for x in c]) for a, b, *c, _ in got] == [(0x10, 0x11, n[(0x10, 0x11)]), (0x11, 0x10, n[(0x11, 0x10)])]
    assert [[int(s) for s in re.findall(r"MADSIM_TEST_SEED=(\d+)", rest)] for *_, rest in got] == [
        [first[c][k] for k in range(4) if n[c][k]] for c in ((0x10, 0x11), (0x11, 0x10))]
