"""The probe-set census through the public calls (runtime.probe_sets, Context.probe_sets, madsim_hip_probe_sets_range / _seeds, the C++
example) on the device.  The truth is never the code under test: it is the oracle's observe_seed lists fed to tests/sets_ref.py — the
directed inputs of tests/test_probe_sets.py, which proves by the oracle alone that they are not vacuous — and every comparison is of whole
reports, byte for byte: the same bytes whatever the chunk size, the form (range or list), the context and the run."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from madsim_amd import _abi as A
from madsim_amd import runtime
from tests import sets_ref as R
from tests import test_probe_sets as T

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def same(got, want, tag):
    assert got.n_counted == want.n_counted and got.n_runner == want.n_runner, (tag, got.n_counted, want.n_counted, got.n_runner, want.n_runner)
    assert [int(s) for s in got.runner_seeds] == list(want.runner_seeds), tag
    assert got.sets.tobytes() == want.sets.tobytes(), (tag, got.sets, want.sets)
    assert got.tobytes() == want.tobytes(), tag
    assert tuple(int(x) for x in got.sets["n_seeds"].sum(axis=0)) == got.n_counted if len(got.sets) else sum(got.n_counted) == 0, tag


# ---- 1. the probe ping-pong: chunks, forms, contexts, lists ---------------------------------------------------------------------------------
@pytest.mark.parametrize("vocab", [T.PROBE_VOCAB, T.PAIR0_VOCAB])
@pytest.mark.parametrize("chunk", [0, 1, 64, 777])
def test_probe_pingpong_whatever_the_chunk(hip, vocab, chunk):
    w, cfg, seeds, _, _ = T.truth("probe")
    n = 300 if chunk == 1 else len(seeds)                                          # (one seed per launch: the first 300)
    same(hip.probe_sets(w, vocab, seeds[0], n, config=cfg, chunk=chunk), T.ref_of("probe", vocab, pick=range(n)), (vocab, chunk))


def test_the_four_sets_and_what_the_marginals_hide(hip):
    w, cfg, seeds, _, _ = T.truth("probe")
    got = hip.probe_sets(w, T.PROBE_VOCAB, seeds[0], len(seeds), config=cfg)
    assert [(got.values_of(e["set"]), tuple(int(x) for x in e["n_seeds"])) for e in got.sets] == [
        ((0x10, 0x11), (0, 0, 427, 0)), ((0x10, 0x11, 0x20), (0, 0, 496, 0)), ((0x10, 0x11, 0x21), (0, 0, 506, 0)), ((0x10, 0x11, 0x20, 0x21), (571, 0, 0, 0))]
    assert got.count(all_of=(0x20, 0x21), verdicts=A.PASS) == got.n_counted[A.PASS] == 571 and got.count(all_of=(0x20, 0x21), verdicts=(1, 2, 3)) == 0
    assert got.count(all_of=(0x20,)) == 1067 and got.count(all_of=(0x20,), verdicts=A.DEADLOCK) == 496 and got.count(all_of=(0x30,)) == 0
    assert got.mixed() == [] and got.failing_share(all_of=(0x20,), none_of=(0x21,))[0] == 1
    pair0 = hip.probe_sets(w, T.PAIR0_VOCAB, seeds[0], len(seeds), config=cfg)
    assert [m[0] for m in pair0.mixed()] == [A.PROBE_SET_OTHER | 0b11] and pair0.count(other=False) == 0
    # the cover, re-run as a corpus: it reaches every reached value
    cover = got.cover()
    again = hip.probe_sets(w, T.PROBE_VOCAB, seeds=cover, config=cfg)
    assert len(cover) == 1 and again.count(all_of=(0x10, 0x11, 0x20, 0x21)) == 1


def test_list_form_and_a_second_context_give_the_same_bytes(hip):
    w, cfg, seeds, _, _ = T.truth("probe")
    want = T.ref_of("probe", T.PROBE_VOCAB)
    dense = hip.probe_sets(w, T.PROBE_VOCAB, seeds=np.array(seeds, dtype=np.uint64), config=cfg, chunk=100)
    same(dense, want, "dense list")
    with runtime.Context(0) as ctx:
        a = ctx.probe_sets(w, T.PROBE_VOCAB, seeds[0], len(seeds), config=cfg, chunk=300)
        b = ctx.probe_sets(w, T.PROBE_VOCAB, seeds=seeds, config=cfg)
        assert a.tobytes() == b.tobytes() == dense.tobytes() == want.tobytes()
    again = hip.probe_sets(w, T.PROBE_VOCAB, seeds[0], len(seeds), config=cfg)
    assert again.tobytes() == want.tobytes()


def test_a_sparse_list_and_the_include_masks(hip):
    w, cfg, seeds, _, _ = T.truth("probe")
    pick = list(range(0, len(seeds), 3))                                           # every third seed
    for chunk in (0, 33):
        same(hip.probe_sets(w, T.PROBE_VOCAB, seeds=[seeds[i] for i in pick], config=cfg, chunk=chunk), T.ref_of("probe", T.PROBE_VOCAB, pick=pick),
             ("sparse", chunk))
    with pytest.raises(runtime.MadsimHipError, match="numpy.unique"):
        hip.probe_sets(w, T.PROBE_VOCAB, seeds=[5, 4], config=cfg)
    for include in ((A.PASS,), (A.PANIC, A.DEADLOCK), A.DEADLOCK):
        mask = sum(1 << v for v in ((include,) if isinstance(include, int) else include))
        same(hip.probe_sets(w, T.PROBE_VOCAB, seeds[0], len(seeds), include=include, config=cfg, chunk=500),
             T.ref_of("probe", T.PROBE_VOCAB, include=mask), include)


# ---- 2. the looping workload: TRUNCATED on every seed at 256, on none at 512 ------------------------------------------------------------------
@pytest.mark.parametrize("obs_cap,chunk", [(256, 0), (256, 7), (512, 0), (130, 64), (1, 0), (A.CENSUS_MAX_OBS_CAP, 0)])
def test_looping_workload(hip, obs_cap, chunk):
    w, cfg, seeds, _, _ = T.truth("loop")
    got = hip.probe_sets(w, T.LOOP_VOCAB, seeds[0], len(seeds), obs_cap=obs_cap, config=cfg, chunk=chunk)
    same(got, T.ref_of("loop", T.LOOP_VOCAB, obs_cap=obs_cap), (obs_cap, chunk))
    assert got.count(truncated=True) == (len(seeds) if obs_cap < 300 else 0) and got.count(truncated=False) == (0 if obs_cap < 300 else len(seeds))


# ---- 3. runner verdicts -----------------------------------------------------------------------------------------------------------------------
def test_runner_verdicts_are_tallied_listed_and_settled(hip):
    """Limits nobody fits: the first pass answers every seed with MADSIM_OVERFLOW.  Without resolve rounds they are all tallied and listed,
    ascending, and nothing is counted; with them the report is the oracle's."""
    w, cfg, seeds, _, _ = T.truth("probe")
    n = 500
    lim = A.Limits()
    lim.heap_lds_slots, lim.heap_spill_slots = 2, 0
    first, _ = hip.run_batch(w, seeds[0], 64, cfg, lim)
    assert (first["verdict"] == A.OVERFLOW).all()
    raw = hip.probe_sets(w, T.PROBE_VOCAB, seeds[0], n, config=cfg, limits=lim, chunk=128, resolve=None)
    assert raw.n_runner == n and [int(s) for s in raw.runner_seeds] == seeds[:n] and len(raw.sets) == 0 and raw.n_counted == (0, 0, 0, 0)
    # the C call with room for ten: the ten smallest, ascending
    sets, runner, vocab = np.zeros(16, dtype=A.PROBE_SET_DTYPE), np.full(12, 0xA5A5, dtype=np.uint64), np.array(T.PROBE_VOCAB, dtype=np.uint64)
    ps = A.ProbeSets(include=T.ALL, obs_cap=16, n_vocab=len(vocab), cap=16, runner_cap=10)
    ps.vocab, ps.sets = vocab.ctypes.data_as(C.POINTER(C.c_uint64)), sets.ctypes.data_as(C.POINTER(A.ProbeSet))
    ps.runner_seeds = runner.ctypes.data_as(C.POINTER(C.c_uint64))
    assert runtime.lib().madsim_hip_probe_sets_range(w.ref(), C.byref(cfg), seeds[0], n, 128, C.byref(lim), C.byref(ps)) == 0
    assert (ps.n_runner, ps.n_runner_listed, ps.n_sets) == (n, 10, 0) and list(runner) == seeds[:10] + [0xA5A5, 0xA5A5]
    same(hip.probe_sets(w, T.PROBE_VOCAB, seeds[0], n, config=cfg, limits=lim, chunk=128, resolve=True), T.ref_of("probe", T.PROBE_VOCAB, pick=range(n)),
         "resolved")


# ---- 4. more distinct sets than the cap -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chunk", [0, 1, 64])
def test_more_sets_than_max_sets_reports_nothing(hip, chunk):
    w, cfg, seeds, _, _ = T.truth("probe")
    n = 400 if chunk == 1 else len(seeds)
    assert len(T.ref_of("probe", T.PROBE_VOCAB, pick=range(n)).sets) == 4
    for max_sets in (1, 3):
        with pytest.raises(runtime.MadsimHipError, match="distinct probe sets"):
            hip.probe_sets(w, T.PROBE_VOCAB, seeds[0], n, max_sets=max_sets, config=cfg, chunk=chunk)
    sets, vocab = np.zeros(1, dtype=A.PROBE_SET_DTYPE), np.array(T.PROBE_VOCAB, dtype=np.uint64)
    ps = A.ProbeSets(include=T.ALL, obs_cap=256, n_vocab=len(vocab), cap=1, n_sets=77, n_runner=77)
    ps.n_counted[0] = 77
    ps.vocab, ps.sets = vocab.ctypes.data_as(C.POINTER(C.c_uint64)), sets.ctypes.data_as(C.POINTER(A.ProbeSet))
    rc = runtime.lib().madsim_hip_probe_sets_range(w.ref(), C.byref(cfg), seeds[0], n, chunk, C.byref(A.Limits()), C.byref(ps))
    assert rc == T.E_LIMITS and (ps.n_sets, tuple(ps.n_counted), ps.n_runner, ps.n_runner_listed) == (0, (0, 0, 0, 0), 0, 0)      # nothing is reported
    # with room it is a report like any other, and the table the failed calls used is clean
    same(hip.probe_sets(w, T.PROBE_VOCAB, seeds[0], n, max_sets=4, config=cfg, chunk=chunk), T.ref_of("probe", T.PROBE_VOCAB, pick=range(n)), ("room", chunk))


# ---- 5. vocabulary=None, and the census beside it ----------------------------------------------------------------------------------------------
def test_no_vocabulary_takes_the_census_values_and_the_census_is_left_alone(hip):
    w, cfg, seeds, _, _ = T.truth("probe")
    with runtime.Context(0) as ctx:
        before = ctx.census(w, seeds[0], len(seeds), config=cfg)
        vocab = [int(v) for v in before.values["value"]]
        assert vocab == [0x10, 0x11, 0x20, 0x21]
        auto = ctx.probe_sets(w, None, seeds[0], len(seeds), config=cfg)
        explicit = ctx.probe_sets(w, vocab, seeds[0], len(seeds), config=cfg)
        after = ctx.census(w, seeds[0], len(seeds), config=cfg)
    assert auto.vocabulary == tuple(vocab) and auto.tobytes() == explicit.tobytes() == T.ref_of("probe", vocab).tobytes()
    assert before.tobytes() == after.tobytes()
    assert hip.probe_sets(w, seed0=seeds[0], total=len(seeds), config=cfg).tobytes() == explicit.tobytes()
    for v in vocab:                                                                # the marginals of the sets are the census's rows
        assert [explicit.count(all_of=(v,), verdicts=k) for k in range(4)] == [int(x) for x in before.row(v)["n_seeds"]], hex(v)


# ---- 6. the example ----------------------------------------------------------------------------------------------------------------------------
def test_the_example_prints_the_four_sets_and_the_line(hip):
    """examples/probe_sets_test.cpp (C++ Builder mirror): every set with its per-verdict counts and a seed to replay, the conjunction and the cover."""
    env = dict(os.environ, MADSIM_TEST_SEED="0", MADSIM_TEST_NUM="2000")
    out = subprocess.run([os.path.join(ROOT, "examples", "probe_sets_test")], env=env, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    want = T.ref_of("probe", T.PROBE_VOCAB)
    lines = re.findall(r"set \{((?: 0x[0-9a-f]+)*) \}: (\d+) pass, (\d+) panic, (\d+) deadlock, (\d+) time-limit seeds;(.*)", out.stdout)
    assert [(sum(1 << T.PROBE_VOCAB.index(int(x, 16)) for x in names.split()), int(a), int(b), int(c), int(d)) for names, a, b, c, d, _ in lines] == \
        [(int(e["set"]), *(int(x) for x in e["n_seeds"])) for e in want.sets]
    replay = [[int(s) for s in re.findall(r"MADSIM_TEST_SEED=(\d+)", rest)] for *_, rest in lines]
    assert replay == [[int(e["first_seed"][k]) for k in range(4) if int(e["n_seeds"][k])] for e in want.sets]
    assert "passes exactly when 0x20 and 0x21 are both reached (571 seeds; none of the 1429 failing seeds reaches both)" in out.stdout
    assert re.search(r"cover: (\d+)\n", out.stdout).group(1) == str(int(want.sets[-1]["first_seed"][A.PASS]))
    assert "2000 seeds from 0: 571 pass, 0 panic, 1429 deadlock, 0 time-limit; 4 probe sets" in out.stdout
