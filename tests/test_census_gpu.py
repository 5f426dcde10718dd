"""The observation census through the public calls (runtime.census, Context.census, madsim_hip_census_range / _seeds, the C++ example) on
the device.  The truth is never the code under test: it is the oracle's observe_seed lists fed to tests/census_ref.py — for the traced
lossy ping-pong over 2 000 seeds, the looping workload that overruns obs_cap, and every program of tests/test_observe.py's fuzz blocks
(the trace builds of all six families) — and every comparison is of whole reports, byte for byte: the same bytes whatever the chunk
size, the form (range or list), the context and the run."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from madsim_amd import _abi as A
from madsim_amd import runtime
from tests import census_ref as R
from tests import test_census as T
from tests import test_observe as TO

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def same(got, want, tag):
    assert got.n_counted == want.n_counted and got.n_silent == want.n_silent, (tag, got.n_counted, want.n_counted, got.n_silent, want.n_silent)
    assert (got.n_truncated, got.n_observations, got.n_runner) == (want.n_truncated, want.n_observations, want.n_runner), tag
    assert [int(s) for s in got.runner_seeds] == list(want.runner_seeds), tag
    assert got.values.tobytes() == want.values.tobytes(), (tag, got.values, want.values)
    assert got.tobytes() == want.tobytes(), tag
    assert int(got.values["n_total"].sum()) == got.n_observations, tag


# ---- 1. the ping-pong range: chunks, forms, contexts, lists, masks, caps ---------------------------------------------------------------------
@pytest.mark.parametrize("chunk", [64, 100, 0])
def test_pingpong_range_whatever_the_chunk(hip, chunk):
    w, cfg, seeds, _, _ = T.truth("pingpong")
    same(hip.census(w, seeds[0], len(seeds), config=cfg, chunk=chunk), T.ref_of("pingpong"), chunk)


def test_one_seed_per_chunk(hip):
    w, cfg, seeds, _, _ = T.truth("pingpong")
    same(hip.census(w, seeds[0], 200, config=cfg, chunk=1), T.ref_of("pingpong", pick=range(200)), "chunk 1")


def test_list_form_and_a_second_context_give_the_same_bytes(hip):
    w, cfg, seeds, _, _ = T.truth("pingpong")
    want = T.ref_of("pingpong")
    dense = hip.census(w, seeds=np.array(seeds, dtype=np.uint64), config=cfg, chunk=100)
    same(dense, want, "dense list")
    with runtime.Context(0) as ctx:
        a = ctx.census(w, seeds[0], len(seeds), config=cfg, chunk=300)
        b = ctx.census(w, seeds=seeds, config=cfg)
        assert a.tobytes() == b.tobytes() == dense.tobytes() == want.tobytes()
    again = hip.census(w, seeds[0], len(seeds), config=cfg)
    assert again.tobytes() == want.tobytes()


def test_a_sparse_list(hip):
    w, cfg, seeds, _, _ = T.truth("pingpong")
    pick = sorted(set(range(0, len(seeds), 7)) | {1, 2, 3, len(seeds) - 1})
    for chunk in (0, 33):
        same(hip.census(w, seeds=[seeds[i] for i in pick], config=cfg, chunk=chunk), T.ref_of("pingpong", pick=pick), ("sparse", chunk))
    with pytest.raises(runtime.MadsimHipError, match="numpy.unique"):
        hip.census(w, seeds=[5, 4], config=cfg)


@pytest.mark.parametrize("include", [(A.PASS,), (A.PANIC, A.DEADLOCK), (A.PASS, A.DEADLOCK, A.TIME_LIMIT), A.DEADLOCK])
def test_include_masks(hip, include):
    w, cfg, seeds, _, _ = T.truth("pingpong")
    mask = sum(1 << v for v in ((include,) if isinstance(include, int) else include))
    same(hip.census(w, seeds[0], len(seeds), include=include, config=cfg, chunk=500), T.ref_of("pingpong", include=mask), include)


def test_obs_cap_below_some_rows(hip):
    w, cfg, seeds, obs, _ = T.truth("pingpong")
    assert max(len(o) for o in obs) == 2
    want = T.ref_of("pingpong", obs_cap=1)
    assert want.n_truncated > 0
    same(hip.census(w, seeds[0], len(seeds), obs_cap=1, config=cfg), want, "obs_cap 1")


# ---- 2. the looping workload: three rounds of 64 and more, truncation, a value in every round --------------------------------------------------
@pytest.mark.parametrize("obs_cap,chunk", [(T.LOOP_OBS_CAP, 0), (T.LOOP_OBS_CAP, 7), (512, 0), (130, 64), (A.CENSUS_MAX_OBS_CAP, 0)])
def test_looping_workload(hip, obs_cap, chunk):
    w, cfg, seeds, _, _ = T.truth("loop")
    want = T.ref_of("loop", obs_cap=obs_cap)
    got = hip.census(w, seeds[0], len(seeds), obs_cap=obs_cap, config=cfg, chunk=chunk)
    same(got, want, (obs_cap, chunk))
    assert int(got.row(7)["max_per_seed"]) == min(obs_cap, 300) // 2 and got.reached(7) == len(seeds) and got.n_truncated == (len(seeds) if obs_cap < 300 else 0)


# ---- 3. the fuzz blocks: the trace builds of all six families ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(TO.BLOCKS))
def test_fuzz_blocks(hip, name):
    """One census per program of the block over its 16 seeds, in the list form, every other program in chunks of five; seeds the first pass
    leaves with a runner verdict are settled by the resolve rounds, a pinned step cap stays a runner verdict on both sides."""
    n_values = 0
    for k, w, cfg, lim, desc, seeds, truth in TO.block_truth(name):
        obs, verdicts = [o for o, _ in truth], [r.verdict for _, r in truth]
        want = R.census_of_lists(obs, verdicts, seeds, T.ALL, 256)
        got = hip.census(w, seeds=seeds, config=cfg, limits=lim, chunk=(0, 5)[k % 2])
        same(got, want, (desc, seeds[0]))
        n_values += len(want.values)
    assert n_values > 0, (name, n_values)                                          # (by the oracle: the block traces something)


# ---- 4. runner verdicts ------------------------------------------------------------------------------------------------------------------------
def test_runner_verdicts_are_tallied_listed_and_settled(hip):
    """Limits nobody fits: the first pass answers every seed with MADSIM_OVERFLOW.  Without resolve rounds they are all tallied and listed,
    ascending, and nothing is counted; with them the census is the oracle's."""
    w, cfg, seeds, _, _ = T.truth("pingpong")
    n = 500
    lim = A.Limits()
    lim.heap_lds_slots, lim.heap_spill_slots = 2, 0
    first, _ = hip.run_batch(w, seeds[0], 64, cfg, lim)
    assert (first["verdict"] == A.OVERFLOW).all()
    raw = hip.census(w, seeds[0], n, config=cfg, limits=lim, chunk=128, resolve=False)
    assert raw.n_runner == n and [int(s) for s in raw.runner_seeds] == seeds[:n] and len(raw.values) == 0
    assert raw.n_counted == raw.n_silent == (0, 0, 0, 0) and raw.n_observations == raw.n_truncated == 0
    # the C call with room for ten: the ten smallest, ascending
    values, runner = np.zeros(16, dtype=A.CENSUS_VALUE_DTYPE), np.full(12, 0xA5A5, dtype=np.uint64)
    cen = A.Census(include=T.ALL, obs_cap=16, cap=16, runner_cap=10)
    cen.values, cen.runner_seeds = values.ctypes.data_as(C.POINTER(A.CensusValue)), runner.ctypes.data_as(C.POINTER(C.c_uint64))
    assert runtime.lib().madsim_hip_census_range(w.ref(), C.byref(cfg), seeds[0], n, 128, C.byref(lim), C.byref(cen)) == 0
    assert (cen.n_runner, cen.n_runner_listed) == (n, 10) and list(runner) == seeds[:10] + [0xA5A5, 0xA5A5]
    same(hip.census(w, seeds[0], n, config=cfg, limits=lim, chunk=128, resolve=True), T.ref_of("pingpong", pick=range(n)), "resolved")


# ---- 5. more distinct values than the cap ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chunk", [0, 1, 7, 64])
def test_a_random_value_is_not_a_probe_vocabulary(hip, chunk):
    w, cfg, seeds, _, _ = T.truth("random")
    with pytest.raises(runtime.MadsimHipError, match="probe vocabulary"):
        hip.census(w, seeds[0], len(seeds), max_values=T.RANDOM_MAX_VALUES, config=cfg, chunk=chunk)
    values = np.zeros(T.RANDOM_MAX_VALUES, dtype=A.CENSUS_VALUE_DTYPE)
    cen = A.Census(include=T.ALL, obs_cap=256, cap=T.RANDOM_MAX_VALUES, n_values=77, n_observations=77)
    cen.values = values.ctypes.data_as(C.POINTER(A.CensusValue))
    rc = runtime.lib().madsim_hip_census_range(w.ref(), C.byref(cfg), seeds[0], len(seeds), chunk, C.byref(A.Limits()), C.byref(cen))
    assert rc == T.E_LIMITS and (cen.n_values, cen.n_observations, tuple(cen.n_counted), cen.n_runner) == (0, 0, (0, 0, 0, 0), 0)      # nothing is reported
    # with room it is a census like any other, and the table the failed calls used is clean
    same(hip.census(w, seeds[0], len(seeds), max_values=len(seeds), config=cfg, chunk=chunk), T.ref_of("random"), ("random", chunk))


# ---- 6. the example ----------------------------------------------------------------------------------------------------------------------------
def test_the_example_agrees_with_the_python_call(hip):
    """examples/probe_census_test.cpp (C++ Builder mirror): every probe with its per-verdict seed counts, and the expected probe that never fired."""
    env = dict(os.environ, MADSIM_TEST_SEED="0", MADSIM_TEST_NUM="3000")
    out = subprocess.run([os.path.join(ROOT, "examples", "probe_census_test")], env=env, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    got = hip.census(T.probe_pingpong_workload(), 0, 3000, config=A.Config.default(packet_loss_rate=0.002))
    lines = re.findall(r"probe 0x([0-9a-f]+): (\d+) pass, (\d+) panic, (\d+) deadlock, (\d+) time-limit seeds, (\d+) times, first at MADSIM_TEST_SEED=(\d+)", out.stdout)
    assert [(int(v, 16), int(a), int(b), int(c), int(d), int(t), int(s)) for v, a, b, c, d, t, s in lines] == \
        [(int(e["value"]), *(int(x) for x in e["n_seeds"]), int(e["n_total"]), int(e["first_seed"])) for e in got.values]
    assert [int(e["value"]) for e in got.values] == [0x10, 0x11, 0x20, 0x21] and got.n_counted[A.DEADLOCK] > 0
    assert got.reached(0x20) < got.reached(0x10) == 3000
    assert re.findall(r"probe 0x([0-9a-f]+) never fired", out.stdout) == ["30"] and got.never([0x10, 0x11, 0x20, 0x21, 0x30]) == [0x30]
    head = re.search(r"3000 seeds from 0: (\d+) pass, (\d+) panic, (\d+) deadlock, (\d+) time-limit; (\d+) silent, 4 probes", out.stdout)
    assert head and tuple(int(x) for x in head.groups()) == got.n_counted + (sum(got.n_silent),)
