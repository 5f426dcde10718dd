"""The observation census — which traced values the seeds of a range reach, by verdict (madsim_hip_census_range / _seeds, runtime.census) —
on the CPU: the numpy reference (tests/census_ref.py) against a dict-based restatement; the host fold (madsim_k_fold_census) over every
cut of an array into chunks, at `cap` and one over it; Census.merge; the surface and its argument errors, which need no device; and the
directed inputs that tests/test_census_gpu.py runs on the device, with the proof — by the oracle alone — that they are not vacuous."""
import ctypes as C
import functools
import inspect
import os
import subprocess

import numpy as np
import pytest

import oracle
from madsim_amd import _abi as A
from madsim_amd import runtime
from madsim_amd import workload as W
from tests import census_ref as R
from tests import cheader as H
from tests import groups_ref as G

SEED = 20261020
ALL = 0xf
E_ARG, E_NOINIT, E_LIMITS = (int(H.defines()[k]) for k in ("MADSIM_E_ARG", "MADSIM_E_NOINIT", "MADSIM_E_LIMITS"))


# ---- the directed inputs of the GPU file --------------------------------------------------------------------------------------------------
PINGPONG_SEED0, PINGPONG_TOTAL, PINGPONG_LOSS = 0, 2000, 0.02
LOOP_SEEDS, LOOP_OBS_CAP = 96, 256
RANDOM_SEEDS, RANDOM_MAX_VALUES = 64, 8


def looping_workload():
    """150 iterations that trace the constant 7 and then 100 + the loop counter: 300 observations, the 7 in every round of 64, 150 values
    that occur once each."""
    wl = W.WorkloadBuilder()
    t = wl.task(wl.create_node())
    t.set(0, 150)
    top = t.label()
    t.trace(7).trace(100, add_reg=0).djnz(0, top).done()
    m = wl.main()
    m.spawn(t)
    m.join(t)
    m.done()
    return wl.build()


def random_value_workload():
    """random(); trace_val(): a traced random value is not a probe vocabulary."""
    wl = W.WorkloadBuilder()
    t = wl.task(wl.create_node())
    t.random_u32().trace_val().done()
    m = wl.main()
    m.spawn(t)
    m.join(t)
    m.done()
    return wl.build()


def probe_pingpong_workload(rounds=16):
    """examples/probe_census_test.cpp's body: the lossy two-pair ping-pong whose clients trace 0x10 + pair before their loop and 0x20 + pair
    behind it."""
    wl = W.WorkloadBuilder()
    tasks = []
    for pair in range(2):
        n1, n2 = wl.create_node(), wl.create_node()
        a1, a2 = wl.addr(n1, 1), wl.addr(n2, 1)
        t1 = wl.task(n1)
        t1.bind(a1).sleep(secs=1).trace(0x10 + pair).set(0, rounds)
        top1 = t1.label()
        t1.send_to(a1, a2, 1, W.PING).recv_from(a1, 1).assert_val(W.PONG).djnz(0, top1).trace(0x20 + pair).done()
        t2 = wl.task(n2)
        t2.bind(a2).set(0, rounds)
        top2 = t2.label()
        t2.recv_from(a2, 1).assert_val(W.PING).reply(a2, 1, W.PONG).djnz(0, top2).done()
        tasks += [t1, t2]
    m = wl.main()
    for t in tasks:
        m.spawn(t)
    for t in tasks:
        m.join(t)
    m.done()
    return wl.build()


@functools.lru_cache(maxsize=None)
def truth(name):
    """(workload, config, seeds, [observation list] per seed, [verdict] per seed) of a directed input, by the oracle; computed once and
    shared, read-only, by the tests of both files."""
    w, cfg, seeds = {"pingpong": (G.traced_pingpong_workload(), A.Config.default(packet_loss_rate=PINGPONG_LOSS), range(PINGPONG_SEED0, PINGPONG_SEED0 + PINGPONG_TOTAL)),
                     "loop": (looping_workload(), A.Config.default(), range(LOOP_SEEDS)),
                     "random": (random_value_workload(), A.Config.default(), range(RANDOM_SEEDS))}[name]
    got = [oracle.observe_seed(w, s, cfg) for s in seeds]
    return w, cfg, list(seeds), tuple(tuple(o) for o, _ in got), tuple(r.verdict for _, r in got)


def ref_of(name, include=ALL, obs_cap=256, pick=None):
    """The reference census of a directed input (of the seeds at the indices `pick`, when given)."""
    _, _, seeds, obs, verdicts = truth(name)
    idx = range(len(seeds)) if pick is None else pick
    return R.census_of_lists([obs[i] for i in idx], [verdicts[i] for i in idx], [seeds[i] for i in idx], include, obs_cap)


def test_the_pingpong_range_is_not_vacuous():
    want = ref_of("pingpong")
    assert sum(1 for n in want.n_counted if n) >= 2, want.n_counted                # at least two verdicts
    assert [int(v) for v in want.values["value"]] == [0, 1]
    assert tuple(want.values["n_seeds"][0]) != tuple(want.values["n_seeds"][1])     # the two probes split differently over the verdicts
    assert sum(want.n_silent) > 0 and want.n_runner == 0


def test_the_looping_workload_is_not_vacuous():
    _, _, _, obs, verdicts = truth("loop")
    assert all(len(o) == 300 > LOOP_OBS_CAP for o in obs) and set(verdicts) == {A.PASS}
    assert obs[0][0] == obs[0][64] == obs[0][128] == obs[0][192] == 7              # a value repeated across index 64
    want = ref_of("loop", obs_cap=LOOP_OBS_CAP)
    assert want.n_truncated == LOOP_SEEDS and int(want.values[want.values["value"] == 7]["max_per_seed"][0]) == 128
    whole = ref_of("loop", obs_cap=512)
    assert whole.n_truncated == 0 and int(whole.values[whole.values["value"] == 7]["max_per_seed"][0]) == 150 and len(whole.values) == 151


def test_the_random_value_workload_holds_more_values_than_its_cap():
    assert len(ref_of("random").values) > RANDOM_MAX_VALUES


# ---- the reference against the definition ------------------------------------------------------------------------------------------------
def random_lists(rng, n, vocab, max_len):
    obs = [[int(x) for x in rng.choice(vocab, int(rng.integers(0, max_len + 1)))] for _ in range(n)]
    verdicts = [int(v) for v in rng.choice([0, 1, 2, 3, 4, 5, 7, 0xffffffff], n)]
    seeds = [int(s) for s in np.cumsum(rng.integers(1, 50, n))]
    return obs, verdicts, seeds


@pytest.mark.parametrize("include", [ALL, 1, 6, 8, 0xd])
@pytest.mark.parametrize("obs_cap", [1, 3, 8, 100])
def test_reference_equals_the_dict_restatement(include, obs_cap):
    rng = np.random.default_rng([SEED, include, obs_cap])
    vocab = np.array([0, A.U64_MAX, A.FNV_OFFSET, 5, 6, 7, 1 << 63], dtype=np.uint64)
    obs, verdicts, seeds = random_lists(rng, 60, vocab, 12)
    want = R.census_of_lists(obs, verdicts, seeds, include, obs_cap)
    table, n_counted, n_silent, n_truncated, n_observations, runner = R.census_by_dict(obs, verdicts, seeds, include, obs_cap)
    assert [int(v) for v in want.values["value"]] == sorted(table)
    for e in want.values:
        ns, tot, first, mx = table[int(e["value"])]
        assert ([int(x) for x in e["n_seeds"]], int(e["n_total"]), int(e["first_seed"]), int(e["max_per_seed"])) == (ns, tot, first, mx)
    assert (want.n_counted, want.n_silent, want.n_truncated, want.n_observations, want.runner_seeds) == (n_counted, n_silent, n_truncated, n_observations, runner)
    assert want.n_runner == len(runner) and int(want.values["n_total"].sum()) == n_observations


# ---- the host fold ---------------------------------------------------------------------------------------------------------------------------
def words_of(ref):
    w = np.zeros(16, dtype=np.uint64)
    w[0], w[2:6], w[6:10], w[10], w[11], w[12] = len(ref.values), ref.n_counted, ref.n_silent, ref.n_truncated, ref.n_observations, ref.n_runner
    return w


def fold_chunks(obs, verdicts, seeds, include, obs_cap, cuts, cap, rng=None):
    """(rc of the last fold, Census struct, its value array): the chunks between `cuts` folded by madsim_k_fold_census, each chunk's entries
    made by the reference — in shuffled order when `rng` is given, as the device hands them over."""
    L = runtime.lib()
    values = np.zeros(cap, dtype=A.CENSUS_VALUE_DTYPE)
    cen = A.Census(include=include, obs_cap=obs_cap, cap=cap)
    cen.values = values.ctypes.data_as(C.POINTER(A.CensusValue))
    rc = 0
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        part = R.census_of_lists(obs[lo:hi], verdicts[lo:hi], seeds[lo:hi], include, obs_cap)
        e = part.values.copy()
        if rng is not None:
            rng.shuffle(e)
        w = words_of(part)
        rc = L.madsim_k_fold_census(C.byref(cen), w.ctypes.data_as(C.c_void_p), e.ctypes.data_as(C.c_void_p), len(e))
        if rc:
            break
    return rc, cen, values


@pytest.mark.parametrize("chunk", [1, 7, 64, "uneven", "whole"])
def test_any_cut_into_chunks_folds_to_the_whole(chunk):
    rng = np.random.default_rng([SEED, 3])
    n = 300
    vocab = np.concatenate([np.array([0, A.U64_MAX, A.FNV_OFFSET], dtype=np.uint64), rng.integers(0, 1 << 64, 40, dtype=np.uint64)])
    obs, verdicts, seeds = random_lists(rng, n, vocab, 20)
    want = R.census_of_lists(obs, verdicts, seeds, ALL, 16)
    cuts = {"uneven": [0, 1, 2, 50, 51, 200, 299, 300], "whole": [0, n]}.get(chunk) or list(range(0, n, chunk)) + [n]
    rc, cen, values = fold_chunks(obs, verdicts, seeds, ALL, 16, cuts, len(want.values), rng)          # cap exactly met
    assert rc == 0 and cen.n_values == len(want.values)
    assert values[:cen.n_values].tobytes() == want.values.tobytes()
    assert (tuple(cen.n_counted), tuple(cen.n_silent), cen.n_truncated, cen.n_observations, cen.n_runner) == \
        (want.n_counted, want.n_silent, want.n_truncated, want.n_observations, want.n_runner)
    assert want.n_truncated and want.n_runner and sum(want.n_silent)
    rc, cen, values = fold_chunks(obs, verdicts, seeds, ALL, 16, cuts, len(want.values) - 1, rng)      # one over: the fold that would pass cap fails
    assert rc == -1 and cen.n_values <= len(want.values) - 1
    assert list(values["value"][:cen.n_values]) == sorted(values["value"][:cen.n_values])              # ... and leaves the table as it was


def _as_census(ref, include, obs_cap):
    return runtime.Census(ref.values.copy(), ref.n_counted, ref.n_silent, ref.n_truncated, ref.n_observations, ref.n_runner,
                          np.array(ref.runner_seeds, dtype=np.uint64), include, obs_cap)


def test_merge_of_two_disjoint_halves_is_the_whole():
    rng = np.random.default_rng([SEED, 4])
    obs, verdicts, seeds = random_lists(rng, 200, np.arange(30, dtype=np.uint64) * np.uint64(0x0101010101010101), 10)
    whole = _as_census(R.census_of_lists(obs, verdicts, seeds, ALL, 8), ALL, 8)
    even, odd = (_as_census(R.census_of_lists(obs[k::2], verdicts[k::2], seeds[k::2], ALL, 8), ALL, 8) for k in (0, 1))
    assert even.merge(odd).tobytes() == odd.merge(even).tobytes() == whole.tobytes()
    assert whole.n_runner and len(whole.runner_seeds) == whole.n_runner
    with pytest.raises(runtime.MadsimHipError):
        even.merge(_as_census(R.census_of_lists(obs[1::2], verdicts[1::2], seeds[1::2], ALL, 9), ALL, 9))
    # the readers
    v = int(whole.values["value"][3])
    row = whole.row(v)
    assert whole.reached(v) == int(row["n_seeds"].sum()) > 0 and whole.reached(12345) == 0 and whole.row(12345) is None
    assert whole.never([v, 12345, 0, 54321]) == [12345, 54321]
    share, overall = whole.failing_share(v)
    assert share == runtime.Fraction(int(row["n_seeds"][1:].sum()), int(row["n_seeds"].sum()))
    assert overall == runtime.Fraction(sum(whole.n_counted[1:]), sum(whole.n_counted)) and whole.failing_share(12345)[0] is None


# ---- the surface ---------------------------------------------------------------------------------------------------------------------------
NEW = ("madsim_hip_census_range", "madsim_hip_census_seeds", "madsim_hip_ctx_census_range", "madsim_hip_ctx_census_seeds")


def test_the_header_declares_the_four_functions_and_the_mirrors_follow():
    protos = H.functions()
    L = runtime.lib()
    for fn in NEW:
        assert fn in protos, fn
        assert len(getattr(L, fn).argtypes) == len(protos[fn][1]) and protos[fn][0] == "int", fn
    assert not any("census" in fn and fn.endswith("_multi") for fn in protos)
    d = H.defines()
    assert A.CENSUS_MAX_VALUES == int(d["MADSIM_CENSUS_MAX_VALUES"].rstrip("u")) == 1 << 20
    assert A.CENSUS_MAX_OBS_CAP == int(d["MADSIM_CENSUS_MAX_OBS_CAP"].rstrip("u")) >= 256
    assert A.ABI_VERSION == 7                                       # additive: the version stays
    assert C.sizeof(A.CensusValue) == 64 == np.dtype(A.CENSUS_VALUE_DTYPE).itemsize
    params = ("workload", "seed0", "total", "seeds", "include", "obs_cap", "max_values", "chunk", "config", "limits", "resolve")
    for fn, names in ((runtime.census, params), (runtime.Context.census, ("self",) + params)):
        p = inspect.signature(fn).parameters
        assert tuple(p) == names, fn
        assert (p["seed0"].default, p["total"].default, p["seeds"].default, p["obs_cap"].default, p["max_values"].default, p["chunk"].default,
                p["resolve"].default) == (0, 0, None, 256, 4096, 0, True)
        assert p["include"].default == (A.PASS, A.PANIC, A.DEADLOCK, A.TIME_LIMIT)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hpp = open(os.path.join(root, "include", "madsim_hip.hpp")).read()
    rs = open(os.path.join(root, "bindings", "rust", "madsim-hip", "src", "builder.rs")).read()
    assert "Census census(const Workload& wl" in hpp and "pub fn census(" in rs and "pub fn census_seeds(" in rs


def test_argument_errors_need_no_device():
    """The argument checks come before the context is looked at; an empty range reports the empty census without one."""
    L = runtime.lib()
    w, cfg, lim = W.pingpong(2, 2), A.Config.default(), A.Limits()
    values, runner = (A.CensusValue * 8)(), (C.c_uint64 * 4)()

    def cen(**kw):
        c = A.Census(include=ALL, obs_cap=16, cap=8, n_values=99, n_runner=99)
        c.values = values
        for k, v in kw.items():
            setattr(c, k, v)
        return c

    rng_call = lambda c, total=4, chunk=0: L.madsim_hip_ctx_census_range(None, w.ref(), C.byref(cfg), 0, total, chunk, C.byref(lim), C.byref(c))          # noqa: E731
    lst_call = lambda c, s, n, chunk=0: L.madsim_hip_ctx_census_seeds(None, w.ref(), C.byref(cfg), s, n, chunk, C.byref(lim), C.byref(c))                # noqa: E731
    c = cen()
    assert rng_call(c, total=0) == 0 and (c.n_values, c.n_runner, tuple(c.n_counted)) == (0, 0, (0, 0, 0, 0))
    c = cen()
    assert lst_call(c, None, 0) == 0 and c.n_values == 0
    assert rng_call(cen()) == E_NOINIT                                                 # everything in order: only the context is missing
    assert L.madsim_hip_ctx_census_range(None, w.ref(), C.byref(cfg), 0, 4, 0, C.byref(lim), None) == E_ARG
    for bad in (dict(include=0), dict(include=0x10), dict(include=0x1f), dict(cap=0), dict(cap=A.CENSUS_MAX_VALUES + 1), dict(obs_cap=0),
                dict(obs_cap=A.CENSUS_MAX_OBS_CAP + 1), dict(runner_cap=4), dict(values=None)):
        assert rng_call(cen(**bad)) == E_ARG, bad
        assert lst_call(cen(**bad), (C.c_uint64 * 2)(1, 2), 2) == E_ARG, bad
    ok = cen(runner_cap=4)
    ok.runner_seeds = runner
    assert rng_call(ok) == E_NOINIT
    assert lst_call(cen(), None, 2) == E_ARG                                           # a list of two without a list
    assert lst_call(cen(), (C.c_uint64 * 3)(1, 3, 2), 3) == E_ARG                      # unsorted
    assert b"strictly ascending" in L.madsim_hip_last_error()
    assert lst_call(cen(), (C.c_uint64 * 3)(1, 2, 2), 3) == E_ARG                      # a duplicate
    assert lst_call(cen(), (C.c_uint64 * 3)(1, 2, A.U64_MAX), 3) == E_NOINIT
    # a chunk is never larger than MADSIM_TRACE_MAX_BYTES allows, and chunk x obs_cap stays below 2^32 - 1
    assert rng_call(cen(), total=1 << 40, chunk=1 << 30) == E_LIMITS and b"MADSIM_TRACE_MAX_BYTES" in L.madsim_hip_last_error()
    assert rng_call(cen(obs_cap=1), total=1 << 40, chunk=A.TRACE_MAX_BYTES // 80 + 1) == E_LIMITS
    assert rng_call(cen(obs_cap=1), total=1 << 40, chunk=A.TRACE_MAX_BYTES // 80 - 4096) == E_NOINIT
    # the Python wrapper points at numpy.unique before anything is run
    with pytest.raises(runtime.MadsimHipError, match="numpy.unique"):
        runtime.seed_list([3, 1, 2])


def test_the_example_compiles_without_warnings(tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", os.path.join(root, "examples", "probe_census_test.cpp"), "-o",
                           str(tmp_path / "probe_census_test"), "-L" + os.path.join(root, "madsim_amd"), "-lmadsim_hip",
                           "-Wl,-rpath," + os.path.join(root, "madsim_amd")])
