"""The probe-set census — which combinations of traced values the seeds of a range reach, by verdict (madsim_hip_probe_sets_range / _seeds,
runtime.probe_sets) — on the CPU: the numpy reference (tests/sets_ref.py) against a dict-and-set restatement; the host fold
(madsim_k_fold_probe_sets) over every cut of an array into chunks, at `cap` and one over it; the readers of runtime.ProbeSets against
brute force over per-seed sets; the surface and its argument errors, which need no device; and the directed inputs that
tests/test_probe_sets_gpu.py runs on the device, with the proof — by the oracle alone — that they are not vacuous."""
import ctypes as C
import functools
import inspect
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle
from madsim_amd import _abi as A
from madsim_amd import runtime
from madsim_amd import workload as W
from tests import cheader as H
from tests import sets_ref as R
from tests import test_census as TC

SEED = 20261021
ALL = 0xf
E_ARG, E_NOINIT, E_LIMITS = (int(H.defines()[k]) for k in ("MADSIM_E_ARG", "MADSIM_E_NOINIT", "MADSIM_E_LIMITS"))
OTHER, TRUNCATED = A.PROBE_SET_OTHER, A.PROBE_SET_TRUNCATED

# ---- the directed inputs of the GPU file --------------------------------------------------------------------------------------------------
PROBE_SEED0, PROBE_TOTAL, PROBE_LOSS = 0, 2000, 0.02
PROBE_VOCAB, PAIR0_VOCAB, LOOP_VOCAB = (0x10, 0x11, 0x20, 0x21, 0x30), (0x10, 0x20), (7, 100, 249)


@functools.lru_cache(maxsize=None)
def truth(name):
    """(workload, config, seeds, [observation list] per seed, [verdict] per seed) of a directed input, by the oracle; computed once and
    shared, read-only, by the tests of both files."""
    if name == "loop":
        return TC.truth("loop")
    w, cfg, seeds = TC.probe_pingpong_workload(), A.Config.default(packet_loss_rate=PROBE_LOSS), range(PROBE_SEED0, PROBE_SEED0 + PROBE_TOTAL)
    got = [oracle.observe_seed(w, s, cfg) for s in seeds]
    return w, cfg, list(seeds), tuple(tuple(o) for o, _ in got), tuple(r.verdict for _, r in got)


def ref_of(name, vocab, include=ALL, obs_cap=256, pick=None):
    """The reference report of a directed input (of the seeds at the indices `pick`, when given)."""
    _, _, seeds, obs, verdicts = truth(name)
    idx = range(len(seeds)) if pick is None else pick
    return R.probe_sets_of_lists([obs[i] for i in idx], [verdicts[i] for i in idx], [seeds[i] for i in idx], include, obs_cap, vocab)


def brute(name, vocab, obs_cap=256):
    """[(seed, verdict, set word)] of a directed input, one seed at a time with Python sets."""
    _, _, seeds, obs, verdicts = truth(name)
    return [(s, v, R.seed_set_word(o, obs_cap, vocab)) for s, v, o in zip(seeds, verdicts, obs)]


def test_the_probe_pingpong_gives_exactly_the_four_sets_of_the_issue():
    want = ref_of("probe", PROBE_VOCAB)
    P, D = A.PASS, A.DEADLOCK
    table = {int(e["set"]): [int(x) for x in e["n_seeds"]] for e in want.sets}
    assert table == {0b01111: [571, 0, 0, 0], 0b00011: [0, 0, 427, 0], 0b00111: [0, 0, 496, 0], 0b01011: [0, 0, 506, 0]}, table
    assert want.n_counted == (571, 0, 1429, 0) and want.n_runner == 0
    assert not any(int(e["set"]) & (1 << 4 | OTHER | TRUNCATED) for e in want.sets)        # 0x30 never fires, nothing foreign, nothing cut
    per_seed = brute("probe", PROBE_VOCAB)
    for e in want.sets:
        for k in range(4):
            having = [s for s, v, word in per_seed if v == k and word == int(e["set"])]
            assert int(e["n_seeds"][k]) == len(having) and int(e["first_seed"][k]) == (min(having) if having else 0), (int(e["set"]), k)
    assert [int(e["n_seeds"][P]) > 0 for e in want.sets] == [False, False, False, True] and D == 2
    # what the marginals hide: a seed passes exactly when 0x20 and 0x21 are both reached
    assert all((v == P) == (word & 0b1100 == 0b1100) for _, v, word in per_seed)


def test_two_values_leave_a_mixed_set_and_set_other():
    want = ref_of("probe", PAIR0_VOCAB)
    assert [(int(e["set"]), [int(x) for x in e["n_seeds"]]) for e in want.sets] == [(OTHER | 0b01, [0, 0, 933, 0]), (OTHER | 0b11, [571, 0, 496, 0])]
    per_seed = brute("probe", PAIR0_VOCAB)
    for e in want.sets:
        for k in (A.PASS, A.DEADLOCK):
            having = [s for s, v, word in per_seed if v == k and word == int(e["set"])]
            assert int(e["first_seed"][k]) == (min(having) if having else 0)


def test_the_looping_workload_is_truncated_at_256_and_whole_at_512():
    _, _, seeds, obs, _ = truth("loop")
    assert all(len(o) == 300 for o in obs)
    cut, whole = ref_of("loop", LOOP_VOCAB, obs_cap=256), ref_of("loop", LOOP_VOCAB, obs_cap=512)
    assert all(word & TRUNCATED for _, _, word in brute("loop", LOOP_VOCAB, 256)) and not any(word & TRUNCATED for _, _, word in brute("loop", LOOP_VOCAB, 512))
    # 100 + counter runs from 250 down: 249 is the second value traced, 100 never is (the counter ends at 101)
    assert [(int(e["set"]), int(e["n_seeds"][0])) for e in cut.sets] == [(TRUNCATED | OTHER | 0b101, len(seeds))]
    assert [(int(e["set"]), int(e["n_seeds"][0])) for e in whole.sets] == [(OTHER | 0b101, len(seeds))]


# ---- the reference against the definition ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("include", [ALL, 1, 6, 8, 0xd])
@pytest.mark.parametrize("obs_cap", [1, 3, 8, 100])
def test_reference_equals_the_dict_restatement(include, obs_cap):
    rng = np.random.default_rng([SEED, include, obs_cap])
    universe = np.array([0, A.U64_MAX, A.FNV_OFFSET, 5, 6, 7, 1 << 63], dtype=np.uint64)
    vocab = [int(v) for v in universe[:5]]                                          # 6, 7 and 2^63 are foreign
    obs, verdicts, seeds = TC.random_lists(rng, 80, universe, 12)
    want = R.probe_sets_of_lists(obs, verdicts, seeds, include, obs_cap, vocab)
    table, n_counted, runner = R.probe_sets_by_dict(obs, verdicts, seeds, include, obs_cap, vocab)
    assert [int(s) for s in want.sets["set"]] == sorted(table), (SEED, include, obs_cap)
    for e in want.sets:
        assert ([int(x) for x in e["n_seeds"]], [int(x) for x in e["first_seed"]]) == tuple(table[int(e["set"])]), (SEED, int(e["set"]))
    assert (want.n_counted, want.runner_seeds, want.n_runner) == (n_counted, runner, len(runner))
    assert tuple(int(x) for x in want.sets["n_seeds"].sum(axis=0)) == want.n_counted


# ---- the host fold ---------------------------------------------------------------------------------------------------------------------------
def words_of(ref):
    w = np.zeros(8, dtype=np.uint64)
    w[0], w[2:6], w[6] = len(ref.sets), ref.n_counted, ref.n_runner
    return w


def fold_chunks(obs, verdicts, seeds, include, obs_cap, vocab, cuts, cap, rng=None):
    """(rc of the last fold, ProbeSets struct, its set array): the chunks between `cuts` folded by madsim_k_fold_probe_sets, each chunk's
    entries made by the reference — in shuffled order when `rng` is given, as the device hands them over."""
    L = runtime.lib()
    sets = np.zeros(cap, dtype=A.PROBE_SET_DTYPE)
    ps = A.ProbeSets(include=include, obs_cap=obs_cap, cap=cap)
    ps.sets = sets.ctypes.data_as(C.POINTER(A.ProbeSet))
    rc = 0
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        part = R.probe_sets_of_lists(obs[lo:hi], verdicts[lo:hi], seeds[lo:hi], include, obs_cap, vocab)
        e = part.sets.copy()
        if rng is not None:
            rng.shuffle(e)
        w = words_of(part)
        rc = L.madsim_k_fold_probe_sets(C.byref(ps), w.ctypes.data_as(C.c_void_p), e.ctypes.data_as(C.c_void_p), len(e))
        if rc:
            break
    return rc, ps, sets


def fold_input(tag):
    rng = np.random.default_rng([SEED, tag])
    universe = np.concatenate([np.array([0, A.U64_MAX, A.FNV_OFFSET], dtype=np.uint64), rng.integers(0, 1 << 64, 9, dtype=np.uint64)])
    obs, verdicts, seeds = TC.random_lists(rng, 300, universe, 6)
    return rng, [int(v) for v in universe[:8]], obs, verdicts, seeds


@pytest.mark.parametrize("chunk", [1, 7, 64, "uneven", "whole"])
def test_any_cut_into_chunks_folds_to_the_whole(chunk):
    rng, vocab, obs, verdicts, seeds = fold_input(3)
    n = len(seeds)
    want = R.probe_sets_of_lists(obs, verdicts, seeds, ALL, 4, vocab)
    assert len(want.sets) > 20 and want.n_runner and any(int(s) & TRUNCATED for s in want.sets["set"]) and any(int(s) & OTHER for s in want.sets["set"])
    assert any(int(s) == 0 for s in want.sets["set"])                                  # the empty set is an entry like any other
    cuts = {"uneven": [0, 1, 2, 50, 51, 200, 299, 300], "whole": [0, n]}.get(chunk) or list(range(0, n, chunk)) + [n]
    rc, ps, sets = fold_chunks(obs, verdicts, seeds, ALL, 4, vocab, cuts, len(want.sets), rng)            # cap exactly met
    assert rc == 0 and ps.n_sets == len(want.sets), (SEED, chunk)
    assert sets[:ps.n_sets].tobytes() == want.sets.tobytes(), (SEED, chunk)
    assert (tuple(ps.n_counted), ps.n_runner) == (want.n_counted, want.n_runner)
    rc, ps, sets = fold_chunks(obs, verdicts, seeds, ALL, 4, vocab, cuts, len(want.sets) - 1, rng)        # one over: the fold that would pass cap fails
    assert rc == -1 and ps.n_sets <= len(want.sets) - 1
    assert list(sets["set"][:ps.n_sets]) == sorted(sets["set"][:ps.n_sets])                              # ... and leaves the table as it was


def test_the_fold_combines_equal_sets_inside_one_chunk_and_keeps_first_seed_zero_where_nothing_is():
    e = np.zeros(3, dtype=A.PROBE_SET_DTYPE)
    e["set"] = [5, 9, 5]
    e["n_seeds"][0], e["first_seed"][0] = [2, 0, 0, 0], [40, 0, 0, 0]
    e["n_seeds"][1], e["first_seed"][1] = [0, 1, 0, 0], [0, 7, 0, 0]
    e["n_seeds"][2], e["first_seed"][2] = [1, 0, 3, 0], [11, 0, 0, 0]                  # (a deadlocking seed 0 is a seed like any other)
    sets = np.zeros(2, dtype=A.PROBE_SET_DTYPE)
    ps = A.ProbeSets(include=ALL, obs_cap=4, cap=2)
    ps.sets = sets.ctypes.data_as(C.POINTER(A.ProbeSet))
    assert runtime.lib().madsim_k_fold_probe_sets(C.byref(ps), None, e.ctypes.data_as(C.c_void_p), 3) == 0 and ps.n_sets == 2
    assert [int(x) for x in sets["set"]] == [5, 9]
    assert [int(x) for x in sets["n_seeds"][0]] == [3, 0, 3, 0] and [int(x) for x in sets["first_seed"][0]] == [11, 0, 0, 0]
    assert tuple(ps.n_counted) == (0, 0, 0, 0)                                         # (no words: no totals)


# ---- runtime.ProbeSets ---------------------------------------------------------------------------------------------------------------------
def as_report(ref, vocab, include=ALL, obs_cap=4):
    return runtime.ProbeSets(vocab, ref.sets.copy(), ref.n_counted, ref.n_runner, np.array(ref.runner_seeds, dtype=np.uint64), include, obs_cap)


def test_the_readers_against_brute_force_over_per_seed_sets():
    _, vocab, obs, verdicts, seeds = fold_input(4)
    rep = as_report(R.probe_sets_of_lists(obs, verdicts, seeds, ALL, 4, vocab), vocab)
    per_seed = [(s, v, R.seed_set_word(o, 4, vocab)) for o, v, s in zip(obs, verdicts, seeds) if v < 4]
    has = lambda word, vals: all(word >> vocab.index(x) & 1 for x in vals)             # noqa: E731
    hasnt = lambda word, vals: not any(word >> vocab.index(x) & 1 for x in vals)       # noqa: E731
    for all_of, none_of in (((), ()), (vocab[:1], ()), (vocab[1:3], vocab[:1]), ((), vocab[2:5]), (vocab[:2], vocab[5:6]), (vocab, ())):
        for vs in (None, (A.PASS,), (A.PANIC, A.DEADLOCK), A.TIME_LIMIT):
            ks = (0, 1, 2, 3) if vs is None else (vs,) if isinstance(vs, int) else vs
            hit = [(s, v) for s, v, word in per_seed if v in ks and has(word, all_of) and hasnt(word, none_of)]
            assert rep.count(all_of, none_of, verdicts=vs) == len(hit), (SEED, all_of, none_of, vs)
            assert rep.first_seeds(all_of, none_of, vs) == {k: min(s for s, v in hit if v == k) for k in ks if any(v == k for _, v in hit)}
        n = sum(1 for s, v, word in per_seed if has(word, all_of) and hasnt(word, none_of))
        f = sum(1 for s, v, word in per_seed if v and has(word, all_of) and hasnt(word, none_of))
        share, overall = rep.failing_share(all_of, none_of)
        assert share == (runtime.Fraction(f, n) if n else None) and overall == runtime.Fraction(sum(1 for _, v, _ in per_seed if v), len(per_seed))
    for flag, bit in (("other", OTHER), ("truncated", TRUNCATED)):
        for want_bit in (True, False):
            assert rep.count(**{flag: want_bit}) == sum(1 for _, _, word in per_seed if bool(word & bit) == want_bit) > 0
    assert rep.count() == len(per_seed) == sum(rep.n_counted)
    for vs in (None, (A.PASS,), (A.DEADLOCK, A.TIME_LIMIT)):
        ks = (0, 1, 2, 3) if vs is None else vs
        want = [[sum(1 for _, v, word in per_seed if v in ks and word >> i & 1 and word >> j & 1) for j in range(len(vocab))] for i in range(len(vocab))]
        assert rep.cooccurrence(vs) == want, (SEED, vs)
    mixed = rep.mixed()
    words = sorted({word for _, v, word in per_seed if v == 0} & {word for _, v, word in per_seed if v})
    assert [m[0] for m in mixed] == words and words
    for word, p, f in mixed:
        assert p == min(s for s, v, x in per_seed if x == word and v == 0) and f == min(s for s, v, x in per_seed if x == word and v)
    assert all(isinstance(x, int) for row in rep.cooccurrence() for x in row) and isinstance(rep.count(), int)
    assert rep.values_of(0b101 | OTHER) == (vocab[0], vocab[2]) and rep.mask(vocab[1:3]) == 0b110
    with pytest.raises(runtime.MadsimHipError, match="not in the vocabulary"):
        rep.count(all_of=(12345,))


@pytest.mark.parametrize("vs", [None, (A.PASS,), (A.PANIC, A.DEADLOCK, A.TIME_LIMIT)])
def test_cover_reaches_every_reached_value_and_is_the_same_on_every_call(vs):
    _, vocab, obs, verdicts, seeds = fold_input(5)
    rep = as_report(R.probe_sets_of_lists(obs, verdicts, seeds, ALL, 4, vocab), vocab)
    ks = (0, 1, 2, 3) if vs is None else vs
    word_of = {s: R.seed_set_word(o, 4, vocab) for o, v, s in zip(obs, verdicts, seeds) if v in ks}
    reached = functools.reduce(int.__or__, word_of.values()) & ((1 << len(vocab)) - 1)
    cover = rep.cover(vs)
    assert cover == sorted(set(cover)) == rep.cover(vs) and all(isinstance(s, int) for s in cover), (SEED, vs)
    assert functools.reduce(int.__or__, (word_of[s] for s in cover)) & ((1 << len(vocab)) - 1) == reached and reached
    assert len(cover) <= bin(reached).count("1")                                       # every chosen entry adds a value
    # the directed input: the passing set alone covers all that is reached
    probe = as_report(ref_of("probe", PROBE_VOCAB), PROBE_VOCAB, obs_cap=256)
    assert probe.cover() == [int(probe.sets[-1]["first_seed"][A.PASS])] and probe.cover(A.DEADLOCK) == sorted(
        int(e["first_seed"][A.DEADLOCK]) for e in probe.sets[1:3])


def test_merge_of_two_disjoint_halves_is_the_whole():
    _, vocab, obs, verdicts, seeds = fold_input(6)
    whole = as_report(R.probe_sets_of_lists(obs, verdicts, seeds, ALL, 4, vocab), vocab)
    even, odd = (as_report(R.probe_sets_of_lists(obs[k::2], verdicts[k::2], seeds[k::2], ALL, 4, vocab), vocab) for k in (0, 1))
    assert even.merge(odd).tobytes() == odd.merge(even).tobytes() == whole.tobytes()
    assert whole.n_runner and len(whole.runner_seeds) == whole.n_runner
    for other in (as_report(R.probe_sets_of_lists(obs[1::2], verdicts[1::2], seeds[1::2], ALL, 5, vocab), vocab, obs_cap=5),
                  as_report(R.probe_sets_of_lists(obs[1::2], verdicts[1::2], seeds[1::2], ALL, 4, vocab[::-1]), vocab[::-1]),
                  as_report(R.probe_sets_of_lists(obs[1::2], verdicts[1::2], seeds[1::2], 1, 4, vocab), vocab, include=1)):
        with pytest.raises(runtime.MadsimHipError):
            even.merge(other)


# ---- the surface ---------------------------------------------------------------------------------------------------------------------------
NEW = ("madsim_hip_probe_sets_range", "madsim_hip_probe_sets_seeds", "madsim_hip_ctx_probe_sets_range", "madsim_hip_ctx_probe_sets_seeds")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_header_declares_the_four_functions_and_the_mirrors_follow():
    protos = H.functions()
    L = runtime.lib()
    for fn in NEW:
        assert fn in protos, fn
        assert len(getattr(L, fn).argtypes) == len(protos[fn][1]) and protos[fn][0] == "int", fn
    assert not any("probe_sets" in fn and fn.endswith("_multi") for fn in protos)
    for fn in ("madsim_k_fold_probe_sets", "madsim_k_launch_probe_sets", "madsim_k_probe_sets_slots"):
        assert hasattr(L, fn), fn
    raw = open(H.HEADER_PATH).read()
    d = H.defines()
    assert A.PROBE_SETS_MAX_VOCAB == int(d["MADSIM_PROBE_SETS_MAX_VOCAB"].rstrip("u")) == 62
    assert A.PROBE_SETS_MAX == int(d["MADSIM_PROBE_SETS_MAX"].rstrip("u")) == 1 << 20
    assert "#define MADSIM_PROBE_SET_OTHER      0x4000000000000000ull" in raw and "#define MADSIM_PROBE_SET_TRUNCATED  0x8000000000000000ull" in raw
    assert (A.PROBE_SET_OTHER, A.PROBE_SET_TRUNCATED) == (1 << 62, 1 << 63)
    assert A.ABI_VERSION == 7                                       # additive: the version stays
    fields, size = H.structs()["madsim_probe_set_t"], 72
    assert [(f[0], f[2]) for f in fields] == [("set", 0), ("n_seeds", 4), ("first_seed", 4)]
    assert C.sizeof(A.ProbeSet) == size == np.dtype(A.PROBE_SET_DTYPE).itemsize and C.sizeof(A.ProbeSets) == 112
    assert [f[0] for f in H.structs()["madsim_probe_sets_t"]] == [f[0] for f in A.ProbeSets._fields_]
    params = ("workload", "vocabulary", "seed0", "total", "seeds", "include", "obs_cap", "max_sets", "chunk", "config", "limits", "resolve")
    for fn, names in ((runtime.probe_sets, params), (runtime.Context.probe_sets, ("self",) + params)):
        p = inspect.signature(fn).parameters
        assert tuple(p) == names, fn
        assert (p["vocabulary"].default, p["seed0"].default, p["total"].default, p["seeds"].default, p["obs_cap"].default, p["max_sets"].default,
                p["chunk"].default, p["resolve"].default) == (None, 0, 0, None, 256, 4096, 0, True)
        assert p["include"].default == (A.PASS, A.PANIC, A.DEADLOCK, A.TIME_LIMIT)
    hpp = open(os.path.join(ROOT, "include", "madsim_hip.hpp")).read()
    rs = open(os.path.join(ROOT, "bindings", "rust", "madsim-hip", "src", "builder.rs")).read()
    assert "ProbeSets probe_sets(const Workload& wl" in hpp and "pub fn probe_sets(" in rs and "pub fn probe_sets_seeds(" in rs
    sys_rs = open(os.path.join(ROOT, "bindings", "rust", "madsim-hip-sys", "src", "lib.rs")).read()
    gen = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_rust_sys.py")], capture_output=True, text=True, check=True)
    assert gen.stdout == sys_rs                                     # the committed binding is what the generator produces
    assert "pub const MADSIM_PROBE_SET_TRUNCATED: u64 = 0x8000000000000000;" in sys_rs


def test_argument_errors_need_no_device():
    """The argument checks come before the context is looked at; an empty range reports the empty result without one."""
    L = runtime.lib()
    w, cfg, lim = W.pingpong(2, 2), A.Config.default(), A.Limits()
    sets, runner, vocab = (A.ProbeSet * 8)(), (C.c_uint64 * 4)(), (C.c_uint64 * 62)(*range(100, 162))

    def rep(**kw):
        p = A.ProbeSets(include=ALL, obs_cap=16, n_vocab=3, cap=8, n_sets=99, n_runner=99, n_runner_listed=99)
        p.n_counted[2] = 99
        p.sets, p.vocab = sets, vocab
        for k, v in kw.items():
            setattr(p, k, v)
        return p

    rng_call = lambda p, total=4, chunk=0: L.madsim_hip_ctx_probe_sets_range(None, w.ref(), C.byref(cfg), 0, total, chunk, C.byref(lim), C.byref(p))          # noqa: E731
    lst_call = lambda p, s, n, chunk=0: L.madsim_hip_ctx_probe_sets_seeds(None, w.ref(), C.byref(cfg), s, n, chunk, C.byref(lim), C.byref(p))                # noqa: E731
    p = rep()
    assert rng_call(p, total=0) == 0 and (p.n_sets, p.n_runner, p.n_runner_listed, tuple(p.n_counted)) == (0, 0, 0, (0, 0, 0, 0))
    p = rep()
    assert lst_call(p, None, 0) == 0 and p.n_sets == 0
    assert rng_call(rep()) == E_NOINIT                                                 # everything in order: only the context is missing
    assert rng_call(rep(n_vocab=62)) == E_NOINIT and rng_call(rep(n_vocab=1)) == E_NOINIT
    assert L.madsim_hip_ctx_probe_sets_range(None, w.ref(), C.byref(cfg), 0, 4, 0, C.byref(lim), None) == E_ARG
    for bad in (dict(include=0), dict(include=0x10), dict(include=0x1f), dict(cap=0), dict(cap=A.PROBE_SETS_MAX + 1), dict(obs_cap=0),
                dict(obs_cap=A.CENSUS_MAX_OBS_CAP + 1), dict(runner_cap=4), dict(sets=None), dict(n_vocab=0), dict(n_vocab=63), dict(vocab=None)):
        assert rng_call(rep(**bad)) == E_ARG, bad
        assert lst_call(rep(**bad), (C.c_uint64 * 2)(1, 2), 2) == E_ARG, bad
    for dup in ((C.c_uint64 * 3)(5, 6, 5), (C.c_uint64 * 3)(0, 0, 1), (C.c_uint64 * 3)(1, A.U64_MAX, A.U64_MAX)):
        assert rng_call(rep(vocab=dup)) == E_ARG and b"twice" in L.madsim_hip_last_error(), list(dup)
    assert rng_call(rep(vocab=(C.c_uint64 * 3)(0, A.U64_MAX, A.FNV_OFFSET))) == E_NOINIT                  # every value is legal
    ok = rep(runner_cap=4)
    ok.runner_seeds = runner
    assert rng_call(ok) == E_NOINIT
    assert lst_call(rep(), None, 2) == E_ARG                                           # a list of two without a list
    assert lst_call(rep(), (C.c_uint64 * 3)(1, 3, 2), 3) == E_ARG                      # unsorted
    assert b"strictly ascending (sort and deduplicate it first)" in L.madsim_hip_last_error()
    assert lst_call(rep(), (C.c_uint64 * 3)(1, 2, 2), 3) == E_ARG                      # a duplicate
    assert lst_call(rep(), (C.c_uint64 * 3)(1, 2, A.U64_MAX), 3) == E_NOINIT
    # a chunk is never larger than MADSIM_TRACE_MAX_BYTES allows (chunk x (8 obs_cap + 80) + 48 slots + 76 cap + 64), and chunk x obs_cap stays below 2^32 - 1
    assert rng_call(rep(), total=1 << 40, chunk=1 << 30) == E_LIMITS and b"MADSIM_TRACE_MAX_BYTES" in L.madsim_hip_last_error()
    fixed = 48 * 128 + 76 * 8 + 64
    assert rng_call(rep(obs_cap=1), total=1 << 40, chunk=(A.TRACE_MAX_BYTES - fixed) // 88 + 1) == E_LIMITS
    assert rng_call(rep(obs_cap=1), total=1 << 40, chunk=(A.TRACE_MAX_BYTES - fixed) // 88) == E_NOINIT
    # the Python wrapper's own checks come before anything is run
    for vocab_bad in ([], list(range(63)), [1, 2, 1]):
        with pytest.raises(runtime.MadsimHipError, match="vocabulary"):
            runtime._probe_sets(None, None, None, w, vocab_bad, 0, 4, None, ALL_VERDICTS, 16, 8, 0, None, None, None)


ALL_VERDICTS = (A.PASS, A.PANIC, A.DEADLOCK, A.TIME_LIMIT)


def test_the_example_compiles_without_warnings(tmp_path):
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", os.path.join(ROOT, "examples", "probe_sets_test.cpp"), "-o",
                           str(tmp_path / "probe_sets_test"), "-L" + os.path.join(ROOT, "madsim_amd"), "-lmadsim_hip",
                           "-Wl,-rpath," + os.path.join(ROOT, "madsim_amd")])
