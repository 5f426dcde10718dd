"""The probe-order census — which traced value the seeds of a range reach first, by verdict (madsim_hip_probe_order_range / _seeds,
runtime.probe_order) — on the CPU: the numpy reference (tests/order_ref.py) against a plain-Python restatement, one seed at a time with
list.index; the host fold (madsim_k_fold_probe_order) over every cut of an array into chunks; the readers of runtime.ProbeOrder against
brute force over per-seed first-occurrence maps; the surface and its argument errors, which need no device; and the directed inputs that
tests/test_probe_order_gpu.py runs on the device, with the proof — by the oracle alone — that they are not vacuous."""
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
from tests import order_ref as R
from tests import test_census as TC

SEED = 20261022
ALL = 0xf
E_ARG, E_NOINIT, E_LIMITS = (int(H.defines()[k]) for k in ("MADSIM_E_ARG", "MADSIM_E_NOINIT", "MADSIM_E_LIMITS"))

# ---- the directed inputs of the GPU file --------------------------------------------------------------------------------------------------
PROBE_SEED0, PROBE_TOTAL, PROBE_LOSS = 0, 2000, 0.02
PROBE_VOCAB, LOOP_VOCAB = (0x10, 0x11, 0x20, 0x21, 0x30), (7, 100, 249)


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
    return R.probe_order_of_lists([obs[i] for i in idx], [verdicts[i] for i in idx], [seeds[i] for i in idx], include, obs_cap, vocab)


def brute(name, vocab, obs_cap=256):
    """[(seed, verdict, {index: first})] of a directed input, one seed at a time with list.index."""
    _, _, seeds, obs, verdicts = truth(name)
    return [(s, v, R.seed_firsts(o, obs_cap, vocab)) for s, v, o in zip(seeds, verdicts, obs)]


def cells(ref, vocab, what="n_seeds"):
    return {(vocab[int(e["a"])], vocab[int(e["b"])]): [int(x) for x in e[what]] for e in ref.pairs}


def test_the_probe_pingpong_gives_exactly_the_cells_of_the_issue():
    want = ref_of("probe", PROBE_VOCAB)
    n, first = cells(want, PROBE_VOCAB), cells(want, PROBE_VOCAB, "first_seed")
    # Twelve cells: four on the diagonal, both orders inside each pair of equals, and the four "a start before an end".  Their non-zero
    # per-verdict counts number 22 — the figure the feature's specification gives as the number of entries: it counts (cell, verdict)
    # pairs; with 72-byte entries of four verdicts each and no cell below the diagonal blocks, twelve is all there can be.
    assert len(want.pairs) == 12 and sum(1 for e in want.pairs for x in e["n_seeds"] if int(x)) == 22
    assert n[(0x10, 0x11)] == [266, 0, 723, 0] and first[(0x10, 0x11)] == [16, 0, 0, 0]
    assert n[(0x11, 0x10)] == [305, 0, 706, 0]
    assert n[(0x20, 0x21)] == [286, 0, 0, 0]
    assert n[(0x21, 0x20)] == [285, 0, 0, 0] and first[(0x21, 0x20)] == [19, 0, 0, 0]
    assert n[(0x10, 0x20)] == [571, 0, 496, 0]
    assert n[(0x20, 0x20)] == [571, 0, 496, 0] and n[(0x21, 0x21)] == [571, 0, 506, 0]
    assert not any(a in (0x20, 0x21) and b in (0x10, 0x11) for a, b in n)             # a loop never ends before both have started
    assert not any(0x30 in c for c in n)                                              # 0x30 never fires
    assert want.n_counted == (571, 0, 1429, 0) and want.n_none == (0, 0, 0, 0) and want.n_truncated == 0 and want.n_runner == 0
    # every entry once more, one seed at a time with list.index
    per_seed = brute("probe", PROBE_VOCAB)
    for e in want.pairs:
        a, b = int(e["a"]), int(e["b"])
        for k in range(4):
            having = [s for s, v, f in per_seed if v == k and a in f and b in f and (a == b or f[a] < f[b])]
            assert int(e["n_seeds"][k]) == len(having) and int(e["first_seed"][k]) == (min(having) if having else 0), (a, b, k)
    # what the set words hide: the sets are symmetric in the pairs, the order is not
    assert n[(0x10, 0x11)] != n[(0x11, 0x10)] and n[(0x10, 0x11)][0] + n[(0x11, 0x10)][0] == 571


def test_the_looping_workload_differs_at_256_and_512_only_in_n_truncated():
    _, _, seeds, obs, _ = truth("loop")
    assert all(len(o) == 300 and o[0] == 7 and o[1] == 250 and o[3] == 249 for o in obs)      # 7 at index 0; 249 is the second counter value, at index 3
    cut, whole = ref_of("loop", LOOP_VOCAB, obs_cap=256), ref_of("loop", LOOP_VOCAB, obs_cap=512)
    assert cut.pairs.tobytes() == whole.pairs.tobytes() and (cut.n_counted, cut.n_none) == (whole.n_counted, whole.n_none)
    assert (cut.n_truncated, whole.n_truncated) == (len(seeds), 0)
    # 100 + counter runs from 250 down and ends at 101: 100 is never traced; 7 at index 0 comes before 249 at index 3
    assert cells(cut, LOOP_VOCAB) == {(7, 7): [len(seeds), 0, 0, 0], (7, 249): [len(seeds), 0, 0, 0], (249, 249): [len(seeds), 0, 0, 0]}
    assert cells(cut, LOOP_VOCAB, "first_seed")[(7, 249)] == [min(seeds), 0, 0, 0]


# ---- the reference against the definition ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("include", [ALL, 1, 6, 8, 0xd])
@pytest.mark.parametrize("obs_cap", [1, 3, 8, 100])
def test_reference_equals_the_plain_python_restatement(include, obs_cap):
    rng = np.random.default_rng([SEED, include, obs_cap])
    universe = np.array([0, A.U64_MAX, A.FNV_OFFSET, 5, 6, 7, 1 << 63], dtype=np.uint64)
    vocab = [int(v) for v in universe[:5]]                                          # 6, 7 and 2^63 are foreign
    obs, verdicts, seeds = TC.random_lists(rng, 80, universe, 12)
    want = R.probe_order_of_lists(obs, verdicts, seeds, include, obs_cap, vocab)
    table, n_counted, n_none, n_truncated, runner = R.probe_order_by_dict(obs, verdicts, seeds, include, obs_cap, vocab)
    assert [(int(e["a"]), int(e["b"])) for e in want.pairs] == sorted(table), (SEED, include, obs_cap)
    for e in want.pairs:
        assert ([int(x) for x in e["n_seeds"]], [int(x) for x in e["first_seed"]]) == tuple(table[(int(e["a"]), int(e["b"]))]), (SEED, int(e["a"]), int(e["b"]))
    assert (want.n_counted, want.n_none, want.n_truncated, want.runner_seeds, want.n_runner) == (n_counted, n_none, n_truncated, runner, len(runner))


# ---- the host fold ---------------------------------------------------------------------------------------------------------------------------
def fold_chunks(obs, verdicts, seeds, include, obs_cap, vocab, cuts, cap, rng=None):
    """(rc of the last fold, ProbeOrder struct, its pair array): the chunks between `cuts` folded by madsim_k_fold_probe_order, each chunk's
    entries made by the reference — in shuffled order when `rng` is given."""
    L = runtime.lib()
    pairs = np.zeros(cap, dtype=A.PROBE_ORDER_PAIR_DTYPE)
    po = A.ProbeOrder(include=include, obs_cap=obs_cap, cap=cap)
    po.pairs = pairs.ctypes.data_as(C.POINTER(A.ProbeOrderPair))
    rc = 0
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        part = R.probe_order_of_lists(obs[lo:hi], verdicts[lo:hi], seeds[lo:hi], include, obs_cap, vocab)
        e = part.pairs.copy()
        if rng is not None:
            rng.shuffle(e)
        w = part.words()
        rc = L.madsim_k_fold_probe_order(C.byref(po), w.ctypes.data_as(C.c_void_p), e.ctypes.data_as(C.c_void_p), len(e))
        if rc:
            break
    return rc, po, pairs


def fold_input(tag):
    rng = np.random.default_rng([SEED, tag])
    universe = np.concatenate([np.array([0, A.U64_MAX, A.FNV_OFFSET], dtype=np.uint64), rng.integers(0, 1 << 64, 9, dtype=np.uint64)])
    obs, verdicts, seeds = TC.random_lists(rng, 300, universe, 6)
    return rng, [int(v) for v in universe[:8]], obs, verdicts, seeds


@pytest.mark.parametrize("chunk", [1, 7, 64, "uneven", "whole"])
def test_any_cut_into_chunks_folds_to_the_whole(chunk):
    rng, vocab, obs, verdicts, seeds = fold_input(3)
    n = len(seeds)
    want = R.probe_order_of_lists(obs, verdicts, seeds, ALL, 4, vocab)
    assert len(want.pairs) > 40 and want.n_runner and want.n_truncated and sum(want.n_none)
    cuts = {"uneven": [0, 1, 2, 50, 51, 200, 299, 300], "whole": [0, n]}.get(chunk) or list(range(0, n, chunk)) + [n]
    rc, po, pairs = fold_chunks(obs, verdicts, seeds, ALL, 4, vocab, cuts, len(want.pairs), rng)            # cap exactly met
    assert rc == 0 and po.n_pairs == len(want.pairs), (SEED, chunk)
    assert pairs[:po.n_pairs].tobytes() == want.pairs.tobytes(), (SEED, chunk)
    assert (tuple(po.n_counted), tuple(po.n_none), po.n_truncated, po.n_runner) == (want.n_counted, want.n_none, want.n_truncated, want.n_runner)
    rc, po, pairs = fold_chunks(obs, verdicts, seeds, ALL, 4, vocab, cuts, len(want.pairs) - 1, rng)        # one short: the fold that would pass cap fails
    assert rc == -1 and po.n_pairs <= len(want.pairs) - 1
    keys = [(int(e["a"]), int(e["b"])) for e in pairs[:po.n_pairs]]
    assert keys == sorted(keys)                                                        # ... and leaves the table as it was


def test_the_fold_orders_by_a_then_b_and_keeps_first_seed_zero_where_nothing_is():
    e = np.zeros(4, dtype=A.PROBE_ORDER_PAIR_DTYPE)
    e["a"], e["b"] = [1, 0, 1, 0], [0, 31, 0, 2]
    e["n_seeds"][0], e["first_seed"][0] = [2, 0, 0, 0], [40, 0, 0, 0]
    e["n_seeds"][1], e["first_seed"][1] = [0, 1, 0, 0], [0, 7, 0, 0]
    e["n_seeds"][2], e["first_seed"][2] = [1, 0, 3, 0], [11, 0, 0, 0]                  # (a deadlocking seed 0 is a seed like any other)
    e["n_seeds"][3], e["first_seed"][3] = [0, 0, 0, 5], [0, 0, 0, 9]
    pairs = np.zeros(3, dtype=A.PROBE_ORDER_PAIR_DTYPE)
    po = A.ProbeOrder(include=ALL, obs_cap=4, cap=3)
    po.pairs = pairs.ctypes.data_as(C.POINTER(A.ProbeOrderPair))
    assert runtime.lib().madsim_k_fold_probe_order(C.byref(po), None, e.ctypes.data_as(C.c_void_p), 4) == 0 and po.n_pairs == 3
    assert [(int(x["a"]), int(x["b"])) for x in pairs] == [(0, 2), (0, 31), (1, 0)]
    assert [int(x) for x in pairs["n_seeds"][2]] == [3, 0, 3, 0] and [int(x) for x in pairs["first_seed"][2]] == [11, 0, 0, 0]
    assert tuple(po.n_counted) == (0, 0, 0, 0)                                         # (no words: no totals)


# ---- runtime.ProbeOrder --------------------------------------------------------------------------------------------------------------------
def as_report(ref, vocab, include=ALL, obs_cap=4):
    return runtime.ProbeOrder(vocab, ref.pairs.copy(), ref.n_counted, ref.n_none, ref.n_truncated, ref.n_runner,
                              np.array(ref.runner_seeds, dtype=np.uint64), include, obs_cap)


def test_the_readers_against_brute_force_over_per_seed_first_occurrences():
    _, vocab, obs, verdicts, seeds = fold_input(4)
    rep = as_report(R.probe_order_of_lists(obs, verdicts, seeds, ALL, 4, vocab), vocab)
    per_seed = [(s, v, {vocab[j]: i for j, i in R.seed_firsts(o, 4, vocab).items()}) for o, v, s in zip(obs, verdicts, seeds) if v < 4]
    for vs in (None, (A.PASS,), (A.PANIC, A.DEADLOCK), A.TIME_LIMIT):
        ks = (0, 1, 2, 3) if vs is None else (vs,) if isinstance(vs, int) else vs
        mine = [(s, v, f) for s, v, f in per_seed if v in ks]
        for a in vocab:
            assert rep.reached(a, vs) == sum(1 for _, _, f in mine if a in f), (SEED, a, vs)
            for b in vocab:
                both = [(s, f) for s, _, f in mine if a in f and b in f]
                ab = [s for s, f in both if f[a] < f[b]]
                assert rep.before(a, b, vs) == (len(both) if a == b else len(ab)), (SEED, a, b, vs)
                assert rep.both(a, b, vs) == len(both) and rep.without(a, b, vs) == sum(1 for _, _, f in mine if a in f and b not in f)
                assert rep.always_before(a, b, vs) == (a != b and bool(both) and len(ab) == len(both))
        always = {(a, b) for a in vocab for b in vocab if rep.always_before(a, b, vs)}
        prec = rep.precedence(vs)
        assert set(prec) <= always and prec == sorted(prec, key=lambda p: (vocab.index(p[0]), vocab.index(p[1])))

        def reach(a, b, edges):                                                        # a chain of pairs from a to b
            todo, seen = [a], set()
            while todo:
                x = todo.pop()
                for p, q in edges:
                    if p == x and q not in seen:
                        seen.add(q)
                        todo.append(q)
            return b in seen

        for a, b in always:                                                            # dropped exactly when another chain leads there
            assert ((a, b) in prec) == (not reach(a, b, always - {(a, b)})), (SEED, a, b, vs)
    for k in range(4):
        for a in vocab:
            for b in vocab:
                having = [s for s, v, f in per_seed if v == k and a in f and b in f and (a == b or f[a] < f[b])]
                assert rep.witness(a, b, k) == (min(having) if having else None)
    want = []
    for a in vocab:
        for b in vocab:
            passing = [f for _, v, f in per_seed if v == 0 and a in f and b in f]
            failing = [s for s, v, f in per_seed if v and a in f and b in f and f[b] < f[a]]
            if a != b and passing and all(f[a] < f[b] for f in passing) and failing:
                want.append((a, b, min(failing)))
    assert rep.discriminating() == want and want, SEED
    assert all(isinstance(x, int) for x in (rep.reached(vocab[0]), rep.before(vocab[0], vocab[1]), rep.both(vocab[0], vocab[1]), rep.without(vocab[0], vocab[1])))
    with pytest.raises(runtime.MadsimHipError, match="not in the vocabulary"):
        rep.before(vocab[0], 12345)


def test_precedence_drops_what_a_chain_implies_and_discriminating_names_the_failing_witness():
    """A hand-made input: 1 before 2 before 3 in every seed; passing seeds trace 4 before 5, one failing seed 5 before 4."""
    vocab = [1, 2, 3, 4, 5]
    obs = [[1, 2, 3, 4, 5], [9, 1, 1, 2, 4, 3, 5], [1, 2, 3, 5, 4], [1, 2, 3, 4, 5]]
    rep = as_report(R.probe_order_of_lists(obs, [0, 0, 2, 2], [10, 11, 12, 13], ALL, 16, vocab), vocab, obs_cap=16)
    assert rep.precedence(A.PASS) == [(1, 2), (2, 3), (2, 4), (3, 5), (4, 5)]          # (3 and 4 come both ways; 1 -> 3, 1 -> 4, 2 -> 5, .. are implied)
    assert rep.discriminating() == [(4, 5, 12)]
    assert rep.always_before(1, 3) and not rep.always_before(4, 5) and rep.always_before(4, 5, A.PASS) and rep.witness(5, 4, A.DEADLOCK) == 12


def test_merge_of_two_disjoint_halves_is_the_whole():
    _, vocab, obs, verdicts, seeds = fold_input(6)
    whole = as_report(R.probe_order_of_lists(obs, verdicts, seeds, ALL, 4, vocab), vocab)
    even, odd = (as_report(R.probe_order_of_lists(obs[k::2], verdicts[k::2], seeds[k::2], ALL, 4, vocab), vocab) for k in (0, 1))
    assert even.merge(odd).tobytes() == odd.merge(even).tobytes() == whole.tobytes()
    assert whole.n_runner and len(whole.runner_seeds) == whole.n_runner
    for other in (as_report(R.probe_order_of_lists(obs[1::2], verdicts[1::2], seeds[1::2], ALL, 5, vocab), vocab, obs_cap=5),
                  as_report(R.probe_order_of_lists(obs[1::2], verdicts[1::2], seeds[1::2], ALL, 4, vocab[::-1]), vocab[::-1]),
                  as_report(R.probe_order_of_lists(obs[1::2], verdicts[1::2], seeds[1::2], 1, 4, vocab), vocab, include=1)):
        with pytest.raises(runtime.MadsimHipError):
            even.merge(other)


# ---- the surface ---------------------------------------------------------------------------------------------------------------------------
NEW = ("madsim_hip_probe_order_range", "madsim_hip_probe_order_seeds", "madsim_hip_ctx_probe_order_range", "madsim_hip_ctx_probe_order_seeds")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL_VERDICTS = (A.PASS, A.PANIC, A.DEADLOCK, A.TIME_LIMIT)


def test_the_header_declares_the_four_functions_and_the_mirrors_follow():
    protos = H.functions()
    L = runtime.lib()
    for fn in NEW:
        assert fn in protos, fn
        assert len(getattr(L, fn).argtypes) == len(protos[fn][1]) and protos[fn][0] == "int", fn
    assert not any("probe_order" in fn and fn.endswith("_multi") for fn in protos)
    for fn in ("madsim_k_fold_probe_order", "madsim_k_launch_probe_order", "madsim_k_launch_probe_order_form"):
        assert hasattr(L, fn), fn
    d = H.defines()
    assert A.PROBE_ORDER_MAX_VOCAB == int(d["MADSIM_PROBE_ORDER_MAX_VOCAB"].rstrip("u")) == 32
    assert A.ABI_VERSION == 7                                       # additive: the version stays
    fields = H.structs()["madsim_probe_order_pair_t"]
    assert [(f[0], f[2]) for f in fields] == [("a", 0), ("b", 0), ("n_seeds", 4), ("first_seed", 4)]
    assert C.sizeof(A.ProbeOrderPair) == 72 == np.dtype(A.PROBE_ORDER_PAIR_DTYPE).itemsize and C.sizeof(A.ProbeOrder) == 152
    assert [f[0] for f in H.structs()["madsim_probe_order_t"]] == [f[0] for f in A.ProbeOrder._fields_]
    params = ("workload", "vocabulary", "seed0", "total", "seeds", "include", "obs_cap", "chunk", "config", "limits", "resolve")
    for fn, names in ((runtime.probe_order, params), (runtime.Context.probe_order, ("self",) + params)):
        p = inspect.signature(fn).parameters
        assert tuple(p) == names, fn
        assert (p["vocabulary"].default, p["seed0"].default, p["total"].default, p["seeds"].default, p["obs_cap"].default, p["chunk"].default,
                p["resolve"].default) == (None, 0, 0, None, 256, 0, True)
        assert p["include"].default == ALL_VERDICTS
    hpp = open(os.path.join(ROOT, "include", "madsim_hip.hpp")).read()
    rs = open(os.path.join(ROOT, "bindings", "rust", "madsim-hip", "src", "builder.rs")).read()
    assert "ProbeOrder probe_order(const Workload& wl" in hpp and "pub fn probe_order(" in rs and "pub fn probe_order_seeds(" in rs
    sys_rs = open(os.path.join(ROOT, "bindings", "rust", "madsim-hip-sys", "src", "lib.rs")).read()
    gen = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_rust_sys.py")], capture_output=True, text=True, check=True)
    assert gen.stdout == sys_rs                                     # the committed binding is what the generator produces
    assert "pub struct madsim_probe_order_pair_t" in sys_rs and "pub fn madsim_hip_ctx_probe_order_seeds(" in sys_rs


def test_argument_errors_need_no_device():
    """The argument checks come before the context is looked at; an empty range reports the empty result without one."""
    L = runtime.lib()
    w, cfg, lim = W.pingpong(2, 2), A.Config.default(), A.Limits()
    pairs, runner, vocab = (A.ProbeOrderPair * 1024)(), (C.c_uint64 * 4)(), (C.c_uint64 * 33)(*range(100, 133))

    def rep(**kw):
        p = A.ProbeOrder(include=ALL, obs_cap=16, n_vocab=3, cap=9, n_pairs=99, n_truncated=99, n_runner=99, n_runner_listed=99)
        p.n_counted[2] = p.n_none[1] = 99
        p.pairs, p.vocab = pairs, vocab
        for k, v in kw.items():
            setattr(p, k, v)
        return p

    rng_call = lambda p, total=4, chunk=0: L.madsim_hip_ctx_probe_order_range(None, w.ref(), C.byref(cfg), 0, total, chunk, C.byref(lim), C.byref(p))          # noqa: E731
    lst_call = lambda p, s, n, chunk=0: L.madsim_hip_ctx_probe_order_seeds(None, w.ref(), C.byref(cfg), s, n, chunk, C.byref(lim), C.byref(p))                # noqa: E731
    p = rep()
    assert rng_call(p, total=0) == 0
    assert (p.n_pairs, p.n_truncated, p.n_runner, p.n_runner_listed, tuple(p.n_counted), tuple(p.n_none)) == (0, 0, 0, 0, (0, 0, 0, 0), (0, 0, 0, 0))
    p = rep()
    assert lst_call(p, None, 0) == 0 and p.n_pairs == 0
    assert rng_call(rep()) == E_NOINIT                                                 # everything in order: only the context is missing
    assert rng_call(rep(n_vocab=32, cap=1024)) == E_NOINIT and rng_call(rep(n_vocab=1, cap=1)) == E_NOINIT and rng_call(rep(cap=1 << 40)) == E_NOINIT
    assert L.madsim_hip_ctx_probe_order_range(None, w.ref(), C.byref(cfg), 0, 4, 0, C.byref(lim), None) == E_ARG
    for bad in (dict(include=0), dict(include=0x10), dict(include=0x1f), dict(cap=0), dict(cap=8), dict(n_vocab=32, cap=1023), dict(obs_cap=0),
                dict(obs_cap=A.CENSUS_MAX_OBS_CAP + 1), dict(runner_cap=4), dict(pairs=None), dict(n_vocab=0), dict(n_vocab=33, cap=33 * 33), dict(vocab=None)):
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
    # a chunk is never larger than MADSIM_TRACE_MAX_BYTES allows (chunk x (8 obs_cap + 72) + 32768 + 76 n_vocab^2 + 96), and chunk x obs_cap stays below 2^32 - 1
    assert rng_call(rep(), total=1 << 40, chunk=1 << 30) == E_LIMITS and b"MADSIM_TRACE_MAX_BYTES" in L.madsim_hip_last_error()
    fixed = 32768 + 76 * 9 + 96
    assert rng_call(rep(obs_cap=1), total=1 << 40, chunk=(A.TRACE_MAX_BYTES - fixed) // 80 + 1) == E_LIMITS
    assert rng_call(rep(obs_cap=1), total=1 << 40, chunk=(A.TRACE_MAX_BYTES - fixed) // 80) == E_NOINIT
    assert rng_call(rep(obs_cap=1, cap=1 << 40), total=1 << 40, chunk=(A.TRACE_MAX_BYTES - fixed) // 80) == E_NOINIT      # the caller's cap asks nothing of the device
    # the Python wrapper's own checks come before anything is run
    for vocab_bad in ([], list(range(33)), [1, 2, 1]):
        with pytest.raises(runtime.MadsimHipError, match="vocabulary"):
            runtime._probe_order(None, None, None, w, vocab_bad, 0, 4, None, ALL_VERDICTS, 16, 0, None, None, None)


def test_the_example_compiles_without_warnings(tmp_path):
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", os.path.join(ROOT, "examples", "probe_order_test.cpp"), "-o",
                           str(tmp_path / "probe_order_test"), "-L" + os.path.join(ROOT, "madsim_amd"), "-lmadsim_hip",
                           "-Wl,-rpath," + os.path.join(ROOT, "madsim_amd")])
