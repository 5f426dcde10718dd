"""The campaign report kernels (summary, summary6, collect count + write, statistics fold + top) and the host fold on SYNTHETIC result
arrays: values, verdicts, orders, counts and seeds the simulator never produces — bit 63 set, every histogram bucket's two edges, verdicts
of 7 and more, the 256-workgroup grid cap, ties at rank K across a round, a piece and a workgroup, a `cap` that ends inside a wave's round.

Three layers, each exact (no tolerance anywhere):
  1. without a GPU: tests/report_ref.py's and tests/stats_ref.py's numpy truths against a restatement in plain Python ints on every
     synthetic family at every count up to 4 097, and the device-word layout;
  2. without a GPU: madsim_k_fold_stats (the host fold, csrc/madsim_hip.cpp) over stats_words(...) of synthetic truths against
     stats_ref.fold;
  3. on the MI355X: the kernels, launched directly (tests/report_kernels.py), against the truths of layer 1.
Every array comes from numpy.random.default_rng([SEED, count, case number]); SEED is in every assertion message."""
import collections
import functools
import struct

import numpy as np
import pytest

from madsim_amd import _abi as A
from tests import report_kernels as K
from tests import report_ref as T
from tests import stats_ref as R

SEED = 20261017
U64, U32 = (1 << 64) - 1, (1 << 32) - 1
COUNTS = (1, 63, 64, 65, 1023, 1024, 1025, 4097, 262_144, 262_209)
SMALL = tuple(c for c in COUNTS if c <= 4097)
PASS = R.mask(A.PASS)
PANIC_TL = R.mask(A.PANIC, A.TIME_LIMIT)
ALL = R.mask(A.PASS, A.PANIC, A.DEADLOCK, A.TIME_LIMIT)
TOP_KS = (0, 1, 2, 15, 16)
METRICS64 = ("clock_ns", "msg_count", "rng_calls")

Case = collections.namedtuple("Case", "name results seed0 k")       # k: the K a pattern was laid out for (None: any)


def seed0s(count):
    return (0, (1 << 40) + 7, (1 << 64) - count)                    # the last: the batch ends with seed 2^64 - 1


# ---- values ------------------------------------------------------------------------------------------------------------------
def v_zero(rng, n, bits):
    return np.zeros(n, dtype=np.uint64)


def v_ones(rng, n, bits):
    return np.full(n, (1 << bits) - 1, dtype=np.uint64)


def v_edges(rng, n, bits):
    """bucket_floor(b) and bucket_floor(b) - 1 for every b in 1 .. 251 (those that fit `bits`), in a random order, repeated to n."""
    edges = [x for b in range(1, 252) for x in (R.bucket_floor(b), R.bucket_floor(b) - 1) if x < 1 << bits]
    return np.resize(rng.permutation(np.array(edges, dtype=np.uint64)), n)


def v_uniform(rng, n, bits):
    return rng.integers(0, 1 << bits, n, dtype=np.uint64)


def v_bitlen(rng, n, bits):
    """Bit lengths 1 .. bits, each as likely as the other."""
    x = rng.integers(0, 1 << 64, n, dtype=np.uint64) | np.uint64(1 << 63)
    return x >> (64 - rng.integers(1, bits + 1, n)).astype(np.uint64)


def v_one_max(rng, n, bits):
    v = rng.integers(0, 1000, n, dtype=np.uint64)
    v[rng.integers(n)] = (1 << bits) - 1
    return v


VALUES = (v_zero, v_ones, v_edges, v_uniform, v_bitlen, v_one_max)


def blank(rng, n, verdict):
    r = np.zeros(n, dtype=A.RESULT_DTYPE)
    r["verdict"] = verdict
    r["trace_hash"], r["obs_hash"] = rng.integers(0, 1 << 64, n, dtype=np.uint64), rng.integers(0, 1 << 64, n, dtype=np.uint64)
    return r


def with_values(rng, n, verdict, rot):
    """Rotation `rot`: clock_ns, msg_count, rng_calls and (at 32 bits) steps each from another family — six rotations give every metric
    every family."""
    r = blank(rng, n, verdict)
    for j, name in enumerate(METRICS64):
        r[name] = VALUES[(rot + j) % 6](rng, n, 64)
    r["steps"] = VALUES[(rot + 3) % 6](rng, n, 32)
    return r


def below_the_extremes(rng, n, verdict):
    """Random values under 2^62 (steps: 2^30): whatever a pattern puts above them are the extremes."""
    r = blank(rng, n, verdict)
    for name in METRICS64:
        r[name] = rng.integers(0, 1 << 62, n, dtype=np.uint64)
    r["steps"] = rng.integers(0, 1 << 30, n)
    return r


# ---- verdicts ----------------------------------------------------------------------------------------------------------------
def uniform_verdicts(rng, n):
    return rng.integers(0, 8, n).astype(np.uint32)


def counted_mix(rng, n):
    """PASS, PANIC, DEADLOCK, TIME_LIMIT and OVERFLOW: the counted subset of an order pattern depends on `include`."""
    return rng.integers(0, 5, n).astype(np.uint32)


def owned(count):
    """(grid, piece, last wave that owns a result)"""
    grid, piece = T.cut(count)
    return grid, piece, (count - 1) // piece


def edge_positions(count):
    """The first and the last index, the last lane of a full round, the first lane of the last (partial) round, both sides of a piece
    boundary and of a workgroup boundary — those that exist at this count."""
    grid, piece, last_wave = owned(count)
    lo = last_wave * piece
    pos = {0, count - 1, piece - 1, piece, 4 * piece - 1, 4 * piece}
    if count - lo >= 64:
        pos.add(lo + (count - lo) // 64 * 64 - 1)
    if (count - lo) % 64:
        pos.add(lo + (count - lo) // 64 * 64)
    if count >= 64:
        pos.add(63)
    return sorted(p for p in pos if 0 <= p < count)


# ---- orders for the top K ----------------------------------------------------------------------------------------------------
def ascending(rng, n):
    """Strictly ascending with the index: every round of every wave brings the list new entries."""
    r = blank(rng, n, counted_mix(rng, n))
    i = np.arange(n, dtype=np.uint64)
    r["clock_ns"], r["msg_count"], r["rng_calls"], r["steps"] = np.uint64(1 << 63) + i, i * np.uint64(3), np.uint64(U64 - (n - 1)) + i, i + np.uint64(1)
    return r


def descending(rng, n):
    r = blank(rng, n, counted_mix(rng, n))
    i = np.arange(n, dtype=np.uint64)
    r["clock_ns"], r["msg_count"], r["rng_calls"], r["steps"] = np.uint64(U64) - i, (np.uint64(n) - i) << np.uint64(20), np.uint64(1 << 63) - i, np.uint64(n) - i
    return r


def constant(rng, n):
    """A total tie: the K smallest counted seeds win."""
    r = blank(rng, n, counted_mix(rng, n))
    r["clock_ns"], r["msg_count"], r["rng_calls"], r["steps"] = U64, 0, 12345, U32
    return r


def ties(rng, n, k, placement):
    """2K seeds tied at the maximum around a boundary — clock_ns: a 64-lane round inside a wave, msg_count and steps: a piece inside a
    workgroup, rng_calls: a workgroup.  placement 0: the K winners lie on both sides; 1: the K winners end at the boundary's last lane
    and the K losers begin behind it."""
    grid, piece, last_wave = owned(n)
    r = below_the_extremes(rng, n, counted_mix(rng, n))
    w = min(3, last_wave)
    bounds = {"clock_ns": w * piece + 64, "msg_count": (last_wave // 4 * 4 + 1) * piece, "steps": piece, "rng_calls": max(last_wave // 4, 1) * 4 * piece}
    for name, b in bounds.items():
        if not 0 < b < n:
            b = n // 2                                               # (no such boundary at this count: any place)
        first = b - ((k + 1) // 2 if placement == 0 else k)
        at = np.arange(max(first, 0), min(first + 2 * k, n))
        r[name][at] = U32 if name == "steps" else U64
        r["verdict"][at] = A.PASS
    return r


def few_counted(rng, n, k):
    """Exactly k counted seeds (PASS; the rest DEADLOCK or OVERFLOW), anywhere in the batch."""
    r = with_values(rng, n, rng.choice(np.array([A.DEADLOCK, A.OVERFLOW], dtype=np.uint32), n), 3)
    r["verdict"][rng.choice(n, min(max(k, 0), n), replace=False)] = A.PASS
    return r


def _extremes(rng, r, at):
    for name in METRICS64:
        r[name][at] = np.uint64(1 << 63) + rng.permutation(len(at)).astype(np.uint64)
    r["steps"][at] = (1 << 31) + rng.permutation(len(at))
    r["verdict"][at] = A.PASS


def one_per_workgroup(rng, n):
    """The 16 largest values, one per workgroup in 16 workgroups (as many as own a result)."""
    grid, piece, last_wave = owned(n)
    r = below_the_extremes(rng, n, counted_mix(rng, n))
    wgs = rng.choice(last_wave // 4 + 1, min(16, last_wave // 4 + 1), replace=False)
    _extremes(rng, r, np.array([rng.integers(g * 4 * piece, min((g + 1) * 4 * piece, n)) for g in wgs]))
    return r


def one_round(rng, n):
    """The 16 largest values in one 64-lane round of one wave."""
    grid, piece, last_wave = owned(n)
    r = below_the_extremes(rng, n, counted_mix(rng, n))
    lo = int(rng.integers(0, last_wave + 1)) * piece
    lo += int(rng.integers(0, (min(lo + piece, n) - lo + 63) // 64)) * 64
    lanes = min(64, n - lo)
    _extremes(rng, r, lo + rng.choice(lanes, min(16, lanes), replace=False))
    return r


def last_wave_only(rng, n):
    """Counted (and passing) seeds only in the last wave that owns anything."""
    grid, piece, last_wave = owned(n)
    v = rng.choice(np.array([A.OVERFLOW, A.STEP_LIMIT, A.INTERNAL], dtype=np.uint32), n)
    v[last_wave * piece:] = rng.integers(0, 4, n - last_wave * piece)
    return with_values(rng, n, v, 4)


# ---- the cases of a count ----------------------------------------------------------------------------------------------------
def case_makers(count):
    """[(name, maker(rng), K or None)] — the same list, in the same order, for the truth tests and the GPU tests."""
    out = [(f"values{rot}", lambda g, rot=rot: with_values(g, count, uniform_verdicts(g, count), rot), None) for rot in range(6)]
    out.append(("all-pass", lambda g: with_values(g, count, A.PASS, 3), None))
    out += [(f"all-{A.VERDICT_NAMES[v]}", lambda g, v=v: with_values(g, count, v, 2 + v), None) for v in range(1, 8)]
    out.append(("verdicts-8-and-more", lambda g: with_values(g, count, g.choice(np.array([0, 2, 6, 7, 8, 255, 1 << 31, U32], dtype=np.uint32), count), 4), None))
    out.append(("last-wave-only", lambda g: last_wave_only(g, count), None))

    def single(g, p, v):
        r = with_values(g, count, A.PASS, 3)
        r["verdict"][p] = v
        return r
    kinds = (A.PANIC, A.DEADLOCK, A.TIME_LIMIT, A.OVERFLOW, A.STEP_LIMIT, A.INTERNAL)
    out += [(f"single-{A.VERDICT_NAMES[kinds[j % 6]]}@{p}", lambda g, p=p, v=kinds[j % 6]: single(g, p, v), None) for j, p in enumerate(edge_positions(count))]
    out += [("ascending", lambda g: ascending(g, count), None), ("descending", lambda g: descending(g, count), None),
            ("constant", lambda g: constant(g, count), None), ("one-per-workgroup", lambda g: one_per_workgroup(g, count), None),
            ("one-round", lambda g: one_round(g, count), None)]
    for k in TOP_KS[1:]:
        out += [(f"ties-k{k}-straddling", lambda g, k=k: ties(g, count, k, 0), k), (f"ties-k{k}-ending", lambda g, k=k: ties(g, count, k, 1), k)]
        out += [(f"counted-{k + d}-k{k}", lambda g, k=k, d=d: few_counted(g, count, k + d), k) for d in (-1, 0, 1)]
    return out


def case_names(count):
    return [name for name, _, _ in case_makers(count)]


def make_case(count, number):
    name, maker, k = case_makers(count)[number]
    results = maker(np.random.default_rng([SEED, count, number]))
    assert results.dtype == np.dtype(A.RESULT_DTYPE) and len(results) == count
    results.setflags(write=False)
    return Case(f"seed {SEED} count {count} case {number} {name}", results, seed0s(count)[number % 3], k)


def cases(count):
    return (make_case(count, j) for j in range(len(case_makers(count))))


def stats_settings(case):
    """[(include, K)] a case's statistics are checked at."""
    if case.k is not None:
        return [(PASS, case.k), (ALL, case.k)]
    if " single-" in case.name:                                      # (all but one seed pass: the verdict's place is collect's business)
        return [(ALL, 16), (PASS, 2)]
    return [(ALL, k) for k in TOP_KS] + [(PASS, 16), (PANIC_TL, 16), (PANIC_TL, 2)]


def caps(results, list_runner):
    """0, 1, L - 1, L, L + 1 and count, L the number of listed seeds."""
    n_listed = int(T.listed_mask(results, list_runner).sum())
    return sorted({c for c in (0, 1, n_listed - 1, n_listed, n_listed + 1, len(results)) if 0 <= c <= len(results)})


def truth(results, seed0, include, top_k):
    return R.stats_truth(results, np.uint64(seed0), include, top_k)


# ---- layer 1: the truths against plain Python ints (no GPU) --------------------------------------------------------------------
def py_bucket(v):
    if v < 4:
        return v
    e = v.bit_length() - 1
    return 4 * (e - 1) + ((v >> (e - 2)) & 3)


def py_summary(rows, seed0):
    first = gfirst = U64
    nfail = nrun = steps = clk = 0
    for i, r in enumerate(rows):
        if r[0] != A.PASS:
            nfail += 1
            first = min(first, seed0 + i)
            if r[0] >= A.OVERFLOW:
                nrun += 1
            else:
                gfirst = min(gfirst, seed0 + i)
        steps, clk = (steps + r[1]) % (1 << 64), (clk + r[2]) % (1 << 64)
    return [first, nfail, steps, clk], [first, nfail, steps, clk, gfirst, nrun]


def py_collect(rows, seed0, cap, list_runner):
    by, recs, n_listed = [0] * 8, [], 0
    for i, r in enumerate(rows):
        by[min(r[0], 7)] += 1
        if r[0] != A.PASS and (list_runner or r[0] < A.OVERFLOW):
            n_listed += 1
            if len(recs) < cap:
                recs.append(struct.pack("<QIIQQQQQ", seed0 + i, *r))
    return py_summary(rows, seed0)[1] + by + [n_listed], b"".join(recs)


def py_wave_counts(rows, list_runner):
    grid, piece = T.cut(len(rows))
    out = [0] * (4 * grid)
    for i, r in enumerate(rows):
        if r[0] != A.PASS and (list_runner or r[0] < A.OVERFLOW):
            out[i // piece] += 1
    return out


def py_stats_words(rows, seed0, include, top_k):
    """The 657 words, every one a Python int."""
    counted = [(seed0 + i, (r[2], r[1], r[3], r[4])) for i, r in enumerate(rows) if r[0] < 4 and include >> r[0] & 1]
    w = [0] * T.STATS_WORDS
    w[0] = len(counted)
    for m in range(4):
        vals = [v[m] for _, v in counted]
        w[1 + m], w[5 + m] = U64 ^ min(vals + [U64]), max(vals + [0])
        w[9 + m], w[13 + m] = sum(v & U32 for v in vals), sum(v >> 32 for v in vals)
        assert w[9 + m] + (w[13 + m] << 32) == sum(vals)                                     # (the 128-bit sum, as the host fold rebuilds it)
        hist = collections.Counter(map(py_bucket, vals))
        for j in range(128):
            w[T.HIST_OFF + 128 * m + j] = hist.get(2 * j, 0) | hist.get(2 * j + 1, 0) << 32
        for r, (seed, v) in enumerate(sorted(counted, key=lambda e: (-e[1][m], e[0]))[:top_k]):
            w[T.TOP_OFF + 2 * (16 * m + r)], w[T.TOP_OFF + 2 * (16 * m + r) + 1] = v[m], seed
    return w


def test_the_driver_restates_the_headers_sizes():
    assert K.header_constants() == {"COLLECT_WORDS": K.COLLECT_WORDS, "COLLECT_WAVES": K.COLLECT_WAVES, "STATS_WORDS": K.STATS_WORDS,
                                    "STATS_CAND_WORDS": K.STATS_CAND_WORDS}
    assert (T.COLLECT_WORDS, T.STATS_WORDS, T.TOP_OFF) == (K.COLLECT_WORDS, K.STATS_WORDS, K.TOP_OFF)


def test_the_cut_of_a_batch():
    """What the issue's counts exercise, as the launchers cut them."""
    assert [T.cut(c) for c in COUNTS] == [(1, 64), (1, 64), (1, 64), (1, 64), (1, 256), (1, 256), (2, 192), (5, 256), (256, 256), (256, 320)]
    assert owned(1025)[2] == 5 and owned(4097)[2] == 16 and owned(262_209) == (256, 320, 819) and 262_209 - 819 * 320 == 129
    for c in list(COUNTS) + [100_000, 62_209, 262_145]:
        grid, piece = T.cut(c)
        assert 4 * grid * piece >= c and piece % 64 == 0 and grid <= 256 and 4 * grid <= K.COLLECT_WAVES


def test_the_families_hold_what_they_promise():
    rng = np.random.default_rng([SEED, 0])
    edges = set(v_edges(rng, 502, 64).tolist())
    assert edges == {x for b in range(1, 252) for x in (R.bucket_floor(b), R.bucket_floor(b) - 1)} and U64 not in edges and (1 << 63) in edges
    assert {py_bucket(x) for x in edges} == set(range(252))
    assert max(v_edges(rng, 4097, 32).tolist()) == U32 and {py_bucket(x) for x in v_edges(rng, 4097, 32).tolist()} == set(range(124))
    assert {int(x).bit_length() for x in v_bitlen(rng, 4097, 64)} == set(range(1, 65)) and {int(x).bit_length() for x in v_bitlen(rng, 4097, 32)} == set(range(1, 33))
    assert int(v_uniform(rng, 4097, 64).max()) >> 63 == 1 and int(v_uniform(rng, 4097, 32).max()) <= U32
    assert sorted(v_one_max(rng, 65, 64).tolist())[-2:][0] < 1000 and int(v_one_max(rng, 65, 64).max()) == U64
    assert edge_positions(1025) == [0, 63, 191, 192, 767, 768, 1023, 1024] and edge_positions(1) == [0]
    assert edge_positions(262_209) == [0, 63, 319, 320, 1279, 1280, 262_207, 262_208]
    r = ties(rng, 262_209, 16, 1)
    for name, b in (("clock_ns", 3 * 320 + 64), ("msg_count", 817 * 320), ("rng_calls", 204 * 1280)):
        assert np.nonzero(r[name] == U64)[0].tolist() == list(range(b - 16, b + 16)), name
    assert np.nonzero(ties(rng, 262_209, 15, 0)["steps"] == U32)[0].tolist() == list(range(320 - 8, 320 + 22))
    assert int((few_counted(rng, 262_209, 15)["verdict"] == A.PASS).sum()) == 15
    r = one_per_workgroup(rng, 262_209)
    assert len({int(p) // 1280 for p in np.nonzero(r["clock_ns"] >= 1 << 63)[0]}) == 16
    r = one_round(rng, 262_209)
    at = np.nonzero(r["rng_calls"] >= 1 << 63)[0]
    assert len(at) == 16 and (at[0] % 320) // 64 == (at[-1] % 320) // 64 and at[0] // 320 == at[-1] // 320
    r = last_wave_only(rng, 262_209)
    assert (r["verdict"][:819 * 320] >= 4).all() and (r["verdict"][819 * 320:] < 4).all()
    assert len(case_names(4097)) == len(set(case_names(4097)))


@pytest.mark.parametrize("count", SMALL)
def test_the_truths_are_plain_pythons(count):
    """summary_truth, collect_truth, wave_counts, stats_truth (its lexsort over ~v, buckets(), the half-sums) and stats_words against
    Python ints, on every case the GPU tests use at this count."""
    for case in cases(count):
        rows, seed0 = case.results.tolist(), case.seed0
        assert T.summary_truth(case.results, seed0) == py_summary(rows, seed0), case.name
        for list_runner in (0, 1):
            assert T.wave_counts(case.results, list_runner).tolist() == py_wave_counts(rows, list_runner), (case.name, list_runner)
            for cap in caps(case.results, list_runner):
                words, recs = T.collect_truth(case.results, seed0, cap, list_runner)
                assert ([int(x) for x in words], recs) == py_collect(rows, seed0, cap, list_runner), (case.name, list_runner, cap)
        full = {}
        for include, top_k in stats_settings(case):
            t = truth(case.results, seed0, include, top_k)
            if include not in full:
                full[include] = py_stats_words(rows, seed0, include, 16)
            want = [0 if j >= T.TOP_OFF and (j - T.TOP_OFF) // 2 % 16 >= top_k else x for j, x in enumerate(full[include])]
            assert [int(x) for x in T.stats_words(t)] == want, (case.name, include, top_k)
            assert (t["n"], t["n_top"]) == (want[0], min(top_k, want[0]))
            assert all(t[name]["sum"] == want[9 + m] + (want[13 + m] << 32) for m, name in enumerate(R.METRICS)), (case.name, include)


def test_the_truth_wraps_and_carries_where_the_kernels_do():
    r = np.zeros(3, dtype=A.RESULT_DTYPE)
    r["clock_ns"], r["steps"] = U64, U32
    assert T.summary_truth(r, 5)[0] == [U64, 0, 3 * U32, U64 - 2]                           # 3 * (2^64 - 1) mod 2^64
    t = truth(r, 5, PASS, 2)
    assert t["clock_ns"]["sum"] == 3 * U64 and t["clock_ns"]["halves"] == (3 * U32, 3 * U32) and t["clock_ns"]["top"] == [(U64, 5), (U64, 6)]
    assert int(t["clock_ns"]["hist"][251]) == 3 and int(t["msg_count"]["hist"][0]) == 3


# ---- layer 2: the host fold (no GPU) -----------------------------------------------------------------------------------------
def batch_of(values, seed0, verdict=A.PASS):
    """(results whose four metrics all hold `values` — steps their low halves —, seed0)"""
    values = np.asarray(values, dtype=np.uint64)
    r = np.zeros(len(values), dtype=A.RESULT_DTYPE)
    r["verdict"] = verdict
    for name in METRICS64:
        r[name] = values
    r["steps"] = values & np.uint64(U32)
    return r, seed0


def fold_both_ways(batches, include, top_k, what):
    """madsim_k_fold_stats over the batches' device words — in order and in reverse — against stats_ref.fold of their truths."""
    truths = [truth(r, s, include, top_k) for r, s in batches]
    want = R.fold(truths, top_k)
    words = [T.stats_words(t) for t in truths]
    for order in (words, words[::-1]):
        got = K.fold(order, top_k, include)
        assert R.same(got, want), (what, f"seed {SEED}", {m: (got[m]["sum"], want[m]["sum"], got[m]["top"], want[m]["top"]) for m in R.METRICS}, got["n"], want["n"])
    return want


def test_fold_carries_into_sum_hi():
    two = batch_of([1 << 63, 1 << 63], 10)
    many = batch_of(np.full(1 << 16, U64, dtype=np.uint64), 1000)
    for batches in ([two], [two, two], [many], [two, many], [many, two, many]):
        want = fold_both_ways(batches, PASS, 16, "carry")
        assert want["clock_ns"]["sum"] >> 64 >= 1 and want["clock_ns"]["sum"] == sum(int(x) for r, _ in batches for x in r["clock_ns"].tolist())
    assert fold_both_ways([two, two], PASS, 2, "carry")["clock_ns"]["sum"] == 1 << 65
    assert truth(*many, PASS, 0)["rng_calls"]["halves"] == (U32 << 16, U32 << 16)             # both half-sums past 2^32


def test_fold_ignores_a_batch_that_counted_nothing():
    rng = np.random.default_rng([SEED, 1])
    a, b = (with_values(rng, 300, A.PASS, 3), 0), (with_values(rng, 200, A.PASS, 4), 600)
    nothing = (with_values(rng, 300, A.DEADLOCK, 3), 300)
    assert truth(*nothing, PASS, 16)["n"] == 0
    want = fold_both_ways([a, nothing, b], PASS, 16, "n = 0 in the middle")
    assert R.same(want, fold_both_ways([a, b], PASS, 16, "without it")) and want["n"] == 500
    assert R.same(K.fold([T.stats_words(truth(*a, PASS, 16)), T.stats_words(truth(*nothing, PASS, 16))], 16), truth(*a, PASS, 16))
    none = K.fold([T.stats_words(truth(*nothing, PASS, 16))] * 3, 16)
    assert none["n"] == none["n_top"] == 0 and all(none[m]["min"] == U64 and none[m]["max"] == 0 and none[m]["sum"] == 0 for m in R.METRICS)


def test_fold_of_batches_with_fewer_than_k_counted_seeds():
    rng = np.random.default_rng([SEED, 2])
    batches = [(few_counted(rng, 500, n), 500 * j) for j, n in enumerate((3, 0, 5, 1, 7, 2))]
    for top_k, n_top in ((16, 16), (15, 15), (2, 2), (1, 1)):
        assert fold_both_ways(batches, PASS, top_k, ("few", top_k))["n_top"] == n_top
    assert fold_both_ways(batches[:4], PASS, 16, "nine of sixteen")["n_top"] == 9
    assert fold_both_ways(batches[:4], PASS, 9, "nine of nine")["n_top"] == 9


def test_fold_of_equal_values_keeps_the_smaller_seeds():
    first, second = batch_of([7] * 6, 100), batch_of([7] * 6, 200)
    for top_k in (1, 4, 6, 8, 16):
        want = fold_both_ways([first, second], PASS, top_k, ("ties", top_k))
        assert want["clock_ns"]["top"] == [(7, s) for s in (list(range(100, 106)) + list(range(200, 206)))[:top_k]]
    # a larger value in the later batch goes in front, equal ones behind
    want = fold_both_ways([first, batch_of([7, 9, 7], 200)], PASS, 4, "mixed")
    assert want["msg_count"]["top"] == [(9, 201), (7, 100), (7, 101), (7, 102)]


@pytest.mark.parametrize("top_k", TOP_KS)
def test_fold_of_the_pieces_of_a_batch(top_k):
    """Every case of 4 097 seeds, cut into pieces of 1 000: the fold of the pieces' words is the truth of the whole (K = 0 included)."""
    for case in cases(4097):
        if case.k not in (None, top_k):
            continue
        for include in (ALL, PASS):
            batches = [(case.results[lo:lo + 1000], case.seed0 + lo) for lo in range(0, 4097, 1000)]
            want = fold_both_ways(batches, include, top_k, (case.name, include, top_k))
            assert R.same(want, truth(case.results, case.seed0, include, top_k)), (case.name, include, top_k)


# ---- layer 3: the kernels (MI355X) -------------------------------------------------------------------------------------------
def check_summaries(d, case):
    four, six = T.summary_truth(case.results, case.seed0)
    got4, got6 = K.summary(d, len(case.results), case.seed0), K.summary6(d, len(case.results), case.seed0)
    print(case.name, "summary", got4, four, "summary6", got6, six)
    assert got4 == four, (case.name, "summary_kernel", got4, four)
    assert got6 == six, (case.name, "summary6_kernel", got6, six)


def check_collect(d, case, list_runner, cap):
    results, count = case.results, len(case.results)
    what = (case.name, "list_runner", list_runner, "cap", cap)
    words, rec_bytes = T.collect_truth(results, case.seed0, cap, list_runner)
    n_recs, grid = min(cap, int(words[14])), T.cut(count)[0]
    first = None
    for launch in (1, 2):                                            # the second on freshly prepared buffers: the same bytes
        rep, wave_cnt, recs = K.collect(d, count, case.seed0, list_runner, cap)
        assert (rep == words).all(), (what, launch, rep.tolist(), words.tolist())
        assert int(rep[6:14].sum()) == count and int(rep[6]) == int((results["verdict"] == A.PASS).sum()), (what, rep[6:14].tolist())
        got = recs[:n_recs]
        assert (got["seed"] == np.frombuffer(rec_bytes, dtype=A.FAILURE_DTYPE)["seed"]).all(), (what, "seeds", got["seed"][:8])
        assert got.tobytes() == rec_bytes, (what, "record bytes")
        assert recs[n_recs:].tobytes() == bytes([K.PATTERN]) * (K.FAILURE_BYTES * (cap - n_recs)), (what, "a record beyond the list was written")
        assert (wave_cnt[:4 * grid] == T.wave_counts(results, list_runner)).all(), (what, "wave_cnt", wave_cnt[:4 * grid].tolist()[:16])
        assert (wave_cnt[4 * grid:] == K.PATTERN32).all(), (what, "wave_cnt beyond the grid")
        both = rep.tobytes() + wave_cnt.tobytes() + recs.tobytes()
        first = first or both
        assert both == first, (what, "the second launch differs")


def check_stats(d, case, include, top_k, results=None, seed0=None):
    """The 657 words of one launch against the truth; returns them."""
    results, seed0 = (case.results, case.seed0) if results is None else (results, seed0)
    what = (case.name, "include", include, "K", top_k, "seed0", seed0, "count", len(results))
    t = truth(results, seed0, include, top_k)
    want = T.stats_words(t)
    srep, cand = K.stats(d, len(results), seed0, include, top_k)
    names = ("n",) + tuple(f"{f}[{m}]" for f in ("~min", "max", "low half-sum", "high half-sum") for m in R.METRICS)
    for j, name in enumerate(names):
        assert int(srep[j]) == int(want[j]), (what, name, int(srep[j]), int(want[j]))
    bad = np.nonzero(srep[T.HIST_OFF:T.TOP_OFF] != want[T.HIST_OFF:T.TOP_OFF])[0]
    assert not len(bad), (what, "histogram words (metric, bucket pair)", [(int(j) // 128, int(j) % 128) for j in bad[:8]])
    top = srep[T.TOP_OFF:].reshape(4, 16, 2)
    if top_k == 0:
        assert (top == K.PATTERN64).all(), (what, "top words written with K = 0")
        assert (cand == K.PATTERN64).all(), (what, "cand written with K = 0")
        return srep
    for m, name in enumerate(R.METRICS):
        got = [(int(v), int(s)) for v, s in top[m, :t["n_top"]]]
        assert got == t[name]["top"], (what, name, "top", got, t[name]["top"])
        assert not top[m, t["n_top"]:].any(), (what, name, "a top slot at n_top or beyond is not zero", top[m].tolist())
    assert (srep == want).all(), what
    assert (cand.reshape(4, K.COLLECT_WAVES // 4, 16, 2)[:, T.cut(len(results))[0]:] == K.PATTERN64).all(), (what, "cand of a workgroup that does not run")
    return srep


def check_case(d, case, every_cap):
    check_summaries(d, case)
    for list_runner in (0, 1):
        n_listed = int(T.listed_mask(case.results, list_runner).sum())
        for cap in caps(case.results, list_runner) if every_cap else sorted({0, min(n_listed, len(case.results))}):
            check_collect(d, case, list_runner, cap)
    for include, top_k in stats_settings(case):
        check_stats(d, case, include, top_k)


@pytest.mark.gpu
@pytest.mark.parametrize("count", SMALL)
def test_every_case_at_a_small_count(hip, count):
    """Every family at 1 .. 4 097 seeds (one partial wave; one workgroup; two, whose waves 6 and 7 own nothing; five, whose last wave owns
    one seed): summary, summary6, collect at list_runner 0 and 1 with every cap, the statistics at every K."""
    for case in cases(count):
        check_case(K.upload(case.results), case, every_cap=True)


BIG_CASES = [(count, number) for count in (262_144, 262_209) for number, name in enumerate(case_names(count))
             if (count == 262_209 and not (name.startswith("all-") and name not in ("all-pass", "all-deadlock", "all-internal-invariant")))
             or name in ("values0", "values3", "all-pass", "ascending", "constant", "ties-k16-ending") or name.endswith(("@1023", "@1024"))]


@pytest.mark.gpu
@pytest.mark.parametrize("count,number", BIG_CASES, ids=[f"{c}-{case_names(c)[n]}" for c, n in BIG_CASES])
def test_a_case_at_the_grid_cap(hip, count, number):
    """262 144 seeds: 256 workgroups, every wave a full piece of 256.  262 209: pieces of 320, waves 0 .. 819 own results, the last one
    129 (a partial round), 204 workgroups' candidates and 52 empty lists merged by stats_top_kernel: 4 096 candidates, 16 rounds a wave."""
    case = make_case(count, number)
    check_case(K.upload(case.results), case, every_cap=case.name.endswith(("values0", "values3")))


@pytest.mark.gpu
@pytest.mark.parametrize("count", COUNTS)
def test_every_seed0(hip, count):
    """seed0 = 0, 2^40 + 7 and 2^64 - count (the last seed is 2^64 - 1) over one array of uniform verdicts."""
    base = make_case(count, 3)
    d = K.upload(base.results)
    for seed0 in seed0s(count):
        case = base._replace(name=f"{base.name} seed0 {seed0}", seed0=seed0)
        check_summaries(d, case)
        for list_runner in (0, 1):
            check_collect(d, case, list_runner, int(T.listed_mask(case.results, list_runner).sum()))
        check_stats(d, case, ALL, 16)
        check_stats(d, case, PASS, 1)


def cap_inside_a_round(count, wave, rng):
    """All PASS but: 37 listed seeds in the pieces before `wave`, 5 in its first round, all 64 lanes of its second round, and more behind
    — so the wave's offset is 37 (not a multiple of 64) and its second round begins at record 42."""
    grid, piece, last_wave = owned(count)
    assert 1 <= wave < last_wave and piece >= 192
    r = with_values(rng, count, A.PASS, 3)
    lo = wave * piece
    r["verdict"][rng.choice(lo, 37, replace=False)] = A.DEADLOCK
    r["verdict"][lo + rng.choice(64, 5, replace=False)] = A.PANIC
    r["verdict"][lo + 64:lo + 128] = A.TIME_LIMIT
    r["verdict"][lo + 128 + rng.choice(count - lo - 128, 50, replace=False)] = A.DEADLOCK
    return r


@pytest.mark.gpu
@pytest.mark.parametrize("count,wave", [(4097, 1), (4097, 9), (262_209, 2), (262_209, 613)])
def test_cap_ends_inside_a_round_of_a_wave_with_an_offset(hip, count, wave):
    results = cap_inside_a_round(count, wave, np.random.default_rng([SEED, count, wave]))
    case = Case(f"seed {SEED} count {count} cap inside a round of wave {wave}", results, seed0s(count)[wave % 3], None)
    assert int(T.wave_counts(results, 0)[:wave].sum()) == 37 and int(T.wave_counts(results, 0)[wave]) >= 69
    d = K.upload(results)
    for into in (1, 32, 63):
        check_collect(d, case, 0, 42 + into)
    for cap in (37, 38, 42, 42 + 64, 42 + 65):                       # the wave's first record, its round's edges
        check_collect(d, case, 0, cap)


@functools.lru_cache(maxsize=None)
def composition_array():
    return make_case(262_209, 2)                                     # values2: bucket edges, uniform 64 bits, every bit length, one maximum


@pytest.mark.gpu
@pytest.mark.parametrize("include,top_k", [(ALL, 16), (PASS, 16), (ALL, 2), (PANIC_TL, 0)])
def test_device_words_through_the_host_fold(hip, include, top_k):
    """One 262 209-seed array cut into batches of 100 000: each batch's device words (checked), folded in order by madsim_k_fold_stats,
    are the truth of the whole and stats_ref.fold of the parts; so is the one-batch form."""
    case = composition_array()
    whole = truth(case.results, case.seed0, include, top_k)
    assert whole["msg_count"]["sum"] >> 64 and whole["n"] > 30_000
    words, parts = [], []
    for lo in range(0, 262_209, 100_000):
        part = case.results[lo:lo + 100_000]
        srep = check_stats(K.upload(part), case, include, top_k, part, case.seed0 + lo)
        if top_k == 0:
            srep[T.TOP_OFF:] = 0                                     # (words the campaign does not read back with K = 0)
        words.append(srep)
        parts.append(truth(part, case.seed0 + lo, include, top_k))
    got = K.fold(words, top_k, include)
    assert R.same(got, whole), (case.name, include, top_k, "the fold of the device's words is not the truth of the whole")
    assert R.same(got, R.fold(parts, top_k)), (case.name, include, top_k)
    one = check_stats(K.upload(case.results), case, include, top_k)
    if top_k == 0:
        one[T.TOP_OFF:] = 0
    assert R.same(K.fold([one], top_k, include), whole), (case.name, include, top_k, "one batch")
