"""span_fold_kernel and span_witness_kernel on synthetic rows (tests/spans_kernels.py drives the launcher directly) against the numpy
reference (tests/spans_ref.py): every size around a wave and a round of 64, the placements of `from` and `to` that the walk can get wrong,
the values and lengths at their edges, every verdict and mask, durations at the edges of 64 bits and of a bucket, ties of an extreme inside
a workgroup and across two, and both forms of the fold kernel — the accumulator in LDS and every update straight to global memory — which
must give the same bytes."""
import numpy as np
import pytest

from madsim_amd import _abi as A
from tests import spans_kernels as K
from tests import spans_ref as R

pytestmark = pytest.mark.gpu

U64 = (1 << 64) - 1
P, PA, D, TL = A.PASS, A.PANIC, A.DEADLOCK, A.TIME_LIMIT
SPANS = [(100, 200), (None, 200), (300, 300), (0, U64), (200, 100), (U64, 0), (None, 0)]


def results_of(verdicts):
    res = np.zeros(len(verdicts), dtype=A.RESULT_DTYPE)
    res["verdict"] = np.array(verdicts, dtype=np.uint64).astype(np.uint32)
    res["clock_ns"] = 0x1111111111111111                                                # (nothing but the verdict may matter)
    return res


def run(rows, times, lens, verdicts, seeds, spans, include=0xf, launches=1):
    """Both forms of the fold kernel against the reference: records (through the library's host fold), words, and the per-(seed, span)
    states and durations the witness kernel reads.  Returns the reference."""
    rows, times = np.ascontiguousarray(rows, dtype=np.uint64), np.ascontiguousarray(times, dtype=np.uint64)
    n, cap = rows.shape
    defs = R.defs_of(spans)
    want = R.report(rows, times, lens, verdicts, seeds, defs, include, cap)
    st, du = R.states(rows, times, lens, defs, cap)
    v = np.asarray(verdicts, dtype=np.uint64)
    counted = (v < 4) & (((include >> np.minimum(v, 63).astype(np.int64)) & 1) == 1)
    st = np.where(counted[:, None], st, K.UNCOUNTED)
    raw = []
    for direct in (False, True):
        for recs, words, got_st, got_du in K.probe_spans(rows, times, lens, results_of(verdicts), seeds, include, defs, launches=launches, direct=direct):
            assert (got_st == st).all(), (direct, np.argwhere(got_st != st)[:5])
            assert (got_du[counted] == du[counted]).all(), direct
            assert (words == want.words()).all(), (direct, words, want.words())
            spans_got, n_counted, n_trunc, n_runner = K.decode(defs, recs, words, include, cap)
            for f in spans_got.dtype.names:
                assert (spans_got[f] == want.spans[f]).all(), (direct, f, spans_got[f], want.spans[f])
            assert spans_got.tobytes() == want.spans.tobytes() and (n_counted, n_trunc, n_runner) == (want.n_counted, want.n_truncated, want.n_runner)
            raw.append(recs)
    assert all((r == raw[0]).all() for r in raw)             # the same words, whichever form and launch
    return want


def random_case(rng, n, cap):
    vocab = np.array([0, U64, 100, 200, 300, 7, 7, 7], dtype=np.uint64)
    rows = rng.choice(vocab, (n, cap))
    quiet = rng.random(n) < 0.15                           # rows that begin a span and never end it: OPEN, or CUT where the list was cut
    rows[quiet] = 7
    rows[quiet, 0] = 100
    lens = rng.integers(0, cap + 9, n).astype(np.uint64)
    lens[rng.random(n) < 0.1] = 0
    steps = rng.integers(0, 1 << 30, (n, cap)).astype(np.uint64)
    steps[rng.random((n, cap)) < 0.02] = np.uint64(1 << 61)
    times = np.cumsum(steps, axis=1, dtype=np.uint64)
    verdicts = rng.choice(np.array([0, 0, 0, 1, 2, 2, 3, 4, 5, 7, 0xffffffff], dtype=np.uint64), n)
    seeds = rng.permutation(np.arange(n, dtype=np.uint64) * np.uint64(3) + np.uint64(5))
    seeds[int(rng.integers(0, n))] = np.uint64(U64)
    return rows, times, lens, verdicts, seeds


@pytest.mark.parametrize("n", [1, 63, 64, 65, 1025])
@pytest.mark.parametrize("cap", [1, 63, 64, 65, 256])
def test_random_rows_at_every_size(n, cap):
    """Lengths from 0 to past the cap: the words behind min(len, cap) hold probe values and must be ignored; len > cap is CUT where the
    span is not closed inside the prefix."""
    rng = np.random.default_rng(1000 * n + cap)
    rows, times, lens, verdicts, seeds = random_case(rng, n, cap)
    want = run(rows, times, lens, verdicts, seeds, SPANS)
    if n >= 1025 and cap >= 63:
        ns = want.spans["n_state"].sum(axis=1)
        assert (ns[0] > 0).all() and want.n_truncated and want.n_runner and want.spans["n"][2] > 0      # every state of 100 -> 200; periods of 300


def directed(cap=130):
    """(rows, times, what each row is) — one row per placement the walk can get wrong.  Times are 1000 * (index + 1) unless said otherwise."""
    cases = []

    def row(values, length=None, times=None, verdict=P):
        r = np.full(cap, 7, dtype=np.uint64)
        r[:len(values)] = np.array([int(x) for x in values], dtype=np.uint64)
        t = np.arange(1, cap + 1, dtype=np.uint64) * np.uint64(1000)
        if times is not None:
            t[:len(times)] = np.array([int(x) for x in times], dtype=np.uint64)
        cases.append((r, t, len(values) if length is None else length, verdict))

    seven = [7] * 63
    row(seven + [100, 200])                                  # 0: from in lane 63 of a round, to in lane 0 of the next
    row([7, 100, 7, 200])                                    # 1: one round, from first: closed
    row([7, 200, 7, 100])                                    # 2: to only before from: OPEN (and 200 -> 100 closed)
    row([300])                                               # 3: from == to, one occurrence: OPEN
    row([300, 7, 300])                                       # 4: two: the period
    row([300, 7, 300, 300])                                  # 5: three: still the first two
    row([200, 100])                                          # 6: the start flag with `to` at index 0: the duration is time[0]
    row([0, U64, 0])                                         # 7: the values 0 and 2^64 - 1, both ways round
    row([100, 200] + [7] * (cap - 2), length=cap + 5)        # 8: len > cap, closed inside the prefix: the true span
    row([100] + [7] * (cap - 1), length=cap + 5)             # 9: len > cap, not closed: CUT
    row([100, 7, 7], length=1)                               # 10: words behind the length are ignored ...
    r = cases[-1][0]; r[1] = 200                             # ... even where they hold `to`: OPEN
    row([100, 200], times=[5, 5])                            # 11: duration 0
    row([100, 200], times=[5, 6])                            # 12: 1
    row([100, 200], times=[0, 1 << 63])                      # 13: 2^63
    row([100, 200], times=[0, U64])                          # 14: 2^64 - 1
    lo, hi = A.stat_bucket_floor(100), A.stat_bucket_floor(101) - 1
    row([100, 200], times=[10, 10 + lo])                     # 15, 16: both edges of bucket 100
    row([100, 200], times=[10, 10 + hi])
    row([100, 200], verdict=A.OVERFLOW)                      # 17: a runner verdict: counted in n_runner, never read
    row([100, 200], verdict=D)
    row([100, 7], verdict=TL)
    row([100, 200], verdict=PA)
    row([])                                                  # 21: an empty list: ABSENT, and OPEN from the start
    rows, times = np.stack([c[0] for c in cases]), np.stack([c[1] for c in cases])
    return rows, times, np.array([c[2] for c in cases], dtype=np.uint64), np.array([c[3] for c in cases], dtype=np.uint64)


def test_directed_placements_values_lengths_and_durations():
    rows, times, lens, verdicts = directed()
    seeds = np.arange(len(rows), dtype=np.uint64) + np.uint64(1000)
    defs = R.defs_of(SPANS)
    st, du = R.states(rows, times, lens, defs, rows.shape[1])
    C, O, AB, CU = R.CLOSED, R.OPEN, R.ABSENT, R.CUT
    # the reference itself, against the issue's words, span 0 = 100 -> 200 unless said otherwise
    assert (st[0, 0], du[0, 0]) == (C, 1000) and (st[1, 0], du[1, 0]) == (C, 2000) and st[2, 0] == O and (st[2, 4], du[2, 4]) == (C, 2000)
    assert st[3, 2] == O and (st[4, 2], du[4, 2]) == (C, 2000) == (st[5, 2], du[5, 2])
    assert (st[6, 1], du[6, 1]) == (C, 1000) and (st[7, 3], du[7, 3]) == (C, 1000) == (st[7, 5], du[7, 5]) and (st[7, 6], du[7, 6]) == (C, 1000)
    assert (st[8, 0], st[9, 0], st[10, 0]) == (C, CU, O) and [int(x) for x in du[11:15, 0]] == [0, 1, 1 << 63, U64]
    assert A.stat_bucket(int(du[15, 0])) == A.stat_bucket(int(du[16, 0])) == 100 and A.stat_bucket(int(du[16, 0]) + 1) == 101
    assert st[21, 0] == AB and st[21, 1] == O
    want = run(rows, times, lens, verdicts, seeds, SPANS)
    s0 = want.spans[0]
    assert (int(s0["min"]), int(s0["max"]), int(s0["min_seed"]), int(s0["max_seed"])) == (0, U64, 1011, 1014) and int(s0["hist"][100]) == 2
    assert int(s0["sum_hi"]) == 1 and want.n_runner == 1 and want.n_truncated == 2 and int(s0["first_open_seed"]) == 1002
    assert [int(x) for x in s0["n_state"][D]] == [0, 1, 0, 0] and [int(x) for x in s0["n_state"][TL]] == [0, 0, 1, 0]
    for v in range(4):                                       # every include mask of one verdict
        one = run(rows, times, lens, verdicts, seeds, SPANS, include=1 << v)
        assert sum(one.n_counted) == one.n_counted[v] == int((verdicts == v).sum()) and one.n_runner == 1
    run(rows, times, lens, verdicts, seeds, [(100, 200)] * 16)      # 16 equal definitions ...
    run(rows, times, lens, verdicts, seeds, [(100, 200)])           # ... and one
    run(rows, times, lens, verdicts, seeds, SPANS, launches=2)       # two launches in a row over the same buffers


@pytest.mark.parametrize("kind", ["max", "min", "open"])
@pytest.mark.parametrize("n,tied", [(8, (1, 2)), (8, (1, 5)), (2050, (3, 2049)), (1025, (0, 1024))])
def test_ties_of_an_extreme_go_to_the_smaller_seed(n, tied, kind):
    """Rows 1 and 2 share a workgroup (two of its waves); rows 1 and 5, and 3 and 2049, lie in two workgroups; rows 0 and 1024 meet in one
    wave's stride.  The seeds DESCEND with the row, so the later row holds the smaller seed, which must win — for the minimum, the maximum
    and OPEN."""
    cap = 4
    rows = np.full((n, cap), 7, dtype=np.uint64)
    rows[:, 0], rows[:, 1] = 100, 200
    times = np.zeros((n, cap), dtype=np.uint64)
    times[:, 1] = 500
    for r in tied:
        if kind == "open":
            rows[r, 1] = 7
        else:
            times[r, 1] = 900 if kind == "max" else 100
    seeds = np.uint64(U64) - np.arange(n, dtype=np.uint64) * np.uint64(7)
    want = run(rows, times, np.full(n, 2, dtype=np.uint64), np.zeros(n, dtype=np.uint64), seeds, [(100, 200), (None, 200)])
    field = {"max": "max_seed", "min": "min_seed", "open": "first_open_seed"}[kind]
    assert int(want.spans[field][0]) == int(seeds[max(tied)]) and int(want.spans["n_state"][0][P][R.OPEN]) == (2 if kind == "open" else 0)


def test_seeds_up_to_the_top_and_nothing_closed():
    rows = np.array([[100, 7], [7, 7], [100, 200]], dtype=np.uint64)
    times = np.array([[1, 2], [1, 2], [1, 2]], dtype=np.uint64)
    seeds = np.array([U64, U64 - 1, 0], dtype=np.uint64)
    want = run(rows, times, [2, 2, 2], [0, 0, 4], seeds, [(100, 200), (200, 100)])          # the one closing row has a runner verdict
    assert int(want.spans["n"][0]) == 0 and int(want.spans["first_open_seed"][0]) == U64 and int(want.spans["min"][0]) == U64
    assert int(want.spans["first_open_seed"][1]) == U64 and int(want.spans["n_state"][1][:, R.OPEN].sum()) == 0
    want = run(rows, times, [2, 2, 2], [0, 0, 0], seeds, [(100, 200)])
    assert (int(want.spans["min_seed"][0]), int(want.spans["first_open_seed"][0])) == (0, U64)


def test_the_launcher_refuses_what_the_kernels_are_not_written_for():
    assert K.refused() == 0
    for bad in (dict(n=0), dict(n=(1 << 31) + 1), dict(n=1 << 24, obs_cap=256), dict(obs_cap=0), dict(obs_cap=A.CENSUS_MAX_OBS_CAP + 1), dict(m=0),
                dict(m=17), dict(include=0), dict(include=0x10), dict(flags=2), dict(missing="obs"), dict(missing="times"), dict(missing="len"),
                dict(missing="res"), dict(missing="seeds"), dict(missing="defs"), dict(missing="st"), dict(missing="dur"), dict(missing="recs"),
                dict(missing="words")):
        assert K.refused(**bad) == -1, bad
