"""The LIST forms of the report kernels (summary6, collect count + write, statistics top, group extract, diff write, resolve write:
csrc/sim_kernel.hip, instantiated on ListSeeds) on synthetic result arrays, launched directly (tests/seedlist_kernels.py) and held, exactly,
against tests/seedlist_ref.py.  Three lists per count: DENSE (2^40 + 7 + i: the bytes must also equal what the RANGE launcher writes for
the same array and seed0 — both are launched here, so a divergence between the two instantiations is caught directly), GAPPED (from 0, the
gaps cycling 1, 2, 3, 2^33: catches a 32-bit truncation of the seed and a confusion of index and seed) and TOP (the last `count` integers
below 2^64: bit 63 set, the sentinel value itself a member).  The result arrays come from the generators of tests/test_report_kernels.py
and its siblings.  Every word, record, entry and wave count is compared."""
import numpy as np
import pytest

from madsim_amd import _abi as A
from tests import diff_kernels as KD
from tests import diff_ref as D
from tests import group_kernels as KG
from tests import report_kernels as K
from tests import report_ref as T
from tests import resolve_kernels as KR
from tests import seedlist_kernels as KL
from tests import seedlist_ref as S
from tests import stats_ref as R
from tests import test_group_kernels as PG
from tests import test_report_kernels as P
from tests import test_resolve_kernels as PR

pytestmark = pytest.mark.gpu

SEED = 20261019
COUNTS = (1, 63, 64, 65, 1023, 1025, 4097)
GRID_CAP = 262_209                                                  # 256 workgroups, pieces of 320, the last piece in use ragged
SEED0 = (1 << 40) + 7                                               # the dense list's first seed


def lists(count):
    """[(name, host list, device list, the seed0 of the range it equals or None)]"""
    return [(name, make(count), KL.SeedList(make(count)), SEED0 if name == "dense" else None) for name, make in S.LISTS]


def report_cases(count):
    """Every verdict value with the runner verdicts (values3), verdicts of 8 and more, a passing batch (no list entry is read), a total tie,
    ties at rank K across a boundary, and a single failure at the last index."""
    names = P.case_names(count)
    want = ["values3", "verdicts-8-and-more", "all-pass", "constant", "ties-k16-straddling", "ties-k2-ending", f"single-{A.VERDICT_NAMES[A.PANIC]}@0"]
    picked = [names.index(n) for n in want if n in names]
    picked += [j for j, n in enumerate(names) if n.endswith(f"@{count - 1}") and j not in picked][:1]
    return [P.make_case(count, j) for j in picked]


def check_summary6(d, results, seeds, sl, seed0, what):
    got, want = KL.summary6(d, len(results), sl), S.summary6_truth(results, seeds)
    print(what, "summary6", got, want)
    assert got == want, (what, "summary6", got, want)
    if seed0 is not None:
        assert got == K.summary6(d, len(results), seed0), (what, "summary6: list and range instantiations differ")


def check_collect(d, results, seeds, sl, seed0, list_runner, cap, what):
    count = len(results)
    what = (what, "list_runner", list_runner, "cap", cap)
    words, rec_bytes = S.collect_truth(results, seeds, cap, list_runner)
    rep, wave_cnt, recs = KL.collect(d, count, sl, list_runner, cap)
    n_recs, grid = min(cap, int(words[14])), T.cut(count)[0]
    assert (rep == words).all(), (what, rep.tolist(), words.tolist())
    got = recs[:n_recs]
    assert (got["seed"] == np.frombuffer(rec_bytes, dtype=A.FAILURE_DTYPE)["seed"]).all(), (what, "seeds", got["seed"][:8])
    assert got.tobytes() == rec_bytes, (what, "record bytes")
    assert recs[n_recs:].tobytes() == bytes([K.PATTERN]) * (K.FAILURE_BYTES * (cap - n_recs)), (what, "a record beyond the list was written")
    assert (wave_cnt[:4 * grid] == T.wave_counts(results, list_runner)).all(), (what, "wave_cnt")
    assert (wave_cnt[4 * grid:] == K.PATTERN32).all(), (what, "wave_cnt beyond the grid")
    if seed0 is not None:
        r_rep, r_cnt, r_recs = K.collect(d, count, seed0, list_runner, cap)
        assert rep.tobytes() + wave_cnt.tobytes() + recs.tobytes() == r_rep.tobytes() + r_cnt.tobytes() + r_recs.tobytes(), (what, "list and range differ")


def check_stats(d, results, seeds, sl, seed0, include, top_k, what, range_cand):
    """The 657 words against the truth; the candidate words hold indices, never seeds, so they equal the range launcher's for every list."""
    what = (what, "include", include, "K", top_k)
    t = S.stats_truth(results, seeds, include, top_k)
    want = T.stats_words(t)
    srep, cand = KL.stats(d, len(results), sl, include, top_k)
    assert (srep[:T.TOP_OFF] == want[:T.TOP_OFF]).all(), (what, "counts, extremes, sums or histogram words")
    top = srep[T.TOP_OFF:].reshape(4, 16, 2)
    if top_k == 0:
        assert (top == K.PATTERN64).all() and (cand == K.PATTERN64).all(), (what, "top or cand written with K = 0")
    else:
        for m, name in enumerate(R.METRICS):
            got = [(int(v), int(s)) for v, s in top[m, :t["n_top"]]]
            assert got == t[name]["top"], (what, name, "top", got[:4], t[name]["top"][:4])
        assert (srep == want).all(), what
    key = (include, top_k)
    if key not in range_cand:
        range_cand[key] = K.stats(d, len(results), SEED0, include, top_k)
    r_srep, r_cand = range_cand[key]
    assert cand.tobytes() == r_cand.tobytes(), (what, "candidate words differ from the range launcher's")
    if seed0 is not None:
        assert srep.tobytes() == r_srep.tobytes(), (what, "list and range differ")


def check_report_case(case, all_lists, every_cap):
    d = K.upload(case.results)
    range_cand = {}
    for name, seeds, sl, seed0 in all_lists:
        what = (case.name, name)
        check_summary6(d, case.results, seeds, sl, seed0, what)
        for list_runner in (0, 1):
            n_listed = int(T.listed_mask(case.results, list_runner).sum())
            for cap in P.caps(case.results, list_runner) if every_cap else sorted({0, min(n_listed, len(case.results))}):
                check_collect(d, case.results, seeds, sl, seed0, list_runner, cap, what)
        for include, top_k in ([(P.ALL, case.k), (P.PASS, case.k)] if case.k is not None else [(P.ALL, 16), (P.ALL, 1), (P.PANIC_TL, 2), (P.PASS, 0)]):
            check_stats(d, case.results, seeds, sl, seed0, include, top_k, what, range_cand)


@pytest.mark.parametrize("count", COUNTS)
def test_summary6_collect_and_statistics(hip, count):
    all_lists = lists(count)
    for j, case in enumerate(report_cases(count)):
        check_report_case(case, all_lists, every_cap=j < 2)


def test_summary6_collect_and_statistics_at_the_grid_cap(hip):
    """262 209 results: 1 024 waves, pieces of 320, 820 in use: uniform verdicts with the caps 0, 1, L - 1, L, L + 1, and ties at rank 16."""
    all_lists = lists(GRID_CAP)
    names = P.case_names(GRID_CAP)
    check_report_case(P.make_case(GRID_CAP, names.index("values3")), all_lists, every_cap=False)
    case = P.make_case(GRID_CAP, names.index("ties-k16-ending"))
    d, range_cand = K.upload(case.results), {}
    for name, seeds, sl, seed0 in all_lists:
        check_stats(d, case.results, seeds, sl, seed0, P.ALL, 16, (case.name, name), range_cand)
        check_collect(d, case.results, seeds, sl, seed0, 1, 1, (case.name, name))


@pytest.mark.parametrize("count,wave", [(4097, 9), (GRID_CAP, 613)])
def test_a_collect_cap_that_ends_inside_a_round(hip, count, wave):
    """test_report_kernels' array: 37 listed seeds before `wave`, 5 in its first round, 64 in its second — the list ends inside that round."""
    results = P.cap_inside_a_round(count, wave, np.random.default_rng([SEED, count, wave]))
    d = K.upload(results)
    for name, seeds, sl, seed0 in lists(count):
        for cap in (0, 37, 38, 42, 43, 42 + 32, 42 + 63, 42 + 64, 42 + 65):
            check_collect(d, results, seeds, sl, seed0, 0, cap, ("cap inside a round", count, wave, name))


# ---- groups ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("count", COUNTS)
def test_groups(hip, count):
    """Few groups, some, and nearly one per seed (test_group_kernels.mixed: verdicts 0-3 and the runner verdicts); every entry, sorted by
    first_seed — arrival order is no part of the answer."""
    all_lists = lists(count)
    for case, n_keys in enumerate((1, 5, 1 << 20)):
        results = PG.mixed(np.random.default_rng([SEED, count, case]), count, n_keys)
        d = KG.upload(results)
        for include, key_field in ((15, A.GROUP_KEY_OBS), (0b1110, A.GROUP_KEY_STEPS)):
            ranged = None
            for name, seeds, sl, seed0 in all_lists:
                what = (SEED, "groups", count, n_keys, include, key_field, name)
                n, entries, _ = KL.groups(d, count, sl, include, key_field)
                got, want = KG.by_first_seed(entries), S.all_groups(results, seeds, include, key_field)
                assert n == len(want) and got == want, (what, n, len(want), [x for x in zip(got, want) if x[0] != x[1]][:3])
                if seed0 is not None:
                    ranged = KG.by_first_seed(KG.groups(d, count, seed0, include, key_field)[1])
                    assert got == ranged, (what, "list and range differ")
            assert ranged is not None


# ---- diff --------------------------------------------------------------------------------------------------------------------------
def check_diff(da, db, a, b, seeds, sl, seed0, fields, cap, what):
    words, waves, recs = KL.diff(da, db, len(a), sl, fields, cap)
    want = S.diff_truth(a, b, seeds, fields, min(cap, len(a)))
    assert words.tolist() == D.words_of(a, b, fields).tolist(), (SEED, what, "words")
    assert waves.tolist() == D.wave_counts(a, b, fields)[1], (SEED, what, "wave counts")
    assert len(recs) == want["n_listed"] and recs.tobytes() == want["records"], (SEED, what, recs["seed"][:4], len(recs), want["n_listed"])
    if seed0 is not None:
        r_words, r_waves, r_recs = KD.diff(da, db, len(a), seed0, fields, cap)
        assert words.tobytes() + waves.tobytes() + recs.tobytes() == r_words.tobytes() + r_waves.tobytes() + r_recs.tobytes(), (SEED, what, "list and range differ")


@pytest.mark.parametrize("count", COUNTS + (GRID_CAP,))
def test_diff(hip, count):
    """diff_ref.synthetic (every verdict value on either side, runner verdicts among them): room for everything, cap = 0, a short cap, two masks."""
    a, b = D.synthetic(np.random.default_rng([SEED, count]), count, p_differ=0.3 if count < 5000 else 0.01)
    da, db = KD.upload(a), KD.upload(b)
    for name, seeds, sl, seed0 in lists(count):
        for fields, cap in ((A.DIFF_ALL, count), (A.DIFF_ALL, 0), (A.DIFF_ALL, 7), (A.DIFF_VERDICT | A.DIFF_OBS, 2)):
            check_diff(da, db, a, b, seeds, sl, seed0, fields, cap, ("diff", count, name, fields, cap))


@pytest.mark.parametrize("count", (4097, GRID_CAP))
def test_a_diff_cap_that_ends_inside_a_round(hip, count):
    """Wave 0 holds 100 differing seeds, wave 1 forty in its second round: the list ends inside that round, at a wave whose offset is not 0."""
    rng = np.random.default_rng([SEED, count, 5])
    a = D.synthetic(rng, count, 0.0, verdicts=(0, 1, 2, 3))[0]
    b = a.copy()
    piece = D.wave_counts(a, b, A.DIFF_OBS)[0]
    b["obs_hash"][np.arange(100)] ^= np.uint64(1)
    b["obs_hash"][piece + 64 + np.arange(0, 60, 3)] ^= np.uint64(1)
    b["obs_hash"][piece + 65 + np.arange(0, 60, 3)] ^= np.uint64(2)
    assert D.wave_counts(a, b, A.DIFF_OBS)[1][:2] == [100, 40]
    da, db = KD.upload(a), KD.upload(b)
    for name, seeds, sl, seed0 in lists(count):
        for cap in (99, 100, 101, 117, 139, 140, 141):
            check_diff(da, db, a, b, seeds, sl, seed0, A.DIFF_OBS, cap, ("inside", count, name, cap))


# ---- resolve -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("count", COUNTS)
def test_resolve_lists(hip, count):
    """test_resolve_kernels' cases (none, every, the last lane, every verdict value, step limits) with both settings of steps_maxed."""
    all_lists = lists(count)
    for case, results in PR.cases(np.random.default_rng([SEED, count]), count).items():
        d = KR.upload(results)
        for steps_maxed in (0, 1):
            for name, seeds, sl, seed0 in all_lists:
                what = (SEED, "resolve", count, case, steps_maxed, name)
                want_seeds, want_idx = S.resolve_truth(results, seeds, steps_maxed)
                m, got_seeds, got_idx = KL.resolve_list(d, count, sl, steps_maxed)
                assert m == len(want_idx) and (got_idx == want_idx).all() and (got_seeds == want_seeds).all(), (what, m, len(want_idx), got_seeds[:4], want_seeds[:4])
                if seed0 is not None:
                    r_m, r_seeds, r_idx = KR.resolve_list(d, count, seed0, steps_maxed)
                    assert (m, got_seeds.tobytes(), got_idx.tobytes()) == (r_m, r_seeds.tobytes(), r_idx.tobytes()), (what, "list and range differ")
