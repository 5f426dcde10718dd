"""The sweep campaign's report kernels (sweep_count_kernel + sweep_write_kernel, csrc/sim_kernel.hip) on SYNTHETIC result arrays, launched
directly (tests/sweep_kernels.py): every word, every record byte and every wave count is held against tests/sweep_ref.py, exactly.
Arrays the simulator rarely or never produces: all 256 fail masks at once, verdicts up to 2^32 - 1 in any variant, a runner verdict in one
variant beside variants that differ everywhere, a single field differing in its top half or in bit 0 only, every seed selected, none
selected, selected seeds on both sides of a 64-seed round's edge, and a list that ends inside a round of a wave whose offset is not zero.
Every array comes from numpy.random.default_rng([SEED, ...]); SEED is in every assertion message."""
import numpy as np
import pytest

from madsim_amd import _abi as A
from tests import diff_ref
from tests import sweep_kernels as K
from tests import sweep_ref as R

pytestmark = pytest.mark.gpu

SEED = 20261019
COUNTS = (1, 63, 64, 65, 1023, 1024, 1025, 4097, 262_209)          # the last: 256 workgroups (the grid cap) and a ragged last piece
CAPS = (0, 1, 2, 63, 64, 65)
MASKS = (0,) + tuple(1 << i for i in range(7)) + (A.DIFF_ALL, A.DIFF_ALL & ~A.DIFF_TRACE)
RULES = (R.MIXED, R.FAILING, R.DIFFERING)
VS = (2, 3, 5, 8)
VERDICTS = np.array([0, 0, 0, 0, 0, 0, 1, 2, 3, 4, 5, 7, 0xffffffff], dtype=np.uint32)


def seed0s(count):
    return (0, (1 << 40) + 7, (1 << 64) - count)                    # the last: the batch ends with seed 2^64 - 1


def gappy(rng, count):
    """A strictly ascending list of `count` seeds with gaps, ending near 2^64."""
    s = np.cumsum(rng.integers(1, 1 << 20, count, dtype=np.uint64))
    return s + (np.uint64((1 << 64) - 1) - s[-1])


def base_results(rng, n, verdict=A.PASS):
    """n results: `verdict` (a value or an array), every other field random."""
    a = np.zeros(n, dtype=A.RESULT_DTYPE)
    a["verdict"] = verdict
    a["steps"] = rng.integers(0, 1 << 32, n, dtype=np.uint64)
    for name in diff_ref.WIDE:
        a[name] = rng.integers(0, 1 << 64, n, dtype=np.uint64)
    return a


def variants_of(rng, n, V, p):
    """V variants of n results: variant 0 random with VERDICTS' mix; every other variant is variant 0 with about p of its seeds changed — a
    new verdict, a bit of steps, a bit of one 64-bit field, each with probability one half."""
    out = [base_results(rng, n, rng.choice(VERDICTS, n))]
    for _ in range(1, V):
        b = out[0].copy()
        hit = rng.random(n) < p
        sub = lambda: hit & (rng.random(n) < 0.5)
        m = sub()
        b["verdict"][m] = rng.choice(VERDICTS, int(m.sum()))
        m = sub()
        b["steps"][m] ^= (np.uint32(1) << rng.integers(0, 32, int(m.sum()), dtype=np.uint32))
        name = diff_ref.WIDE[int(rng.integers(0, len(diff_ref.WIDE)))]
        m = sub()
        b[name][m] ^= (np.uint64(1) << rng.integers(0, 64, int(m.sum()), dtype=np.uint64))
        out.append(b)
    return out


def check(res, seeds, fields, rule, cap, what, d=None, d_seeds=None):
    """One launch against the truth; returns the truth.  `seeds`: an int (the range form) or an array (the list form, d_seeds its upload)."""
    d = d if d is not None else [K.upload(r) for r in res]
    n = len(res[0])
    if not isinstance(seeds, int) and d_seeds is None:
        d_seeds = K.upload_seeds(seeds)
    words, waves, recs = K.sweep(d, n, seeds if isinstance(seeds, int) else d_seeds, fields, rule, cap)
    want = R.sweep_truth(res, seeds, fields, rule, min(cap, n))
    want_words = R.words_of(res, fields, rule)
    piece, want_waves = R.wave_counts(res, fields, rule)
    print(what, "selected", int(words[0]), "want", want["n_selected"], "incomparable", int(words[1]), "listed", len(recs))
    assert words.tolist() == want_words.tolist(), (SEED, what, words[:18].tolist(), want_words[:18].tolist())
    assert waves.tolist() == want_waves, (SEED, what, piece)
    assert len(recs) == want["n_listed"] and recs.tobytes() == want["records"], (SEED, what, recs["seed"][:4], len(recs), want["n_listed"])
    assert int(words[18:].sum()) + int(words[1]) == n and not words[18 + (1 << len(res)):].any()
    return want


@pytest.mark.parametrize("count", COUNTS)
def test_counts_seeds_rules_and_masks(hip, count):
    """Random variants at every count: every seed0 and a list with gaps, every rule, every mask, a cap that takes everything and one that
    does not."""
    V = VS[COUNTS.index(count) % len(VS)]
    rng = np.random.default_rng([SEED, count])
    res = variants_of(rng, count, V, 0.3 if count < 5000 else 0.01)
    d = [K.upload(r) for r in res]
    for k, seed0 in enumerate(seed0s(count)):
        check(res, seed0, A.DIFF_ALL, RULES[k], count, ("seed0", count, seed0), d)
    lst = gappy(rng, count)
    d_lst = K.upload_seeds(lst)
    for rule in RULES:
        check(res, lst, A.DIFF_ALL, rule, count, ("list", count, rule), d, d_lst)
        check(res, lst, A.DIFF_STEPS, rule, 7, ("list cut", count, rule), d, d_lst)
    for fields in MASKS:
        check(res, 77, fields, R.DIFFERING if fields else R.FAILING, 7, ("mask", count, fields), d)


@pytest.mark.parametrize("V", VS)
def test_every_number_of_variants(hip, V):
    """V = 2, 3, 5, 8 at 4 097 seeds (five workgroups) under every rule; dense changes."""
    res = variants_of(np.random.default_rng([SEED, 40, V]), 4097, V, 0.5)
    d = [K.upload(r) for r in res]
    for rule in RULES:
        for fields in (A.DIFF_VERDICT, A.DIFF_ALL):
            check(res, (1 << 40) + 7, fields, rule, 4097, ("V", V, rule, fields), d)


def test_all_256_masks_and_wide_verdicts(hip):
    """V = 8: every fail mask 0 .. 255 populated; verdicts up to 2^32 - 1 in any variant."""
    rng = np.random.default_rng([SEED, 41])
    n = 4097
    masks = np.concatenate([np.arange(256), rng.integers(0, 256, n - 256)])
    res = []
    for v in range(8):
        fails = (masks >> v & 1).astype(bool)
        r = base_results(rng, n)
        r["verdict"][fails] = rng.integers(1, 4, int(fails.sum()))
        res.append(r)
    want = check(res, (1 << 64) - n, A.DIFF_VERDICT, R.MIXED, n, "256 masks")
    assert all(c > 0 for c in want["n_by_mask"]) and want["n_incomparable"] == 0
    assert want["n_selected"] == n - want["n_by_mask"][0] - want["n_by_mask"][255]
    vals = np.array([0, 1, 2, 3, 4, 5, 6, 7, 8, 255, 256, 257, 0x7fffffff, 0x80000000, 0xffffff00, 0xffffffff], dtype=np.uint32)
    for v in range(8):
        res[v]["verdict"] = rng.choice(vals, n, p=[0.5] + [0.5 / 15] * 15)
    for rule in RULES:
        want = check(res, 9, A.DIFF_ALL, rule, n, ("wide verdicts", rule))
        assert want["n_incomparable"] > 0 and want["n_settled"] > 0 and all(want["n_runner_by_variant"])


def test_a_runner_verdict_makes_the_seed_incomparable(hip):
    """A runner verdict in one variant while every other variant differs from variant 0 everywhere and fails: incomparable, never listed,
    counted in exactly its variants' n_runner_by_variant."""
    rng = np.random.default_rng([SEED, 42])
    n = 130
    for V in (2, 5):
        for at in (0, V - 1):
            res = [base_results(rng, n) for _ in range(V)]          # (independent draws: every field differs)
            for v in range(1, V):
                res[v]["verdict"] = A.PANIC
            res[at]["verdict"] = rng.choice(np.array([4, 5, 6, 7, 0xffffffff], dtype=np.uint32), n)
            for rule in RULES:
                want = check(res, 9, A.DIFF_ALL, rule, n, ("runner in", V, at, rule))
                assert (want["n_selected"], want["n_incomparable"], want["n_listed"], want["n_settled"]) == (0, n, 0, 0)
                assert want["n_runner_by_variant"] == [n if v == at else 0 for v in range(8)] and not any(want["n_differ_from_first"])
            res[at]["verdict"][64] = A.PASS if at == 0 else A.DEADLOCK      # one settled seed among them
            want = check(res, 9, A.DIFF_ALL, R.DIFFERING, n, ("one settled", V, at))
            assert want["n_selected"] == 1 and want["n_differ_from_first"] == [0] + [1] * (V - 1) + [0] * (8 - V)


@pytest.mark.parametrize("count", (65, 4097))
def test_one_seed_differs_in_one_field(hip, count):
    """Three equal variants except one seed in one field of variant 2, for each of the seven fields; the 64-bit ones once in bits 32-63 only
    and once in bit 0 only.  Under every single-bit mask, ALL and ALL & ~TRACE: only the masks that name the field see it."""
    rng = np.random.default_rng([SEED, count, 1])
    a = base_results(rng, count, rng.choice(np.arange(4, dtype=np.uint32), count))
    da = K.upload(a)
    at = count - 2
    flips = [("verdict", 1), ("steps", 1), ("steps", 1 << 31)] + [(name, x) for name in diff_ref.WIDE for x in (1, 0xffffffff << 32, 1 << 63)]
    for name, x in flips:
        b = a.copy()
        b[name][at] ^= b[name].dtype.type(x)
        if name == "verdict":
            b[name][at] &= 3                                        # (stays a reference verdict: the seed stays settled)
        db = K.upload(b)
        bit = 1 << R.FIELDS.index(name)
        for fields in MASKS[1:]:
            want = check([a, a, b], 1000, fields, R.DIFFERING, 4, (name, hex(x), fields), [da, da, db])
            assert want["n_selected"] == (1 if fields & bit else 0), (SEED, name, x, fields)
            assert want["n_differ_from_first"] == [0, 0, 1 if fields & bit else 0, 0, 0, 0, 0, 0]


def test_a_mask_that_leaves_later_bytes_unread(hip):
    """Only trace_hash and obs_hash differ (variant 1), only msg_count and rng_calls (variant 2), in every seed: a mask without a 16-byte
    part's fields does not see it, one with either does."""
    n = 1025
    a = base_results(np.random.default_rng([SEED, 2]), n)
    b, c = a.copy(), a.copy()
    b["trace_hash"] ^= np.uint64(1)
    b["obs_hash"] ^= np.uint64(1 << 63)
    c["msg_count"] ^= np.uint64(1 << 32)
    c["rng_calls"] ^= np.uint64(1)
    d = [K.upload(x) for x in (a, b, c)]
    for fields, want in ((A.DIFF_VERDICT | A.DIFF_STEPS | A.DIFF_CLOCK, [0, 0, 0]), (A.DIFF_MSGS, [0, 0, n]), (A.DIFF_OBS, [0, n, 0]),
                         (A.DIFF_RNG | A.DIFF_TRACE, [0, n, n]), (A.DIFF_ALL, [0, n, n])):
        got = check([a, b, c], 5, fields, R.DIFFERING, 8, ("unread", fields), d)
        assert got["n_differ_from_first"] == want + [0] * 5 and got["n_selected"] == (n if any(want) else 0)


def test_density_and_caps(hip):
    """No seed selected (wave counts all zero, n_by_mask[0] = count); every seed selected (4 097); selected seeds at positions 63, 64 and 65
    of a wave's piece and at the last index; caps 0, 1, 2, 63, 64, 65 and more than there are; a cap that ends inside a 64-seed round of a
    wave whose offset is not zero."""
    rng = np.random.default_rng([SEED, 5])
    n = 4097
    a = base_results(rng, n)
    da = K.upload(a)
    for rule in RULES:
        for cap in (0, 5):
            want = check([a, a, a], 3, A.DIFF_ALL, rule, cap, ("none", rule, cap), [da, da, da])
            assert want["n_selected"] == 0 and want["n_by_mask"][0] == n
            assert not any(R.wave_counts([a, a, a], A.DIFF_ALL, rule)[1])
    every = a.copy()
    every["verdict"] = A.DEADLOCK
    every["steps"] ^= np.uint32(1)
    de = K.upload(every)
    for cap in CAPS + (n, n + 10):
        for rule in RULES:
            assert check([a, every], (1 << 40) + 7, A.DIFF_ALL, rule, cap, ("every", rule, cap), [da, de])["n_selected"] == n
    piece, _ = R.wave_counts([a, a], 0, R.FAILING)
    assert piece == 256                                                                 # 4 097 seeds: 5 workgroups, 20 waves, ceil(4 097 / 20) rounded up to 64
    edges = a.copy()
    at = [63, 64, 65, piece + 63, piece + 64, piece + 65, 5 * piece + 63, 5 * piece + 64, 5 * piece + 65, n - 1]
    edges["verdict"][at] = A.TIME_LIMIT
    dg = K.upload(edges)
    for cap in CAPS + (len(at), len(at) + 1):
        want = check([a, a, edges, a], (1 << 64) - n, 0, R.MIXED, cap, ("edges", cap), [da, da, dg, da])
        assert want["n_selected"] == len(at) == want["n_by_mask"][4]
    # a list that ends inside a round: wave 1 (offset 100: wave 0 holds 100 selected seeds) has 40 in its second round, cap cuts them at 17
    inside = a.copy()
    inside["verdict"][np.arange(100)] = A.PANIC
    inside["verdict"][piece + 64 + np.arange(0, 60, 3)] = A.PANIC
    inside["verdict"][piece + 65 + np.arange(0, 60, 3)] = A.DEADLOCK
    di = K.upload(inside)
    _, waves = R.wave_counts([a, inside], 0, R.FAILING)
    assert waves[0] == 100 and waves[1] == 40 and sum(waves) == 140
    lst = gappy(rng, n)
    d_lst = K.upload_seeds(lst)
    for cap in (99, 100, 101, 117, 139, 140, 141):
        check([a, inside], 12345, 0, R.FAILING, cap, ("inside", cap), [da, di])
        check([a, inside], lst, A.DIFF_VERDICT, R.MIXED, cap, ("inside, list", cap), [da, di], d_lst)


@pytest.mark.parametrize("count", (1025, 4097))
def test_two_variants_agree_with_the_differential_truth(hip, count):
    """V = 2 under ALL / LIST_DIFFERING: the record seeds and n_differ_from_first[1] are diff_ref.diff_truth's records and n_differ of the pair."""
    a, b = diff_ref.synthetic(np.random.default_rng([SEED, count, 2]), count, 0.2)
    want = check([a, b], 5000, A.DIFF_ALL, R.DIFFERING, count, ("pair", count))
    t = diff_ref.diff_truth(a, b, 5000, diff_ref.ALL, count)
    recs = np.frombuffer(want["records"], dtype=A.SWEEP_RECORD_DTYPE)
    assert recs["seed"].tolist() == np.frombuffer(t["records"], dtype=A.DIFF_RECORD_DTYPE)["seed"].tolist() and t["n_differ"] > 0
    assert want["n_differ_from_first"][1] == t["n_differ"] == want["n_selected"] and want["n_incomparable"] == t["n_incomparable"]


def test_the_launcher_refuses_what_the_kernels_are_not_written_for(hip):
    """Nothing is launched for V outside 2 .. 8, a NULL side, no seeds, 2^32 seeds, a bit above ALL, an unknown rule, LIST_DIFFERING without
    fields, a list without an array, or the list form without a list."""
    import torch
    L = K._lib()
    a = base_results(np.random.default_rng([SEED, 6]), 64)
    d = [K.upload(a) for _ in range(9)]
    words = torch.zeros(8 * K.SWEEP_WORDS, dtype=torch.uint8, device="cuda")
    wcnt = torch.zeros(4 * K.WAVES, dtype=torch.uint8, device="cuda")
    table = K.side_table(d)
    holed = K.side_table(d[:3])
    holed[1] = None
    for sides, V, count, fields, rule, cap in ((table, 1, 64, 1, 0, 0), (table, 0, 64, 1, 0, 0), (table, 9, 64, 1, 0, 0), (None, 2, 64, 1, 0, 0),
                                               (holed, 3, 64, 1, 0, 0), (table, 2, 0, 1, 0, 0), (table, 2, 1 << 32, 1, 0, 0), (table, 2, 64, 128, 0, 0),
                                               (table, 2, 64, 1 << 31, 0, 0), (table, 2, 64, 1, 3, 0), (table, 2, 64, 0, 2, 0), (table, 2, 64, 1, 0, 4)):
        assert L.madsim_k_launch_sweep(sides, V, count, 0, fields, rule, words.data_ptr(), wcnt.data_ptr(), None, cap, None) == -1
    assert L.madsim_k_launch_sweep_list(table, 2, 64, None, 1, 0, words.data_ptr(), wcnt.data_ptr(), None, 0, None) == -1
    torch.cuda.synchronize()
    assert not bool(words.any()) and not bool(wcnt.any())
