"""The paired campaign's report kernels (paired_fold_kernel + paired_top_kernel, csrc/sim_kernel.hip) on SYNTHETIC result arrays, launched
directly (tests/paired_kernels.py): every report word and every top record is held against tests/paired_ref.py, exactly.
Pairs the simulator rarely or never produces: magnitudes of 2^64 - 1 in both directions and on both edges of every bucket, sums whose high
halves carry, steps at 2^32 - 1, populations that are all equal / all up / all down, a seed that is up in one metric and down in another,
verdicts up to 2^32 - 1, a runner verdict beside a side that differs everywhere, every pair of include masks, and ties at rank K across a
64-seed round, a wave's piece and a workgroup.
Every array comes from numpy.random.default_rng([SEED, ...]); SEED is in every assertion message."""
import numpy as np
import pytest

from madsim_amd import _abi as A
from tests import paired_kernels as K
from tests import paired_ref as R
from tests import stats_ref

pytestmark = pytest.mark.gpu

SEED = 20261019
U64_MAX = (1 << 64) - 1
COUNTS = (1, 63, 64, 65, 1023, 1024, 1025, 4097, 262_209)          # the last: 256 workgroups (the grid cap) and a ragged last piece
TOPS = (0, 1, 2, 15, 16)
INCLUDES = (1, 2, 6, 15)
WIDE = ("clock_ns", "msg_count", "rng_calls")


def seed0s(count):
    return (0, (1 << 40) + 7, (1 << 64) - count)                    # the last: the batch ends with seed 2^64 - 1


def passing(n, value=1000):
    """Two equal sides of n passing results with every metric `value`."""
    a = np.zeros(n, dtype=A.RESULT_DTYPE)
    for name in R.METRICS:
        a[name] = value
    return a, a.copy()


def random_pairs(rng, n, p_verdict=0.1, p_equal=0.3, bits=64):
    """Side B is side A with metrics moved either way; some verdicts changed on either side, runner verdicts and huge ones among them."""
    a = np.zeros(n, dtype=A.RESULT_DTYPE)
    for name in WIDE + ("trace_hash", "obs_hash"):
        a[name] = rng.integers(0, 1 << bits, n, dtype=np.uint64)
    a["steps"] = rng.integers(0, 1 << 32, n, dtype=np.uint64)
    b = a.copy()
    for name in WIDE:
        move = rng.random(n) >= p_equal
        b[name][move] = rng.integers(0, 1 << bits, int(move.sum()), dtype=np.uint64)
    move = rng.random(n) >= p_equal
    b["steps"][move] = rng.integers(0, 1 << 32, int(move.sum()), dtype=np.uint64)
    for side in (a, b):
        ch = rng.random(n) < p_verdict
        side["verdict"][ch] = rng.choice(np.array([1, 2, 3, 4, 5, 6, 7, 9, 0x80000000, 0xffffffff], dtype=np.uint32), int(ch.sum()))
    return a, b


def check(a, b, seeds, inc_a, inc_b, k, what, d=None):
    """One launch against the truth, word for word; returns the truth.  `seeds`: seed0, or a uint64 array (the list form)."""
    da, db = d if d is not None else (K.upload(a), K.upload(b))
    got = K.paired(da, db, len(a), K.upload_seeds(seeds) if isinstance(seeds, np.ndarray) else seeds, inc_a, inc_b, k)
    want = R.paired_truth(a, b, seeds, inc_a, inc_b, k)
    words = R.words_of(want, k)
    print(what, "paired", int(got[0]), "want", want["n_paired"], "incomparable", int(got[1]), "n", got[2:10].tolist())
    bad = np.nonzero(got != words)[0]
    assert len(bad) == 0, (SEED, what, bad[:8].tolist(), got[bad[:8]].tolist(), words[bad[:8]].tolist(),
                           R.differences(R.of_words(got, len(a), k), want))
    assert want["n_paired"] + want["n_unpaired"] + want["n_incomparable"] == len(a)
    return want


@pytest.mark.parametrize("count", COUNTS)
def test_counts_seeds_and_tops(hip, count):
    """Random pairs at every count: every seed0, the list form with seeds up to 2^64 - 1, every K."""
    rng = np.random.default_rng([SEED, count])
    a, b = random_pairs(rng, count, p_verdict=0.1 if count < 5000 else 0.01)
    d = (K.upload(a), K.upload(b))
    for seed0 in seed0s(count) if count < 5000 else seed0s(count)[2:]:      # (the largest count: one range launch, the truth is what takes the time)
        check(a, b, seed0, 1, 1, 16, ("seed0", count, seed0), d)
    lst = np.unique(rng.integers(0, 1 << 64, 2 * count + 8, dtype=np.uint64))[:count].copy()
    lst[-1] = U64_MAX
    assert len(lst) == count and (count == 1 or lst[-2] < lst[-1])
    for k in TOPS if count < 5000 else (0, 16):
        check(a, b, lst, 15, 15, k, ("list", count, k), d)
    if count < 5000:
        check(a, b, 77, 1, 15, 2, ("mixed include", count), d)


def test_every_pair_of_include_masks(hip):
    a, b = random_pairs(np.random.default_rng([SEED, 1]), 3000, p_verdict=0.5)
    d = (K.upload(a), K.upload(b))
    seen = set()
    for inc_a in INCLUDES:
        for inc_b in INCLUDES:
            t = check(a, b, 5, inc_a, inc_b, 3, ("include", inc_a, inc_b), d)
            seen.add(t["n_paired"])
    assert len(seen) > 8                                             # the masks do select different populations


def test_magnitude_edges(hip):
    """a = 0 against b = 2^64 - 1 and the reverse; magnitudes on both edges of every bucket 1 .. 251; steps at 2^32 - 1."""
    edges = sorted({stats_ref.bucket_floor(bk) for bk in range(1, 252)} | {stats_ref.bucket_floor(bk + 1) - 1 for bk in range(1, 251)} | {U64_MAX})
    n = 2 * len(edges) + 2
    a, b = passing(n, 0)
    for i, mag in enumerate(edges):
        base = (U64_MAX - mag) // 3
        a["clock_ns"][2 * i], b["clock_ns"][2 * i] = base, base + mag                    # up by mag
        a["rng_calls"][2 * i + 1], b["rng_calls"][2 * i + 1] = mag, 0                    # down by mag
        a["msg_count"][2 * i], b["msg_count"][2 * i + 1] = mag, mag                      # one down, one up
    a["clock_ns"][n - 2], b["clock_ns"][n - 2] = 0, U64_MAX
    a["clock_ns"][n - 1], b["clock_ns"][n - 1] = U64_MAX, 0
    a["steps"][n - 2], b["steps"][n - 1] = 0xffffffff, 0xffffffff                         # steps: down by 2^32 - 1, up by 2^32 - 1
    for k in (0, 16):
        t = check(a, b, (1 << 64) - n, 1, 1, k, ("edges", k))
        up = t["clock_ns"]["dir"][R.UP]
        assert up["max"] == U64_MAX and up["min"] == 1 and all(int(up["hist"][bk]) >= 1 for bk in range(1, 252)) and int(up["hist"][0]) == 0
        assert t["steps"]["dir"][R.UP]["max"] == t["steps"]["dir"][R.DOWN]["max"] == 0xffffffff
        assert t["clock_ns"]["dir"][R.DOWN]["top"][:1] == ([((1 << 64) - 1, U64_MAX, 0)] if k else [])


def test_sums_carry_into_the_high_words(hip):
    """High halves set in enough seeds that the 128-bit sums need their high word: 70 000 magnitudes of about 2^63."""
    n = 70_000
    rng = np.random.default_rng([SEED, 2])
    a, b = passing(n, 0)
    for name in WIDE:
        b[name] = rng.integers(1 << 63, 1 << 64, n, dtype=np.uint64)
    a["msg_count"], b["msg_count"] = b["msg_count"].copy(), 0                              # ... and the same downwards
    t = check(a, b, 0, 1, 1, 4, "carry")
    assert t["clock_ns"]["dir"][R.UP]["sum"] >> 64 != 0 and t["msg_count"]["dir"][R.DOWN]["sum"] >> 64 != 0
    assert t["clock_ns"]["sum_b"] >> 64 != 0 and t["msg_count"]["sum_a"] >> 64 != 0 and t["clock_ns"]["sum_a"] == 0


@pytest.mark.parametrize("population", ["equal", "up", "down", "mixed"])
def test_extreme_populations(hip, population):
    n = 5000
    rng = np.random.default_rng([SEED, 3])
    a, b = passing(n, 1 << 20)
    delta = rng.integers(1, 1 << 19, n, dtype=np.uint64)
    for name in R.METRICS:
        if population == "up" or (population == "mixed" and name in ("clock_ns", "steps")):
            b[name] += delta.astype(b[name].dtype)
        elif population in ("down", "mixed"):
            b[name] -= delta.astype(b[name].dtype)
    t = check(a, b, 9, 1, 1, 16, population)
    for m, name in enumerate(R.METRICS):
        want_up = n if population == "up" or (population == "mixed" and m < 2) else 0
        want_down = 0 if population == "equal" else n - want_up
        assert (t[name]["dir"][R.UP]["n"], t[name]["dir"][R.DOWN]["n"], t[name]["n_equal"]) == (want_up, want_down, n - want_up - want_down)
    if population == "mixed":                                        # one seed that is up in one metric and down in another: every seed here
        assert t["clock_ns"]["dir"][R.UP]["top"][0][0] == t["rng_calls"]["dir"][R.DOWN]["top"][0][0]


def test_verdicts(hip):
    """Verdicts up to 2^32 - 1 on either side; a runner verdict on one side with every metric different is never paired; a genuine failure
    pairs only under a mask that names it."""
    n = 640
    rng = np.random.default_rng([SEED, 4])
    a, b = random_pairs(rng, n, p_verdict=0.0, p_equal=0.0)
    a["verdict"][0::7] = rng.choice(np.array([4, 5, 6, 7, 8, 255, 256, 0x7fffffff, 0x80000000, 0xffffffff], dtype=np.uint32), len(a[0::7]))
    b["verdict"][3::7] = rng.choice(np.array([4, 5, 6, 7, 8, 255, 256, 0x7fffffff, 0x80000000, 0xffffffff], dtype=np.uint32), len(b[3::7]))
    a["verdict"][1::7], b["verdict"][2::7] = A.DEADLOCK, A.PANIC
    n_inc = len(a[0::7]) + len(b[3::7])
    for inc_a, inc_b, want_paired in ((15, 15, n - n_inc), (1, 1, n - n_inc - len(a[1::7]) - len(b[2::7])), (1 << A.DEADLOCK, 1, len(a[1::7]))):
        t = check(a, b, 1 << 63, inc_a, inc_b, 16, ("verdicts", inc_a, inc_b))
        assert (t["n_paired"], t["n_incomparable"]) == (want_paired, n_inc)
    # every seed incomparable: nothing but the one count
    a["verdict"] = A.OVERFLOW
    t = check(a, b, 0, 15, 15, 16, "all incomparable")
    assert (t["n_paired"], t["n_incomparable"], t["n_unpaired"]) == (0, n, 0)
    # nothing paired, nothing incomparable
    a["verdict"], b["verdict"] = A.PANIC, A.PASS
    assert check(a, b, 0, 1, 1, 16, "all unpaired")["n_unpaired"] == n


@pytest.mark.parametrize("k", TOPS)
def test_ties_at_rank_k(hip, k):
    """Equal magnitudes everywhere in clock_ns (up) and rng_calls (down): the K smallest seeds win.  Then the tie group placed across a 64-seed
    round's edge, a wave's piece and a workgroup, with larger magnitudes before and after it; and fewer paired seeds than K."""
    n = 9000                                                         # 9 workgroups; a wave's piece is 256 seeds
    a, b = passing(n)
    b["clock_ns"] += np.uint64(5)
    b["rng_calls"] -= np.uint64(5)
    t = check(a, b, 100, 1, 1, k, ("all tied", k))
    assert [e[0] for e in t["clock_ns"]["dir"][R.UP]["top"]] == [100 + i for i in range(k)]
    for at in (63, 255, 1023, 1024 + 255, 8 * 1024 - 3):             # a round's edge, a piece's edge, a workgroup's edge ...
        a, b = passing(n)
        tied = np.arange(at - 5, at + 12)
        b["clock_ns"][tied] += np.uint64(700)
        a["steps"][tied] += np.uint32(700)
        b["clock_ns"][[3, n - 2]] += np.uint64(900)                  # ... between two larger ones at the batch's ends
        a["steps"][[3, n - 2]] += np.uint32(900)
        b["clock_ns"][at + 40] += np.uint64(10)
        t = check(a, b, (1 << 64) - n, 1, 1, k, ("tie at", at, k))
        first = [(1 << 64) - n + i for i in [3, n - 2] + tied.tolist()]
        assert [e[0] for e in t["clock_ns"]["dir"][R.UP]["top"]] == first[:k]
        assert [e[0] for e in t["steps"]["dir"][R.DOWN]["top"]] == first[:k]
    # fewer paired seeds than K: three up, one down, the rest failing on side B
    a, b = passing(300)
    b["verdict"] = A.DEADLOCK
    b["verdict"][[7, 100, 299, 150]] = A.PASS
    b["msg_count"][[7, 100, 299]] += np.uint64(1)
    b["msg_count"][150] -= np.uint64(1)
    t = check(a, b, 0, 1, 1, k, ("few", k))
    assert len(t["msg_count"]["dir"][R.UP]["top"]) == min(k, 3) and len(t["msg_count"]["dir"][R.DOWN]["top"]) == min(k, 1) and t["n_paired"] == 4


def test_the_launcher_refuses_what_the_kernels_are_not_written_for(hip):
    a, b = passing(64)
    d = (K.upload(a), K.upload(b))
    for kw in (dict(count=0), dict(count=1 << 32), dict(include_a=0), dict(include_a=16), dict(include_b=0), dict(include_b=1 << 31), dict(top_k=17),
               dict(top_k=1, with_cand=False)):
        args = dict(count=64, include_a=1, include_b=1, top_k=0)
        args.update(kw)
        assert K.refused(*d, **args) == -1, kw
