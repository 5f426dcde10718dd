"""The differential campaign's report kernels (diff_count_kernel + diff_write_kernel, csrc/sim_kernel.hip) on SYNTHETIC result arrays,
launched directly (tests/diff_kernels.py): every word, every record byte and every wave count is held against tests/diff_ref.py, exactly.
Pairs the simulator rarely or never produces: a single field differing in its top half or in bit 0 only, verdicts up to 2^32 - 1 on
either side, all 64 transition cells at once, a runner verdict beside a side that differs everywhere, every seed differing, differing
seeds on both sides of a 64-seed round's edge, and a list that ends inside a round of a wave whose offset is not zero.
Every array comes from numpy.random.default_rng([SEED, ...]); SEED is in every assertion message."""
import numpy as np
import pytest

from madsim_amd import _abi as A
from tests import diff_kernels as K
from tests import diff_ref as R

pytestmark = pytest.mark.gpu

SEED = 20261018
U64_MAX = (1 << 64) - 1
COUNTS = (1, 63, 64, 65, 1023, 1024, 1025, 4097, 262_209)          # the last: 256 workgroups (the grid cap) and a ragged last piece
CAPS = (0, 1, 2, 63, 64, 65)
MASKS = tuple(1 << i for i in range(7)) + (A.DIFF_ALL, A.DIFF_ALL & ~A.DIFF_TRACE)


def seed0s(count):
    return (0, (1 << 40) + 7, (1 << 64) - count)                    # the last: the batch ends with seed 2^64 - 1


def equal_sides(rng, n, verdict=A.PASS):
    """Two equal sides of n results: `verdict` (a value or an array), every other field random."""
    a = np.zeros(n, dtype=A.RESULT_DTYPE)
    a["verdict"] = verdict
    a["steps"] = rng.integers(0, 1 << 32, n, dtype=np.uint64)
    for name in R.WIDE:
        a[name] = rng.integers(0, 1 << 64, n, dtype=np.uint64)
    return a, a.copy()


def check(a, b, seed0, fields, cap, what, d=None):
    """One launch against the truth; returns the truth."""
    da, db = d if d is not None else (K.upload(a), K.upload(b))
    words, waves, recs = K.diff(da, db, len(a), seed0, fields, cap)
    want = R.diff_truth(a, b, seed0, fields, min(cap, len(a)))
    piece, want_waves = R.wave_counts(a, b, fields)
    print(what, "differ", int(words[0]), "want", want["n_differ"], "incomparable", int(words[1]), "listed", len(recs))
    assert words.tolist() == R.words_of(a, b, fields).tolist(), (SEED, what, words[:10].tolist(), R.words_of(a, b, fields)[:10].tolist())
    assert waves.tolist() == want_waves, (SEED, what, piece)
    assert len(recs) == want["n_listed"] and recs.tobytes() == want["records"], (SEED, what, recs["seed"][:4], len(recs), want["n_listed"])
    assert int(words[10:].sum()) == len(a)
    return want


@pytest.mark.parametrize("count", COUNTS)
def test_counts_seeds_and_masks(hip, count):
    """Random pairs at every count: every seed0, every mask, a cap that takes everything and one that does not."""
    a, b = R.synthetic(np.random.default_rng([SEED, count]), count, p_differ=0.3 if count < 5000 else 0.01)
    d = (K.upload(a), K.upload(b))
    for seed0 in seed0s(count):
        check(a, b, seed0, A.DIFF_ALL, count, ("seed0", count, seed0), d)
    for fields in MASKS:
        check(a, b, 77, fields, 7, ("mask", count, fields), d)


@pytest.mark.parametrize("count", (65, 4097))
def test_one_seed_differs_in_one_field(hip, count):
    """Both sides equal except one seed in one field, for each of the seven fields; the 64-bit ones once in bits 32-63 only and once in bit 0
    only.  Under every single-bit mask, ALL and ALL & ~TRACE: only the masks that name the field see it."""
    rng = np.random.default_rng([SEED, count, 1])
    a, b0 = equal_sides(rng, count, rng.choice(np.arange(4, dtype=np.uint32), count))
    da = K.upload(a)
    at = count - 2
    flips = [("verdict", 1), ("steps", 1), ("steps", 1 << 31)] + [(name, x) for name in R.WIDE for x in (1, 0xffffffff << 32, 1 << 63)]
    for name, x in flips:
        b = b0.copy()
        b[name][at] ^= b[name].dtype.type(x)
        if name == "verdict":
            b[name][at] &= 3                                        # (stays a reference verdict: the seed stays compared)
        db = K.upload(b)
        bit = 1 << R.FIELDS.index(name)
        for fields in MASKS:
            want = check(a, b, 1000, fields, 4, (name, hex(x), fields), (da, db))
            assert want["n_differ"] == (1 if fields & bit else 0), (SEED, name, x, fields)
            assert want["n_by_field"] == [1 if (fields & bit and 1 << i == bit) else 0 for i in range(8)]


def test_a_mask_that_leaves_the_third_16_bytes_unread(hip):
    """Only trace_hash and obs_hash differ, in every seed: a mask without them reports no difference, one with either reports every seed."""
    n = 1025
    a, b = equal_sides(np.random.default_rng([SEED, 2]), n)
    b["trace_hash"] ^= np.uint64(1)
    b["obs_hash"] ^= np.uint64(1 << 63)
    d = (K.upload(a), K.upload(b))
    for fields in (A.DIFF_VERDICT | A.DIFF_STEPS | A.DIFF_CLOCK, A.DIFF_ALL & ~(A.DIFF_TRACE | A.DIFF_OBS), A.DIFF_MSGS):
        assert check(a, b, 5, fields, 8, ("unread", fields), d)["n_differ"] == 0
    assert check(a, b, 5, A.DIFF_OBS, 8, "obs", d)["n_differ"] == n
    assert check(a, b, 5, A.DIFF_ALL, 8, "all", d)["n_by_field"] == [0, 0, 0, 0, 0, n, n, 0]
    # ... and the same for the second 16 bytes
    a, b = equal_sides(np.random.default_rng([SEED, 3]), n)
    b["msg_count"] ^= np.uint64(1 << 32)
    b["rng_calls"] ^= np.uint64(1)
    d = (K.upload(a), K.upload(b))
    assert check(a, b, 5, A.DIFF_ALL & ~(A.DIFF_MSGS | A.DIFF_RNG), 8, "second unread", d)["n_differ"] == 0
    assert check(a, b, 5, A.DIFF_RNG | A.DIFF_OBS, 8, "rng", d)["n_by_field"] == [0, 0, 0, 0, n, 0, 0, 0]


def test_verdicts_and_transition_cells(hip):
    """Verdicts up to 2^32 - 1 on either side; every one of the 64 cells populated; a runner verdict on one side with every other field
    different: incomparable, not listed, counted in its cell."""
    rng = np.random.default_rng([SEED, 4])
    vals = np.array([0, 1, 2, 3, 4, 5, 6, 7, 8, 0x7fffffff, 0x80000000, 0xffffffff], dtype=np.uint32)
    n = 4097
    a, b = equal_sides(rng, n, rng.choice(vals, n))
    b["verdict"] = rng.choice(vals, n)
    a["verdict"][:64], b["verdict"][:64] = np.repeat(np.arange(8), 8), np.tile(np.arange(8), 8)      # every cell at least once
    want = check(a, b, (1 << 64) - n, A.DIFF_ALL, n, "cells")
    assert all(c > 0 for row in want["transitions"] for c in row)
    assert want["n_incomparable"] > 0 and want["n_compared"] > 0
    # a runner verdict on one side, every other field different: never a difference
    a, b = equal_sides(rng, 130)
    for name in R.FIELDS[1:]:
        b[name] ^= b[name].dtype.type(1)
    b["verdict"] = rng.choice(np.array([4, 5, 6, 7, 0xffffffff], dtype=np.uint32), 130)
    want = check(a, b, 9, A.DIFF_ALL, 130, "runner on B")
    assert (want["n_differ"], want["n_incomparable"], want["n_listed"]) == (0, 130, 0) and sum(want["transitions"][0][4:]) == 130
    want = check(b, a, 9, A.DIFF_ALL, 130, "runner on A")
    assert (want["n_differ"], want["n_incomparable"]) == (0, 130) and sum(row[0] for row in want["transitions"][4:]) == 130
    b["verdict"][64] = A.PANIC                                       # one compared seed among them
    assert check(a, b, 9, A.DIFF_ALL, 130, "one compared")["n_by_field"] == [1, 1, 1, 1, 1, 1, 1, 0]


def test_density_and_caps(hip):
    """No seed differs; every seed differs (4 097); differing seeds at positions 63, 64 and 65 of a wave's piece and at the last index; caps 0,
    1, 2, 63, 64, 65 and more than there are; a cap that ends inside a 64-seed round of a wave whose offset is not zero."""
    rng = np.random.default_rng([SEED, 5])
    n = 4097
    a, b = equal_sides(rng, n, rng.choice(np.arange(4, dtype=np.uint32), n))
    d = (K.upload(a), K.upload(b))
    for cap in (0, 5):
        assert check(a, b, 3, A.DIFF_ALL, cap, ("none", cap), d)["n_differ"] == 0
    every = b.copy()
    every["steps"] ^= np.uint32(1)
    de = (d[0], K.upload(every))
    for cap in CAPS + (n, n + 10):
        assert check(a, every, (1 << 40) + 7, A.DIFF_ALL, cap, ("every", cap), de)["n_differ"] == n
    piece, _ = R.wave_counts(a, b, A.DIFF_ALL)
    assert piece == 256                                                                 # 4 097 seeds: 5 workgroups, 20 waves, ceil(4 097 / 20) rounded up to 64
    edges = b.copy()
    at = [63, 64, 65, piece + 63, piece + 64, piece + 65, 5 * piece + 63, 5 * piece + 64, 5 * piece + 65, n - 1]
    edges["clock_ns"][at] ^= np.uint64(1 << 40)
    dg = (d[0], K.upload(edges))
    for cap in CAPS + (len(at), len(at) + 1):
        want = check(a, edges, (1 << 64) - n, A.DIFF_CLOCK, cap, ("edges", cap), dg)
        assert want["n_differ"] == len(at)
    # a list that ends inside a round: wave 1 (offset 100: wave 0 holds 100 differing seeds) has 40 in its second round, cap cuts them at 17
    inside = b.copy()
    inside["obs_hash"][np.arange(100)] ^= np.uint64(1)
    inside["obs_hash"][piece + 64 + np.arange(0, 60, 3)] ^= np.uint64(1)
    inside["obs_hash"][piece + 65 + np.arange(0, 60, 3)] ^= np.uint64(2)
    di = (d[0], K.upload(inside))
    _, waves = R.wave_counts(a, inside, A.DIFF_OBS)
    assert waves[0] == 100 and waves[1] == 40 and sum(waves) == 140
    for cap in (99, 100, 101, 117, 139, 140, 141):
        check(a, inside, 12345, A.DIFF_OBS, cap, ("inside", cap), di)


def test_the_launcher_refuses_what_the_kernels_are_not_written_for(hip):
    """Nothing is launched for an empty mask, a bit above ALL, no seeds, 2^32 seeds or a list without an array."""
    import torch
    L = K._lib()
    a, b = equal_sides(np.random.default_rng([SEED, 6]), 64)
    da, db = K.upload(a), K.upload(b)
    words = torch.zeros(8 * K.DIFF_WORDS, dtype=torch.uint8, device="cuda")
    wcnt = torch.zeros(4 * K.WAVES, dtype=torch.uint8, device="cuda")
    for count, fields, cap in ((64, 0, 0), (64, 128, 0), (64, 1 << 31, 0), (0, 127, 0), (1 << 32, 127, 0), (64, 127, 4)):
        assert L.madsim_k_launch_diff(da.data_ptr(), db.data_ptr(), count, 0, fields, words.data_ptr(), wcnt.data_ptr(), None, cap, None) == -1
    torch.cuda.synchronize()
    assert not bool(words.any()) and not bool(wcnt.any())
