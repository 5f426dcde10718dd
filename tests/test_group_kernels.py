"""The grouping campaign's report kernels (group_fold_kernel + group_extract_kernel, csrc/sim_kernel.hip) on SYNTHETIC result arrays,
launched directly (tests/group_kernels.py) and held against tests/groups_ref.py — exactly, after sorting by first_seed: arrival order
places the entries on the device and is no part of the answer.  Signatures the simulator rarely or never produces: keys 0, 2^64 - 1 and
the FNV offset basis, one key under four verdicts, keys that all start probing at one slot, a probe run that wraps around the table's
end, a table at its designed load of 0.5, runner verdicts and a verdict of 2^32 - 1 among the counted ones.
Every array comes from numpy.random.default_rng([SEED, ...]); SEED is in every assertion message."""
import numpy as np
import pytest

from madsim_amd import _abi as A
from tests import group_kernels as K
from tests import groups_ref as G

pytestmark = pytest.mark.gpu

SEED = 20261018
U64_MAX = (1 << 64) - 1
COUNTS = (1, 63, 64, 65, 1025, 4097, 65_536)
RUNNER = np.array([4, 5, 6, 7, 0xffffffff], dtype=np.uint32)


def seed0s(count):
    return (0, (1 << 40) + 7, (1 << 64) - count)                    # the last: the batch ends with seed 2^64 - 1


def blank(rng, n, verdict=A.DEADLOCK):
    """n results with `verdict`, every 64-bit field random and distinct-ish, steps random."""
    r = np.zeros(n, dtype=A.RESULT_DTYPE)
    r["verdict"] = verdict
    for name in G.KEY_FIELDS[:5]:
        r[name] = rng.integers(0, 1 << 64, n, dtype=np.uint64)
    r["steps"] = rng.integers(0, 1 << 32, n, dtype=np.uint64)
    return r


def mixed(rng, n, n_keys):
    """Verdicts 0-3 and the runner verdicts; every key field from a pool of n_keys values that holds 0, 2^64 - 1 and the FNV basis."""
    r = blank(rng, n, rng.choice(np.concatenate([np.arange(4, dtype=np.uint32), RUNNER]), n))
    pool = np.concatenate([np.array([0, U64_MAX, G.FNV_BASIS], dtype=np.uint64), rng.integers(0, 1 << 64, max(n_keys - 3, 0), dtype=np.uint64)])[:max(n_keys, 1)]
    for name in G.KEY_FIELDS[:5]:
        r[name] = rng.choice(pool, n)
    r["steps"] = rng.choice(pool & np.uint64(0xffffffff), n)
    return r


def check(results, seed0, include, key_field, what, d=None, slots=None):
    """One launch against the truth; returns the sorted entries."""
    d = K.upload(results) if d is None else d
    n, entries, _ = K.groups(d, len(results), seed0, include, key_field, slots)
    got, want = K.by_first_seed(entries), G.all_groups(results, seed0, include, key_field)
    print(what, "groups", n, "want", len(want), "first", got[:2], want[:2])
    assert n == len(want), (SEED, what, n, len(want))
    assert got == want, (SEED, what, [x for x in zip(got, want) if x[0] != x[1]][:4])
    assert sum(g[2] for g in got) == int(G.counted(results, include).sum())
    return got


@pytest.mark.parametrize("count", COUNTS)
def test_counts_seeds_keys_and_masks(hip, count):
    """Few groups, some, and nearly one per seed, at every count; every seed0; every key field; include masks of one bit and of all four."""
    for case, n_keys in enumerate((1, 5, 200, 1 << 20)):
        results = mixed(np.random.default_rng([SEED, count, case]), count, n_keys)
        d = K.upload(results)
        for seed0 in seed0s(count):
            check(results, seed0, G.ALL, A.GROUP_KEY_OBS, ("mixed", count, n_keys, seed0), d)
        if case == 1 or count == 4097:
            for include in (1, 2, 4, 8, G.FAILURES):
                check(results, 7, include, A.GROUP_KEY_OBS, ("mask", count, n_keys, include), d)
            for key_field in range(1, A.GROUP_KEYS):
                check(results, 7, G.ALL, key_field, ("field", count, n_keys, key_field), d)


def test_one_group_at_65536(hip):
    """The contention path: every wave adds its 64 seeds to one slot."""
    results = blank(np.random.default_rng([SEED, 1]), 65_536)
    results["obs_hash"] = G.FNV_BASIS
    got = check(results, (1 << 40) + 7, G.FAILURES, A.GROUP_KEY_OBS, "one group")
    assert got == [(A.DEADLOCK, G.FNV_BASIS, 65_536, (1 << 40) + 7)]


def test_every_seed_its_own_group_twice(hip):
    """65 536 groups in 131 072 slots: the table at its designed load of 0.5.  Twice in one process: the same sorted entries."""
    results = blank(np.random.default_rng([SEED, 2]), 65_536)
    results["obs_hash"] = np.random.default_rng([SEED, 3]).permutation(65_536).astype(np.uint64) * np.uint64(0x9E3779B97F4A7C15)
    assert K.slots_for(65_536) == 131_072
    d = K.upload(results)
    first = check(results, 0, G.FAILURES, A.GROUP_KEY_OBS, "all distinct", d)
    assert len(first) == 65_536 and all(g[2] == 1 for g in first)
    assert check(results, 0, G.FAILURES, A.GROUP_KEY_OBS, "all distinct, again", d) == first


def test_two_groups_interleaved_lane_by_lane(hip):
    for count in (64, 65, 4097):
        results = blank(np.random.default_rng([SEED, 4, count]), count)
        results["obs_hash"] = np.where(np.arange(count) % 2 == 0, 0, U64_MAX).astype(np.uint64)
        got = check(results, 100, G.FAILURES, A.GROUP_KEY_OBS, ("interleaved", count))
        assert got == [(A.DEADLOCK, 0, (count + 1) // 2, 100), (A.DEADLOCK, U64_MAX, count // 2, 101)]


def test_one_member_per_wave_across_all_workgroups(hip):
    """65 536 seeds are 1 024 waves of 64: a group with one member in each wave, at a random lane, among seeds that are their own groups.
    Its first_seed is the global minimum — the member of wave 0 — whichever wave's atomic arrives first."""
    rng = np.random.default_rng([SEED, 5])
    results = blank(rng, 65_536)
    members = np.arange(1024) * 64 + rng.integers(0, 64, 1024)
    results["obs_hash"][members] = 0x1234
    got = check(results, 9, G.FAILURES, A.GROUP_KEY_OBS, "one per wave")
    mine = [g for g in got if g[1] == 0x1234]
    assert mine == [(A.DEADLOCK, 0x1234, 1024, 9 + int(members[0]))] and len(got) == 65_536 - 1023


def test_edge_keys_and_one_key_under_four_verdicts(hip):
    n = 4097
    rng = np.random.default_rng([SEED, 6])
    results = blank(rng, n, rng.integers(0, 4, n).astype(np.uint32))
    results["obs_hash"] = rng.choice(np.array([0, U64_MAX, G.FNV_BASIS], dtype=np.uint64), n)
    got = check(results, (1 << 64) - n, G.ALL, A.GROUP_KEY_OBS, "edge keys")
    assert {(g[0], g[1]) for g in got} == {(v, k) for v in range(4) for k in (0, U64_MAX, G.FNV_BASIS)}      # twelve groups: equal keys, different verdicts
    results["obs_hash"] = 77
    assert [(g[0], g[1]) for g in sorted(check(results, 0, G.ALL, A.GROUP_KEY_OBS, "one key"))] == [(v, 77) for v in range(4)]


def colliding_keys(verdict, slots, at, n, rng):
    """n distinct keys whose signature (key, verdict) starts probing at slot `at` of `slots`."""
    keys = []
    while len(keys) < n:
        for k in rng.integers(0, 1 << 64, 4096, dtype=np.uint64):
            if K.slot_of(int(k), verdict, slots) == at and int(k) not in keys:
                keys.append(int(k))
                if len(keys) == n:
                    break
    return keys


@pytest.mark.parametrize("at", ["middle", "last"])
def test_keys_that_start_at_one_slot(hip, at):
    """96 keys that all start probing at one slot of a 256-slot table — in its middle, and at its LAST slot, where the run wraps to slot 0 —,
    one seed each plus 32 repeats: every insertion but the first walks the run the earlier ones left."""
    count, slots = 128, 256
    assert K.slots_for(count) == slots
    start = slots - 1 if at == "last" else 100
    rng = np.random.default_rng([SEED, 7, start])
    keys = colliding_keys(A.DEADLOCK, slots, start, 96, rng)
    assert len(set(keys)) == 96 and all(K.slot_of(k, A.DEADLOCK, slots) == start for k in keys)
    results = blank(rng, count)
    results["obs_hash"] = np.array(keys + keys[:32], dtype=np.uint64)[rng.permutation(count)]
    d = K.upload(results)
    got = check(results, 5, G.FAILURES, A.GROUP_KEY_OBS, ("collide", at), d)
    assert len(got) == 96 and sorted(g[2] for g in got) == [1] * 64 + [2] * 32
    _, _, claimed = K.groups(d, count, 5, G.FAILURES, A.GROUP_KEY_OBS)
    assert sorted(claimed.tolist()) == sorted((start + j) % slots for j in range(96))       # one contiguous run from the start slot, wrapping at the end


def test_runner_verdicts_are_never_grouped(hip):
    n = 1025
    rng = np.random.default_rng([SEED, 8])
    results = blank(rng, n, rng.choice(RUNNER, n))
    results["obs_hash"] = 1
    d = K.upload(results)
    for include in (1, 2, 4, 8, 15):
        count, entries, _ = K.groups(d, n, 0, include, A.GROUP_KEY_OBS)        # nothing counted: no group, no entry written, the table untouched
        assert count == 0 and len(entries) == 0, (SEED, include)
    results["verdict"][::100] = A.PANIC
    got = check(results, 0, G.ALL, A.GROUP_KEY_OBS, "runner verdicts present")
    assert got == [(A.PANIC, 1, 11, 0)]


def test_nothing_counted(hip):
    """A passing batch under include = failures: group count 0; the helper holds the entry buffer, the list and the table untouched."""
    for count in (1, 64, 65_536):
        results = blank(np.random.default_rng([SEED, 9, count]), count, A.PASS)
        n, entries, claimed = K.groups(K.upload(results), count, 3, G.FAILURES, A.GROUP_KEY_OBS)
        assert (n, len(entries), len(claimed)) == (0, 0, 0), (SEED, count)
