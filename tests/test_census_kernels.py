"""census_fold_kernel / census_extract_kernel (csrc/sim_kernel.hip) on SYNTHETIC rows, launched directly (tests/census_kernels.py): every
entry and every count word is held against tests/census_ref.py, exactly.  Rows the simulator rarely or never produces: lengths 0, below,
at and above obs_cap with random NON-ZERO words behind min(len, obs_cap) (a kernel that reads behind a row's end reports values that are
not there); a value repeated inside a round of 64, across the rounds of one row (index 0, 64, 128, ...), across the rows one wave walks,
across waves and workgroups; rows of all-distinct values; the values 0, 2^64 - 1 and the FNV offset basis; values built to start probing
at one slot; a table at exactly `cap` values and one at cap + 1; every verdict 0 .. 7 and 2^32 - 1 under several include masks.
Every case runs in both forms of the fold kernel: the wave accumulator in LDS (rows up to its fill limit of 192 visible observations) and
the direct form (which the longer rows take in either case).  In the cases above a wave walks one row, or two of which one is empty; the
MANY-ROWS cases give every wave four or five non-empty rows (4 500 rows under the cap of 1 024 waves) in three patterns — a shared
vocabulary across a wave's rows; rows of 60 to 190 all-distinct values beside three shared ones, so that the accumulator is flushed
between rows while it holds entries, filled again and flushed again; values that start probing at one entry of the accumulator — and
count, with a host model of the flush rule, the waves that flush in the middle of their walk.
The driver checks the guard regions behind every written buffer, the inputs unmodified and THE TABLE ALL ZERO after every launch, and runs
every input twice on the same table.  Every array comes from numpy.random.default_rng([SEED, ...]); SEED is in every assertion message."""
import numpy as np
import pytest

from madsim_amd import _abi as A
from tests import census_kernels as K
from tests import census_ref as R

pytestmark = pytest.mark.gpu

SEED = 20261020
ROWS = (1, 63, 64, 65, 257, 1025)             # the last: more rows than the grid has waves, so waves stride to further rows
OBS_CAPS = (1, 63, 64, 65, 130, A.CENSUS_MAX_OBS_CAP)
SPECIAL = (0, A.U64_MAX, A.FNV_OFFSET)
VERDICTS = (0, 1, 2, 3, 4, 5, 6, 7, 0xffffffff)
INCLUDES = (0xf, 0x1, 0x6, 0x8, 0xd)
ODD = 0x9E3779B97F4A7C15


def make_case(rng, n, obs_cap, vocab):
    """(rows, lens, results, seeds): row r's length by r % 8, its contents by (r // 8) % 4, its verdict from VERDICTS every fifth row and
    r % 4 otherwise; random non-zero words everywhere a row is not visible, random bytes in every result field but the verdict."""
    rows = rng.integers(1, 1 << 64, (n, obs_cap), dtype=np.uint64)
    lens = np.zeros(n, dtype=np.uint64)
    res = np.frombuffer(rng.bytes(n * K.RESULT_BYTES), dtype=A.RESULT_DTYPE).copy()
    vocab = np.array(vocab, dtype=np.uint64)
    for r in range(n):
        res["verdict"][r] = VERDICTS[(r // 5) % len(VERDICTS)] if r % 5 == 4 else r % 4
        kind = r % 8
        ln = (0, int(rng.integers(0, obs_cap + 1)), obs_cap, obs_cap + int(rng.integers(1, 1000)))[kind] if kind < 4 else int(rng.integers(0, 2 * obs_cap + 1))
        lens[r] = ln
        vis = min(ln, obs_cap)
        what = (r // 8) % 4
        if what == 0:                                                              # draws from the vocabulary: repeats inside a round and across rows
            rows[r, :vis] = vocab[rng.integers(0, len(vocab), vis)]
        elif what == 1:                                                            # every observation distinct (an odd multiplier is a bijection)
            rows[r, :vis] = (np.arange(r * obs_cap, r * obs_cap + vis, dtype=np.uint64) + np.uint64(1 << 40)) * np.uint64(ODD)
        elif what == 2:                                                            # period 3: the same three values in every round of the row
            rows[r, :vis] = vocab[np.arange(vis) % min(3, len(vocab))]
        else:                                                                      # one value, vis times: max_per_seed = vis
            rows[r, :vis] = vocab[r % len(vocab)]
    seeds = np.cumsum(rng.integers(1, 1000, n)).astype(np.uint64) + np.uint64(1 << 63)      # 64-bit seeds, ascending with the row
    return rows, lens, res, seeds


def check(got, want, include, tag):
    entries, w = got
    assert int(w[1]) == 0, (tag, "error word", int(w[1]))
    assert int(w[0]) == len(want.values) == len(entries), (tag, int(w[0]), len(want.values))
    assert entries.tobytes() == want.values.tobytes(), (tag, "entries")
    assert tuple(int(x) for x in w[2:6]) == want.n_counted and tuple(int(x) for x in w[6:10]) == want.n_silent, (tag, "n_counted / n_silent")
    assert (int(w[10]), int(w[11]), int(w[12])) == (want.n_truncated, want.n_observations, want.n_runner), (tag, "totals")
    assert not w[13:].any(), (tag, "words behind the totals")
    assert int(entries["n_total"].sum()) == want.n_observations, (tag, "sum of n_total")


@pytest.mark.parametrize("n", ROWS)
@pytest.mark.parametrize("obs_cap", OBS_CAPS)
def test_census_kernels_match_the_reference(hip, n, obs_cap):
    rng = np.random.default_rng([SEED, n, obs_cap])
    vocab = list(SPECIAL) + [int(x) for x in rng.integers(0, 1 << 64, 7, dtype=np.uint64)]
    rows, lens, res, seeds = make_case(rng, n, obs_cap, vocab)
    include = INCLUDES[(n + obs_cap) % len(INCLUDES)]
    want = R.census(rows, lens, res, seeds, include, obs_cap)
    tag = (SEED, n, obs_cap, include)
    assert want.n_runner or n < 25, tag
    cap = max(len(want.values), 1)                                                 # a table at exactly `cap` distinct values
    for direct in (False, True):
        for got in K.census(rows, lens, res, seeds, include, cap, launches=2, direct=direct):      # the second launch: the same table, left zero by the first
            check(got, want, include, tag + (direct,))
        if len(want.values) > 1:                                                   # ... and one at cap + 1: the error word, no entry, nothing out of bounds
            (entries, w), = K.census(rows, lens, res, seeds, include, cap - 1, direct=direct)
            assert int(w[1]) & K.ERR_CAP and not int(w[1]) & K.ERR_TAG and len(entries) == 0, (tag, direct, int(w[1]))


@pytest.mark.parametrize("include", INCLUDES)
def test_include_masks_and_verdicts(hip, include):
    """Every verdict 0 .. 7 and 2^32 - 1 over the same rows: rows with a runner verdict are tallied and never read, rows with a verdict that
    `include` leaves out are neither counted nor tallied."""
    n, obs_cap = 90, 70
    rng = np.random.default_rng([SEED, 1, include])
    rows, lens, res, seeds = make_case(rng, n, obs_cap, list(SPECIAL) + [5, 6])
    res["verdict"] = [VERDICTS[r % len(VERDICTS)] for r in range(n)]
    want = R.census(rows, lens, res, seeds, include, obs_cap)
    assert want.n_runner == sum(1 for r in range(n) if VERDICTS[r % len(VERDICTS)] >= 4) and sum(want.n_counted) > 0
    for direct in (False, True):
        for got in K.census(rows, lens, res, seeds, include, 4096, launches=2, direct=direct):
            check(got, want, include, (SEED, include, direct))


def test_values_that_start_probing_at_one_slot(hip):
    """40 values whose probe starts at slot 120 of 128: the chains run over one another and wrap past the table's end."""
    cap = 64
    slots = K.slots_for(cap)
    assert slots == 128
    rng = np.random.default_rng([SEED, 2])
    keys = []
    while len(keys) < 40:
        v = int(rng.integers(0, 1 << 64, dtype=np.uint64))
        if K.slot_of(v, slots) == 120 and v not in keys:
            keys.append(v)
    n, obs_cap = 200, 66
    rows, lens, res, seeds = make_case(rng, n, obs_cap, keys)
    for r in range(n):                                                             # every row draws from the colliding keys alone
        vis = min(int(lens[r]), obs_cap)
        rows[r, :vis] = np.array(keys, dtype=np.uint64)[rng.integers(0, len(keys), vis)]
    want = R.census(rows, lens, res, seeds, 0xf, obs_cap)
    assert len(want.values) == 40
    for direct in (False, True):
        for got in K.census(rows, lens, res, seeds, 0xf, cap, launches=2, direct=direct):
            check(got, want, 0xf, (SEED, "collide", direct))


MANY_ROWS, ACC_SLOTS, ACC_FILL = 4500, 256, 192        # CENSUS_ACC_SLOTS / CENSUS_ACC_FILL of sim_kernel.hip


def many_rows_case(rng, pattern):
    """(rows, lens, results, seeds, obs_cap) of MANY_ROWS rows, none empty: wave w of the 1 024 walks rows w, w + 1024, ..  Every 37th row
    carries a runner verdict (37 and 1 024 are coprime: no wave meets them at a fixed place), the others verdicts 0 .. 3."""
    n = MANY_ROWS
    shared = np.array(list(SPECIAL) + [int(x) for x in rng.integers(0, 1 << 64, 9, dtype=np.uint64)], dtype=np.uint64)
    if pattern == "vocabulary":
        obs_cap = 64
        lens = rng.integers(5, 61, n)
    elif pattern == "distinct":
        obs_cap = 192
        lens = rng.integers(60, 191, n)
    else:
        obs_cap = 96
        lens = rng.integers(70, 97, n)
        keys = []
        while len(keys) < 150:                                                     # values that start probing at entry 200 of the accumulator
            v = int(rng.integers(0, 1 << 64, dtype=np.uint64))
            if K.slot_of(v, ACC_SLOTS) == 200 and v not in keys:
                keys.append(v)
        keys = np.array(keys, dtype=np.uint64)
    rows = rng.integers(1, 1 << 64, (n, obs_cap), dtype=np.uint64)                 # random non-zero words behind every row's end
    res = np.frombuffer(rng.bytes(n * K.RESULT_BYTES), dtype=A.RESULT_DTYPE).copy()
    for r in range(n):
        res["verdict"][r] = VERDICTS[4 + r % 5] if r % 37 == 36 else (r // 3) % 4
        ln = int(lens[r])
        if pattern == "vocabulary":
            rows[r, :ln] = shared[rng.integers(0, len(shared), ln)]
        elif pattern == "distinct":                                                # ln - 3 values nobody else has, and three everybody has
            rows[r, :ln] = (np.arange(r * obs_cap, r * obs_cap + ln, dtype=np.uint64) + np.uint64(1 << 40)) * np.uint64(ODD)
            rows[r, rng.choice(ln, 3, replace=False)] = shared[:3]
        else:
            rows[r, :ln] = keys[rng.integers(0, len(keys), ln)]
    seeds = np.cumsum(rng.integers(1, 1000, n)).astype(np.uint64) + np.uint64(1 << 63)
    return rows, lens.astype(np.uint64), res, seeds, obs_cap


def mid_walk_flushes(rows, lens, res, include, obs_cap):
    """A host model of the accumulator's flush rule (sim_kernel.hip census_fold_kernel): (waves that walk two or more counted rows, waves that
    flush between two rows while entries are in use and go on to further rows, the most flushes of one wave)."""
    multi = flushing = most = 0
    for w in range(K.CENSUS_WAVES):
        in_use, held, walked, flushes = 0, set(), 0, 0
        for r in range(w, len(lens), K.CENSUS_WAVES):
            v = int(res["verdict"][r])
            if v >= 4 or not (include >> v) & 1:
                continue
            vis = min(int(lens[r]), obs_cap)
            assert 0 < vis <= ACC_FILL
            if in_use + vis > ACC_FILL:
                flushes += in_use > 0 and walked > 0
                in_use, held = 0, set()
            new = set(int(x) for x in rows[r, :vis]) - held
            held |= new
            in_use += len(new)
            walked += 1
        multi += walked >= 2
        flushing += flushes > 0
        most = max(most, flushes)
    return multi, flushing, most


@pytest.mark.parametrize("pattern", ["vocabulary", "distinct", "collide"])
def test_a_wave_walks_many_rows(hip, pattern):
    rng = np.random.default_rng([SEED, 5, len(pattern)])
    rows, lens, res, seeds, obs_cap = many_rows_case(rng, pattern)
    include = 0xf
    want = R.census(rows, lens, res, seeds, include, obs_cap)
    multi, flushing, most = mid_walk_flushes(rows, lens, res, include, obs_cap)
    print(pattern, "waves with two or more counted rows", multi, "waves that flush in mid-walk", flushing, "most flushes of a wave", most)
    assert multi == K.CENSUS_WAVES, (SEED, pattern, multi)                         # every wave walks several non-empty counted rows
    if pattern == "vocabulary":
        assert flushing == 0 and len(want.values) == 12                            # twelve values: the accumulator holds a wave's whole walk
    else:
        assert flushing >= K.CENSUS_WAVES // 2 and most >= 2, (SEED, pattern, flushing, most)      # flushed, filled again, flushed again
    cap = len(want.values)
    tag = (SEED, pattern)
    for direct in (False, True):
        for got in K.census(rows, lens, res, seeds, include, cap, launches=2, direct=direct):
            check(got, want, include, tag + (direct,))
        (entries, w), = K.census(rows, lens, res, seeds, include, cap - 1, direct=direct)
        assert int(w[1]) & K.ERR_CAP and not int(w[1]) & K.ERR_TAG and len(entries) == 0, (tag, direct, int(w[1]))


def test_one_row_repeats_a_value_across_every_round(hip):
    """One seed, 300 observations at obs_cap 256: a constant at the even indices and 150 increasing values at the odd ones — the constant
    lies in all four rounds and counts its seed once, with max_per_seed 128."""
    obs_cap = 256
    row = np.zeros((1, obs_cap), dtype=np.uint64)
    row[0, 0::2] = 7
    row[0, 1::2] = np.uint64(100) + np.arange(128, dtype=np.uint64)
    res = np.zeros(1, dtype=A.RESULT_DTYPE)
    res["verdict"] = A.DEADLOCK
    want = R.census(row, [300], res, [42], 0xf, obs_cap)
    for direct in (False, True):
        (entries, w), = K.census(row, [300], res, [42], 0xf, 1024, direct=direct)
        check((entries, w), want, 0xf, (SEED, "rounds", direct))
    seven = entries[entries["value"] == 7][0]
    assert tuple(seven["n_seeds"]) == (0, 0, 1, 0) and int(seven["n_total"]) == int(seven["max_per_seed"]) == 128 and int(seven["first_seed"]) == 42
    assert int(w[10]) == 1 and int(w[11]) == 256


def test_launcher_refuses_sizes_the_kernels_are_not_written_for(hip):
    import torch
    L = K._lib()
    buf = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda")
    p, st = buf.data_ptr(), torch.cuda.current_stream().cuda_stream
    ok = dict(obs=p, obs_cap=4, obs_len=p, res=p, seeds=p, n=4, include=0xf, table=p, slots=128, lst=p, cap=8, words=p, ent=p)
    for bad in (dict(n=0), dict(obs_cap=0), dict(obs_cap=A.CENSUS_MAX_OBS_CAP + 1), dict(n=1 << 30, obs_cap=4), dict(include=0), dict(include=0x10),
                dict(cap=0), dict(cap=A.CENSUS_MAX_VALUES + 1), dict(slots=64), dict(slots=192), dict(cap=65), dict(obs=None), dict(table=None),
                dict(words=None), dict(ent=None), dict(lst=None), dict(seeds=None)):
        a = dict(ok, **bad)
        assert L.madsim_k_launch_census(a["obs"], a["obs_cap"], a["obs_len"], a["res"], a["seeds"], a["n"], a["include"], a["table"], a["slots"],
                                        a["lst"], a["cap"], a["words"], a["ent"], st) == -1, bad
    torch.cuda.synchronize()
    assert not bool(buf.any())
