"""sets_mask_kernel / sets_fold_kernel / sets_extract_kernel (csrc/sim_kernel.hip) on SYNTHETIC rows, launched directly
(tests/sets_kernels.py): every set word, every entry and every count word is held against tests/sets_ref.py, exactly.  Rows the simulator
rarely or never produces: lengths 0, below, at and above obs_cap, with the words BEHIND min(len, obs_cap) filled with vocabulary values the
visible part lacks (a kernel that reads behind a row's end reports bits that are not there); a vocabulary value only at index 63, only at
index 64, only at vis - 1; rows of only foreign values and rows of only one value; vocabularies of 1, 2, 31, 32, 33, 61 and 62 values with
0, 2^64 - 1 and the FNV offset basis among them and the last bit reached; all rows one set (the most contention) and every row a set of its
own; set words built to start probing at one slot; a table at exactly `cap` sets and one at cap + 1; every verdict 0 .. 7 and 2^32 - 1 under
several include masks, the rows that are not counted holding sets nobody else has; 64-bit seeds with bit 63 set and seed0 + i.
Every case runs in both forms of the fold kernel: the in-wave combine and one table update per seed.  The driver checks the guard regions
behind every written buffer, the inputs unmodified and THE TABLE ALL ZERO after every launch, and runs every input twice on the same table.
Every array comes from numpy.random.default_rng([SEED, ...]); SEED is in every assertion message."""
import numpy as np
import pytest

from madsim_amd import _abi as A
from tests import sets_kernels as K
from tests import sets_ref as R

pytestmark = pytest.mark.gpu

SEED = 20261021
ROWS = (1, 63, 64, 65, 257, 1025, 4500)       # the last two: more rows than the grid has waves, so waves stride to further rows
OBS_CAPS = (1, 63, 64, 65, 130, A.CENSUS_MAX_OBS_CAP)
VOCAB_SIZES = (1, 2, 31, 32, 33, 61, 62)      # astride a 32-bit shift, and up to the last bit beside OTHER
SPECIAL = (0, A.U64_MAX, A.FNV_OFFSET)
VERDICTS = (0, 1, 2, 3, 4, 5, 6, 7, 0xffffffff)
INCLUDES = (0xf, 0x1, 0x6, 0x8, 0xd)
ODD = 0x9E3779B97F4A7C15
FOREIGN = 0x0123456789ABCDEF                  # in no vocabulary of this file


def make_vocab(rng, m):
    """m distinct values: random ones, with 0 first, 2^64 - 1 last and the FNV offset basis in the middle where there is room."""
    v = []
    while len(v) < m:
        x = int(rng.integers(1, 1 << 63, dtype=np.uint64))
        if x not in v and x not in SPECIAL and x != FOREIGN:
            v.append(x)
    v[0] = SPECIAL[0]
    if m >= 2:
        v[m - 1] = SPECIAL[1]
    if m >= 3:
        v[m // 2] = SPECIAL[2]
    return v


def foreign_words(rng, shape, vocab):
    a = rng.integers(1, 1 << 64, shape, dtype=np.uint64)
    a[np.isin(a, np.array(vocab, dtype=np.uint64))] = np.uint64(FOREIGN)
    return a


def hide_absent_values_behind_the_rows(rng, rows, lens, obs_cap, vocab):
    """Behind min(len, obs_cap) every row gets vocabulary values its visible part lacks (where it lacks none: foreign words, which stay)."""
    vocab = np.array(vocab, dtype=np.uint64)
    for r in range(len(rows)):
        vis = min(int(lens[r]), obs_cap)
        lacking = vocab[~np.isin(vocab, rows[r, :vis])]
        if vis < obs_cap and len(lacking):
            rows[r, vis:] = lacking[rng.integers(0, len(lacking), obs_cap - vis)]


def make_case(rng, n, obs_cap, vocab, bit63_seeds=True):
    """(rows, lens, results, seeds): row r's length by r % 8, its contents by (r // 8) % 6, its verdict from VERDICTS every fifth row and
    r % 4 otherwise; random bytes in every result field but the verdict."""
    m = len(vocab)
    va = np.array(vocab, dtype=np.uint64)
    rows = foreign_words(rng, (n, obs_cap), vocab)
    lens = np.zeros(n, dtype=np.uint64)
    res = np.frombuffer(rng.bytes(n * K.RESULT_BYTES), dtype=A.RESULT_DTYPE).copy()
    for r in range(n):
        res["verdict"][r] = VERDICTS[(r // 5) % len(VERDICTS)] if r % 5 == 4 else r % 4
        kind = r % 8
        ln = (0, int(rng.integers(0, obs_cap + 1)), obs_cap, obs_cap + int(rng.integers(1, 1000)))[kind] if kind < 4 else int(rng.integers(0, 2 * obs_cap + 1))
        if n <= 65 and r == n - 1:
            ln = obs_cap + 1                                                       # (a full row in the smallest cases too)
        lens[r] = ln
        vis = min(ln, obs_cap)
        what = (r // 8) % 6
        if what == 0:                                                              # draws from a few vocabulary values of the row's choosing
            rows[r, :vis] = va[rng.choice(m, min(m, 1 + r % 6), replace=False)][rng.integers(0, min(m, 1 + r % 6), vis)]
        elif what == 1:                                                            # only foreign values: OTHER alone
            pass
        elif what == 2:                                                            # only one value, vis times — the last of the vocabulary every other time
            rows[r, :vis] = va[m - 1] if r % 16 < 8 else va[r % m]
        elif what == 3 and vis:                                                    # foreign values and ONE vocabulary value at one place: 63, 64 or vis - 1
            rows[r, (63, 64, vis - 1)[r % 3] if (63, 64, vis - 1)[r % 3] < vis else vis - 1] = va[(r // 3) % m]
        elif what == 4:                                                            # a mix over the whole vocabulary and foreign words
            take = rng.random(vis) < 0.7
            rows[r, :vis][take] = va[rng.integers(0, m, int(take.sum()))]
        elif what == 5:                                                            # the whole vocabulary, in order, again and again
            rows[r, :vis] = va[np.arange(vis) % m]
    hide_absent_values_behind_the_rows(rng, rows, lens, obs_cap, vocab)
    if bit63_seeds:
        seeds = np.cumsum(rng.integers(1, 1000, n)).astype(np.uint64) + np.uint64(1 << 63)      # 64-bit seeds, ascending with the row
    else:
        seeds = np.uint64(int(rng.integers(0, 1 << 40))) + np.arange(n, dtype=np.uint64)         # seed0 + i
    return rows, lens, res, seeds


def counted_rows(res, include):
    v = res["verdict"].astype(np.uint64)
    return (v < 4) & (((np.uint64(include) >> np.minimum(v, np.uint64(63))) & np.uint64(1)) == 1)


def check(got, want, words, counted, tag):
    entries, w, sig = got
    assert int(w[1]) == 0, (tag, "error word", int(w[1]))
    assert int(w[0]) == len(want.sets) == len(entries), (tag, int(w[0]), len(want.sets))
    assert entries.tobytes() == want.sets.tobytes(), (tag, "entries", entries, want.sets)
    assert tuple(int(x) for x in w[2:6]) == want.n_counted and int(w[6]) == want.n_runner, (tag, "n_counted / n_runner")
    assert not w[7:].any(), (tag, "words behind the totals")
    assert (sig[counted] == words[counted]).all(), (tag, "set words", np.flatnonzero(counted & (sig != words))[:8])
    assert (sig[~counted] == np.uint64(K.PATTERN_WORD)).all(), (tag, "the set word of a row that is not counted was written")
    assert tuple(int(x) for x in entries["n_seeds"].sum(axis=0)) == want.n_counted if len(entries) else sum(want.n_counted) == 0, (tag, "column sums")


def run_both_forms(rows, lens, res, seeds, include, vocab, obs_cap, tag, cap=None, over=True):
    """Both forms of the fold kernel, twice each on one table, at `cap` = the number of sets exactly; and, with two or more sets, at one
    below: the error word, no entry, the table zero (the driver asserts that after every launch)."""
    words = R.set_words(rows, lens, vocab, obs_cap)
    want = R.fold(words, res["verdict"], seeds, include)
    counted = counted_rows(res, include)
    cap = cap or max(len(want.sets), 1)
    for per_seed in (False, True):
        for got in K.probe_sets(rows, lens, res, seeds, include, vocab, cap, launches=2, per_seed=per_seed):
            check(got, want, words, counted, tag + (per_seed,))
        if over and len(want.sets) > 1:
            (entries, w, _), = K.probe_sets(rows, lens, res, seeds, include, vocab, len(want.sets) - 1, per_seed=per_seed)
            assert int(w[1]) & K.ERR_CAP and not int(w[1]) & K.ERR_TAG and len(entries) == 0, (tag, per_seed, int(w[1]))
    return want, words


@pytest.mark.parametrize("n", ROWS)
@pytest.mark.parametrize("obs_cap", OBS_CAPS)
def test_probe_set_kernels_match_the_reference(hip, n, obs_cap):
    m = VOCAB_SIZES[(ROWS.index(n) + OBS_CAPS.index(obs_cap)) % len(VOCAB_SIZES)]
    rng = np.random.default_rng([SEED, n, obs_cap])
    vocab = make_vocab(rng, m)
    rows, lens, res, seeds = make_case(rng, n, obs_cap, vocab, bit63_seeds=(n + obs_cap) % 2 == 0)
    include = INCLUDES[(n + obs_cap) % len(INCLUDES)]
    tag = (SEED, n, obs_cap, m, include)
    want, words = run_both_forms(rows, lens, res, seeds, include, vocab, obs_cap, tag)
    assert want.n_runner or n < 25, tag
    if n >= 257:                                                                   # (by the reference: the case holds what it is meant to)
        sets = [int(s) for s in want.sets["set"]]
        assert any(s >> (m - 1) & 1 for s in sets) and any(s & R.OTHER for s in sets) and any(s & R.TRUNCATED for s in sets), tag
        assert any(not s & R.OTHER for s in sets) and (0 in sets or not include & 1), tag


@pytest.mark.parametrize("m", VOCAB_SIZES)
def test_every_vocabulary_size_reaches_its_last_bit(hip, m):
    """257 rows at obs_cap 130 under each vocabulary size: rows that hold the whole vocabulary, rows that hold its last value alone."""
    n, obs_cap = 257, 130
    rng = np.random.default_rng([SEED, 7, m])
    vocab = make_vocab(rng, m)
    rows, lens, res, seeds = make_case(rng, n, obs_cap, vocab)
    want, words = run_both_forms(rows, lens, res, seeds, 0xf, vocab, obs_cap, (SEED, "vocab", m))
    full = (1 << m) - 1
    sets = [int(s) & ~(R.OTHER | R.TRUNCATED) for s in want.sets["set"]]
    assert full in sets and 1 << (m - 1) in sets and all(s <= full for s in sets), (SEED, m)
    assert all(int(e["first_seed"][k]) >> 63 == 1 for e in want.sets for k in range(4) if int(e["n_seeds"][k])), (SEED, m)


@pytest.mark.parametrize("include", INCLUDES)
def test_include_masks_and_verdicts(hip, include):
    """Every verdict 0 .. 7 and 2^32 - 1 over the same rows: rows with a runner verdict are tallied and never read, rows with a verdict that
    `include` leaves out are neither counted nor tallied — each of them holds a set nobody else has (values 5 .. 9 of the vocabulary, which
    no counted row uses), so reading one shows as an entry."""
    n, obs_cap, m = 180, 70, 10
    rng = np.random.default_rng([SEED, 1, include])
    vocab = make_vocab(rng, m)
    rows, lens, res, seeds = make_case(rng, n, obs_cap, vocab[:5])
    res["verdict"] = [VERDICTS[r % len(VERDICTS)] for r in range(n)]
    counted = counted_rows(res, include)
    k = 0
    for r in np.flatnonzero(~counted):
        k += 1                                                                     # a non-empty subset of values 5 .. 9 and a length of its own
        rows[r] = np.uint64(FOREIGN)
        picks = [vocab[5 + b] for b in range(5) if (1 + k % 31) >> b & 1]
        rows[r, :len(picks)] = picks
        lens[r] = len(picks) + k % 3
    want, words = run_both_forms(rows, lens, res, seeds, include, vocab, obs_cap, (SEED, "include", include))
    assert want.n_runner == sum(1 for r in range(n) if VERDICTS[r % len(VERDICTS)] >= 4) and sum(want.n_counted) == int(counted.sum()) > 0
    assert not any(int(s) >> 5 & 0x1f for s in want.sets["set"]) and all(int(x) >> 5 & 0x1f for x in words[~counted]), (SEED, include)


def test_a_value_only_at_index_63_only_at_index_64_only_at_the_last_visible_index(hip):
    obs_cap, m = 130, 8
    rng = np.random.default_rng([SEED, 2])
    vocab = make_vocab(rng, m)
    places = [(63, 130), (64, 130), (129, 130), (129, 500), (99, 100), (63, 64), (64, 65), (0, 1), (62, 63)]      # (index, true length)
    rows = foreign_words(rng, (len(places), obs_cap), vocab)
    lens = np.array([ln for _, ln in places], dtype=np.uint64)
    for r, (at, _) in enumerate(places):
        rows[r, at] = vocab[1 + r % (m - 1)]
        if r % 2:
            rows[r, :at] = vocab[0]                                                # (0 in front of it, in place of foreign words)
    hide_absent_values_behind_the_rows(rng, rows, lens, obs_cap, vocab)
    res = np.zeros(len(places), dtype=A.RESULT_DTYPE)
    res["verdict"] = [r % 4 for r in range(len(places))]
    seeds = np.arange(len(places), dtype=np.uint64) + np.uint64(77)
    want, words = run_both_forms(rows, lens, res, seeds, 0xf, vocab, obs_cap, (SEED, "places"))
    for r, (at, ln) in enumerate(places):
        vis = min(ln, obs_cap)
        front = (1 if r % 2 else R.OTHER) if at else 0                             # vocab[0] or foreign words in front of it, foreign words behind it
        assert int(words[r]) == 1 << (1 + r % (m - 1)) | front | (R.OTHER if at < vis - 1 else 0) | (R.TRUNCATED if ln > obs_cap else 0), (SEED, r)


@pytest.mark.parametrize("n", [4500, 65])
def test_all_rows_one_set(hip, n):
    """The most contention: every counted seed lands on one slot; the four verdicts keep their own counts and smallest seeds."""
    obs_cap, m = 65, 33
    rng = np.random.default_rng([SEED, 3, n])
    vocab = make_vocab(rng, m)
    rows = np.tile(np.array([vocab[0], vocab[32], FOREIGN, vocab[16]] * 17, dtype=np.uint64)[:obs_cap], (n, 1))
    for r in range(n):
        rows[r] = rows[r][rng.permutation(obs_cap)]
    lens = np.full(n, obs_cap, dtype=np.uint64)
    res = np.frombuffer(rng.bytes(n * K.RESULT_BYTES), dtype=A.RESULT_DTYPE).copy()
    res["verdict"] = [VERDICTS[4 + r % 5] if r % 37 == 36 else (r // 3) % 4 for r in range(n)]
    seeds = np.cumsum(rng.integers(1, 1000, n)).astype(np.uint64) + np.uint64(1 << 63)
    want, _ = run_both_forms(rows, lens, res, seeds, 0xf, vocab, obs_cap, (SEED, "one set", n))
    assert [int(s) for s in want.sets["set"]] == [1 | 1 << 16 | 1 << 32 | R.OTHER] and all(int(x) for x in want.sets["n_seeds"][0]), (SEED, n)


def test_every_row_a_set_of_its_own(hip):
    """1 025 rows, 1 025 sets over 62 values: the table at exactly cap, and (run_both_forms) at one below."""
    n, obs_cap, m = 1025, 64, 62
    rng = np.random.default_rng([SEED, 4])
    vocab = make_vocab(rng, m)
    va = np.array(vocab, dtype=np.uint64)
    rows = np.zeros((n, obs_cap), dtype=np.uint64)
    lens = np.zeros(n, dtype=np.uint64)
    for r in range(n):
        word = ((r + 1) * ODD) & ((1 << m) - 1)
        bits = [b for b in range(m) if word >> b & 1]
        rows[r, :len(bits)] = va[rng.permutation(bits)]
        lens[r] = len(bits)
    hide_absent_values_behind_the_rows(rng, rows, lens, obs_cap, vocab)
    res = np.zeros(n, dtype=A.RESULT_DTYPE)
    res["verdict"] = [r % 4 for r in range(n)]
    seeds = np.uint64(1 << 40) + np.arange(n, dtype=np.uint64)
    want, _ = run_both_forms(rows, lens, res, seeds, 0xf, vocab, obs_cap, (SEED, "distinct"))
    assert len(want.sets) == n and K.slots_for(n) == 4096, (SEED, len(want.sets))


def test_set_words_that_start_probing_at_one_slot(hip):
    """40 set words whose probe starts at slot 120 of 128: the chains run over one another and wrap past the table's end."""
    cap, m, obs_cap = 64, 62, 64
    slots = K.slots_for(cap)
    assert slots == 128
    rng = np.random.default_rng([SEED, 5])
    vocab = make_vocab(rng, m)
    keys = []
    while len(keys) < 40:
        word = int(rng.integers(0, 1 << 62, dtype=np.uint64)) | (R.OTHER if len(keys) % 2 else 0)
        if K.slot_of(word, slots) == 120 and word not in keys and bin(word).count("1") <= obs_cap:
            keys.append(word)
    n = 300
    rows = np.zeros((n, obs_cap), dtype=np.uint64)
    lens = np.zeros(n, dtype=np.uint64)
    for r in range(n):
        word = keys[int(rng.integers(0, len(keys)))] if r >= 40 else keys[r]
        obs = [vocab[b] for b in range(m) if word >> b & 1] + ([FOREIGN] if word & R.OTHER else [])
        rows[r, :len(obs)] = np.array([obs[i] for i in rng.permutation(len(obs))], dtype=np.uint64)
        lens[r] = len(obs)
    hide_absent_values_behind_the_rows(rng, rows, lens, obs_cap, vocab)
    res = np.zeros(n, dtype=A.RESULT_DTYPE)
    res["verdict"] = [(r // 2) % 4 for r in range(n)]
    seeds = np.cumsum(rng.integers(1, 1000, n)).astype(np.uint64) + np.uint64(1 << 63)
    want, words = run_both_forms(rows, lens, res, seeds, 0xf, vocab, obs_cap, (SEED, "collide"), cap=cap, over=False)
    assert sorted(int(s) for s in want.sets["set"]) == sorted(keys), SEED


def test_launcher_refuses_sizes_the_kernels_are_not_written_for(hip):
    import ctypes as C

    import torch
    L = K._lib()
    buf = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda")
    p, st = buf.data_ptr(), torch.cuda.current_stream().cuda_stream
    vocab = (C.c_uint64 * 62)(*range(1, 63))
    v = C.cast(vocab, C.c_void_p).value
    ok = dict(obs=p, obs_cap=4, obs_len=p, res=p, seeds=p, n=4, include=0xf, vocab=v, n_vocab=3, sig=p, table=p, slots=128, lst=p, cap=8, words=p, ent=p)
    for bad in (dict(n=0), dict(obs_cap=0), dict(obs_cap=A.CENSUS_MAX_OBS_CAP + 1), dict(n=1 << 30, obs_cap=4), dict(n=(1 << 31) + 1, obs_cap=1),
                dict(include=0), dict(include=0x10), dict(cap=0), dict(cap=A.PROBE_SETS_MAX + 1), dict(slots=64), dict(slots=192), dict(cap=65),
                dict(n_vocab=0), dict(n_vocab=63), dict(vocab=None), dict(sig=None), dict(obs=None), dict(obs_len=None), dict(res=None), dict(table=None),
                dict(words=None), dict(ent=None), dict(lst=None), dict(seeds=None)):
        a = dict(ok, **bad)
        assert L.madsim_k_launch_probe_sets(a["obs"], a["obs_cap"], a["obs_len"], a["res"], a["seeds"], a["n"], a["include"], a["vocab"], a["n_vocab"],
                                            a["sig"], a["table"], a["slots"], a["lst"], a["cap"], a["words"], a["ent"], st) == -1, bad
    torch.cuda.synchronize()
    assert not bool(buf.any())
