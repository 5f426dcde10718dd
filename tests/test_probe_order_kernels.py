"""order_fold_kernel / order_extract_kernel (csrc/sim_kernel.hip) on SYNTHETIC rows, launched directly (tests/order_kernels.py): every
entry and every count word is held against tests/order_ref.py, exactly, and the entries in the order the device wrote them: ascending by
(a, b).  The rows are those of tests/test_probe_sets_kernels.py (lengths 0, below, at and above obs_cap, the words BEHIND min(len, obs_cap)
filled with vocabulary values the visible part lacks; a value only at index 63, only at 64, only at vis - 1; rows of only foreign values
and of only one value; every verdict 0 .. 7 and 2^32 - 1; 64-bit seeds with bit 63 set) and directed ones: two values at (63, 64),
(64, 63) and (0, vis - 1); a value first seen in round 0 that recurs in later rounds before and after another value's first occurrence (a
kernel that moves `first` gets the order wrong); all rows identical (the most contention on one cell); every row its own permutation of
the vocabulary; a cell whose smallest witness lies in a row handled by a later workgroup than its largest; rows that are not counted
holding orders nobody else has.  Every case runs in both forms of the fold kernel — the workgroup accumulator in LDS and every update
straight to the global matrix — and twice on the same matrix.  The driver checks the guard regions behind every written buffer, the inputs
unmodified and THE MATRIX ALL ZERO after every launch.  Every array comes from numpy.random.default_rng([SEED, ...]); SEED is in every
assertion message."""
import numpy as np
import pytest

from madsim_amd import _abi as A
from tests import order_kernels as K
from tests import order_ref as R
from tests import test_probe_sets_kernels as SK

pytestmark = pytest.mark.gpu

SEED = 20261022
ROWS = (1, 63, 64, 65, 257, 1025, 4500)       # the last two: more rows than the grid has waves, so waves stride to further rows
OBS_CAPS = (1, 63, 64, 65, 130, A.CENSUS_MAX_OBS_CAP)
VOCAB_SIZES = (1, 2, 31, 32)
INCLUDES = (0xf, 0x1, 0x6, 0x8, 0xd)
FOREIGN = SK.FOREIGN


def results_of(rng, verdicts):
    res = np.frombuffer(rng.bytes(len(verdicts) * K.RESULT_BYTES), dtype=A.RESULT_DTYPE).copy()
    res["verdict"] = verdicts
    return res


def seeds_of(rng, n):
    return np.cumsum(rng.integers(1, 1000, n)).astype(np.uint64) + np.uint64(1 << 63)      # 64-bit seeds, ascending with the row


def run_both(rows, lens, res, seeds, include, vocab, tag):
    """Both forms, twice each on one matrix, against the reference; returns the reference."""
    want = R.probe_order(rows, lens, res, seeds, include, rows.shape[1], vocab)
    for direct in (False, True):
        for launch, (entries, w) in enumerate(K.probe_order(rows, lens, res, seeds, include, vocab, launches=2, direct=direct)):
            t = (SEED, tag, "direct" if direct else "lds", launch)
            assert int(w[1]) == 0, (t, "error word", int(w[1]))
            assert [int(x) for x in w] == [int(x) for x in want.words()], (t, "words", w, want.words())
            assert entries.tobytes() == want.pairs.tobytes(), (t, "entries", entries, want.pairs)
    return want


@pytest.mark.parametrize("obs_cap", OBS_CAPS)
@pytest.mark.parametrize("n", ROWS)
def test_every_shape_in_both_forms(n, obs_cap):
    i = ROWS.index(n) * len(OBS_CAPS) + OBS_CAPS.index(obs_cap)
    m, include = VOCAB_SIZES[i % len(VOCAB_SIZES)], INCLUDES[i % len(INCLUDES)]
    rng = np.random.default_rng([SEED, n, obs_cap])
    vocab = SK.make_vocab(rng, m)
    rows, lens, res, seeds = SK.make_case(rng, n, obs_cap, vocab)
    want = run_both(rows, lens, res, seeds, include, vocab, (n, obs_cap, m, include))
    if n >= 257:
        assert len(want.pairs) and want.n_runner and sum(want.n_counted), (SEED, n, obs_cap)
        assert obs_cap == 1 or want.n_truncated


@pytest.mark.parametrize("include", INCLUDES)
@pytest.mark.parametrize("m", VOCAB_SIZES)
def test_every_vocabulary_size_under_every_include_mask(m, include):
    rng = np.random.default_rng([SEED, m, include, 1])
    vocab = SK.make_vocab(rng, m)
    assert vocab[0] == 0 and (m < 2 or vocab[-1] == A.U64_MAX) and (m < 3 or A.FNV_OFFSET in vocab)
    rows, lens, res, seeds = SK.make_case(rng, 300, 130, vocab)
    want = run_both(rows, lens, res, seeds, include, vocab, (m, include))
    assert len(want.pairs) >= min(m * m, 2) and (m < 31 or int(want.pairs["a"].max()) == m - 1 == int(want.pairs["b"].max())), (SEED, m, include)


@pytest.mark.parametrize("obs_cap", [65, 130, A.CENSUS_MAX_OBS_CAP])
def test_two_values_astride_a_round_and_at_the_ends_of_a_row(obs_cap):
    rng = np.random.default_rng([SEED, obs_cap, 2])
    vocab = SK.make_vocab(rng, 3)
    n = 12
    rows = SK.foreign_words(rng, (n, obs_cap), vocab)
    lens = np.full(n, obs_cap, dtype=np.uint64)
    for r in range(n):
        ia, ib = ((63, 64), (64, 63), (0, obs_cap - 1), (obs_cap - 1, 0))[r % 4]
        rows[r, ia], rows[r, ib] = vocab[0], vocab[1]
    res, seeds = results_of(rng, np.arange(n) % 4), seeds_of(rng, n)
    want = run_both(rows, lens, res, seeds, 0xf, vocab, obs_cap)
    cells = {(int(e["a"]), int(e["b"])): [int(x) for x in e["n_seeds"]] for e in want.pairs}
    assert cells == {(0, 0): [3, 3, 3, 3], (0, 1): [3, 0, 3, 0], (1, 0): [0, 3, 0, 3], (1, 1): [3, 3, 3, 3]}, (SEED, cells)


def test_a_value_that_recurs_in_later_rounds_keeps_its_first_occurrence():
    rng = np.random.default_rng([SEED, 3])
    vocab = SK.make_vocab(rng, 4)
    n, obs_cap = 70, 300
    rows = SK.foreign_words(rng, (n, obs_cap), vocab)
    lens = np.full(n, obs_cap, dtype=np.uint64)
    for r in range(n):
        # value 0 first in round 0, again before and after value 1's first (round 1) and value 2's first (round 3); value 3 never
        rows[r, [3, 65, 100, 200, 299]] = vocab[0]
        rows[r, [70, 71, 250]] = vocab[1]
        rows[r, [199, 201]] = vocab[2]
    res, seeds = results_of(rng, np.zeros(n, dtype=np.uint32)), seeds_of(rng, n)
    want = run_both(rows, lens, res, seeds, 0xf, vocab, "recurs")
    assert [(int(e["a"]), int(e["b"])) for e in want.pairs] == [(0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)], SEED
    assert all(int(e["n_seeds"][0]) == n and int(e["first_seed"][0]) == int(seeds[0]) for e in want.pairs)


@pytest.mark.parametrize("n", [257, 4500])
def test_all_rows_identical_meet_on_one_cell(n):
    rng = np.random.default_rng([SEED, n, 4])
    vocab = SK.make_vocab(rng, 32)
    obs_cap = 64
    rows = np.tile(np.array(vocab[::-1] + [FOREIGN] * 32, dtype=np.uint64), (n, 1))      # the vocabulary backwards: (a, b) for every a > b
    lens = np.full(n, 40, dtype=np.uint64)
    res, seeds = results_of(rng, np.full(n, 2, dtype=np.uint32)), seeds_of(rng, n)
    want = run_both(rows, lens, res, seeds, 0x4, vocab, ("identical", n))
    assert len(want.pairs) == 32 * 33 // 2 and all(int(e["n_seeds"][2]) == n and int(e["a"]) >= int(e["b"]) for e in want.pairs), SEED
    assert all(int(e["first_seed"][2]) == int(seeds[0]) for e in want.pairs) and want.n_counted == (0, 0, n, 0)


def test_every_row_its_own_permutation_of_the_vocabulary():
    rng = np.random.default_rng([SEED, 5])
    vocab = SK.make_vocab(rng, 32)
    n, obs_cap = 1025, 65
    rows = SK.foreign_words(rng, (n, obs_cap), vocab)
    for r in range(n):
        rows[r, rng.permutation(obs_cap)[:32]] = np.array(vocab, dtype=np.uint64)[rng.permutation(32)]      # 32 places, 32 values
    lens = np.full(n, obs_cap + 5, dtype=np.uint64)
    res, seeds = results_of(rng, np.arange(n) % 4), seeds_of(rng, n)
    want = run_both(rows, lens, res, seeds, 0xf, vocab, "permutations")
    assert len(want.pairs) == 1024 and want.n_truncated == n and want.n_none == (0, 0, 0, 0), SEED      # every cell, all four verdicts


def test_the_smallest_witness_sits_in_a_later_workgroup_than_the_largest():
    """Row i is walked by workgroup (i % 1024) // 4: row 1020 by the last one, row 1025 by the first on its second stride."""
    rng = np.random.default_rng([SEED, 6])
    vocab = SK.make_vocab(rng, 2)
    n, obs_cap = 1030, 8
    rows = SK.foreign_words(rng, (n, obs_cap), vocab)
    lens = np.full(n, obs_cap, dtype=np.uint64)
    rows[:, 5] = vocab[0]                                                           # everywhere: 0 alone ...
    for r in (1020, 1025):
        rows[r, 2] = vocab[1]                                                       # ... but here 1 comes first
    res, seeds = results_of(rng, np.full(n, 1, dtype=np.uint32)), seeds_of(rng, n)
    want = run_both(rows, lens, res, seeds, 0xf, vocab, "witness")
    cell = {(int(e["a"]), int(e["b"])): e for e in want.pairs}[(1, 0)]
    assert int(cell["n_seeds"][1]) == 2 and int(cell["first_seed"][1]) == int(seeds[1020]), SEED
    assert K.ORDER_WAVES == 1024 and 1020 % 1024 // 4 > 1025 % 1024 // 4


@pytest.mark.parametrize("include", INCLUDES)
def test_rows_that_are_not_counted_hold_orders_nobody_else_has(include):
    rng = np.random.default_rng([SEED, include, 7])
    vocab = SK.make_vocab(rng, 3)
    n, obs_cap = 600, 70
    verdicts = np.array([SK.VERDICTS[r % len(SK.VERDICTS)] for r in range(n)], dtype=np.uint32)
    counted = (verdicts < 4) & ((include >> np.minimum(verdicts, 31)) & 1 == 1)
    rows = SK.foreign_words(rng, (n, obs_cap), vocab)
    lens = np.full(n, obs_cap, dtype=np.uint64)
    for r in range(n):
        if counted[r]:
            rows[r, 10], rows[r, 66] = vocab[0], vocab[1]
        else:
            rows[r, 10], rows[r, 66], rows[r, 30] = vocab[1], vocab[0], vocab[2]      # 1 before 0, and a value the counted rows never see
    res, seeds = results_of(rng, verdicts), seeds_of(rng, n)
    want = run_both(rows, lens, res, seeds, include, vocab, ("uncounted", include))
    assert [(int(e["a"]), int(e["b"])) for e in want.pairs] == [(0, 0), (0, 1), (1, 1)], (SEED, include)
    assert sum(want.n_counted) == int(counted.sum()) > 0 and want.n_runner == int((verdicts >= 4).sum()) > 0
