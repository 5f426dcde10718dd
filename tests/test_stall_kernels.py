"""stall_sites_kernel (csrc/sim_kernel.hip) on SYNTHETIC task rows, launched directly (tests/stall_kernels.py), and the two census passes
behind it: every site word, shape word and length word, every entry and every count word is held against tests/stall_ref.py, exactly.
Rows the simulator rarely or never produces: counts 0, below, at and above task_cap with random NON-ZERO words behind min(len, task_cap)
(a kernel that reads behind a row's end reports tasks that are not there); every state byte 1 .. 255, program 255, pc 65 535; records
that share a site and differ in the loop registers alone (one site, one shape); rows that are permutations of one another (one shape);
every verdict 0 .. 7 and 2^32 - 1, where the rows of runner verdicts hold garbage counts and must not be read; every include mask; a
site table at exactly `cap` and one at cap + 1.  The driver checks the guard regions behind every written buffer, the inputs unmodified
and the census's table all zero after every launch.  Every array comes from numpy.random.default_rng([SEED, ...])."""
import numpy as np
import pytest

from madsim_amd import _abi as A
from madsim_amd import runtime
from tests import census_kernels as CK
from tests import stall_kernels as K
from tests import stall_ref as R

pytestmark = pytest.mark.gpu

SEED = 20261021
ROWS = (1, 63, 64, 65, 1025)                  # the last: more rows than the grid has waves, so waves stride to further rows
TASK_CAPS = (1, 63, 64, 65, 254)
VERDICTS = (0, 1, 2, 3, 4, 5, 6, 7, 0xffffffff)


def make_case(rng, n, task_cap, n_sites=9):
    """(rows, lens, results, seeds): row r's count by r % 6 — 0, random, task_cap, above it, and two random ones; its records drawn from a
    small vocabulary of sites (the extreme field values among them) with random loop registers; every third row a permutation of the row
    before it where the two are equally long; verdicts from VERDICTS every fifth row and r % 4 otherwise, the rows of runner verdicts with
    counts far above the cap; random non-zero words behind every row's visible part, random bytes in every result field but the verdict."""
    sites = [R.site_of(255, 255, 65535), R.site_of(1, 0, 0), R.site_of(R.PANICKED, 0, 1)]
    sites += [R.site_of(int(rng.integers(1, 256)), int(rng.integers(0, 256)), int(rng.integers(0, 65536))) for _ in range(n_sites - len(sites))]
    sites = np.array(sites, dtype=np.uint64)
    rows = rng.integers(1, 1 << 64, (n, task_cap), dtype=np.uint64)
    lens = np.zeros(n, dtype=np.uint64)
    res = np.frombuffer(rng.bytes(n * K.RESULT_BYTES), dtype=A.RESULT_DTYPE).copy()
    for r in range(n):
        v = VERDICTS[(r // 5) % len(VERDICTS)] if r % 5 == 4 else r % 4
        res["verdict"][r] = v
        ln = (0, int(rng.integers(0, task_cap + 1)), task_cap, task_cap + int(rng.integers(1, 200)), int(rng.integers(0, task_cap + 1)),
              int(rng.integers(0, 2 * task_cap + 1)))[r % 6]
        lens[r] = ln if v < 4 else (1 << 40) + r
        vis = min(ln, task_cap)
        if v >= 4:
            continue                                                               # (garbage everywhere: the row is not read)
        if r % 3 == 2 and r and min(int(lens[r - 1]), task_cap) == vis and int(res["verdict"][r - 1]) < 4:
            rows[r, :vis] = rng.permutation(rows[r - 1, :vis])
        else:
            regs = rng.integers(0, 1 << 32, vis, dtype=np.uint64)
            rows[r, :vis] = (sites[rng.integers(0, len(sites), vis)] << np.uint64(32)) | regs
    seeds = np.cumsum(rng.integers(1, 1000, n)).astype(np.uint64) + np.uint64(1 << 63)
    return rows, lens, res, seeds


def check_pass(got, want_entries, tag):
    entries, w = got
    assert int(w[1]) == 0, (tag, "error word", int(w[1]))
    assert int(w[0]) == len(want_entries) == len(entries), (tag, int(w[0]), len(want_entries))
    assert entries.tobytes() == want_entries.tobytes(), (tag, "entries")


@pytest.mark.parametrize("n", ROWS)
@pytest.mark.parametrize("task_cap", TASK_CAPS)
def test_sites_kernel_and_both_passes_match_the_reference(hip, n, task_cap):
    rng = np.random.default_rng([SEED, n, task_cap])
    rows, lens, res, seeds = make_case(rng, n, task_cap)
    include = (0xf, 0x6, 0xe, 0x1, 0xd)[(n + task_cap) % 5]
    tag = (SEED, n, task_cap, include)
    srows, shp, ones = K.sites(rows, lens, res)
    wrows, wshp, wones = R.sites_and_shapes(rows, lens, res, task_cap)
    assert srows.tobytes() == wrows.tobytes(), (tag, "site rows")
    assert shp.tobytes() == wshp.tobytes(), (tag, "shape words")
    assert ones.tobytes() == wones.tobytes(), (tag, "length words")
    for i in range(0, n, max(1, n // 7)):                                          # the exported host twin on the same rows
        vis = min(int(lens[i]), task_cap) if int(res["verdict"][i]) < 4 else 0
        assert runtime.stall_shape(rows[i, :vis]) == int(shp[i]), (tag, i)
    want = R.census(rows, lens, res, seeds, include, task_cap)
    site_cap, shape_cap = max(len(want.sites), 1), max(len(want.shapes), 1)         # tables at exactly `cap` distinct values
    a, b = K.census(rows, lens, res, seeds, include, site_cap, shape_cap, launches=2)
    for got in a:
        check_pass(got, want.sites, tag + ("sites",))
        w = got[1]
        assert tuple(int(x) for x in w[2:6]) == want.n_counted and tuple(int(x) for x in w[6:10]) == want.n_idle, (tag, "n_counted / n_idle")
        assert (int(w[10]), int(w[11]), int(w[12])) == (want.n_truncated, want.n_tasks, want.n_runner), (tag, "totals")
        assert int(got[0]["n_total"].sum()) == want.n_tasks, (tag, "sum of n_total")
    for got in b:
        check_pass(got, want.shapes, tag + ("shapes",))
        assert tuple(int(x) for x in got[1][2:6]) == want.n_counted, (tag, "the shape pass counts the same seeds")
        assert int(got[0]["n_seeds"].sum()) == sum(want.n_counted) and (got[0]["max_per_seed"] == 1).all(), (tag, "one shape per counted seed")
    if len(want.sites) > 1:                                                        # one distinct site more than site_cap
        (entries, w), = CK.census(wrows, lens, res, seeds, include, site_cap - 1)
        assert int(w[1]) & CK.ERR_CAP and not int(w[1]) & CK.ERR_TAG and len(entries) == 0, (tag, int(w[1]))


@pytest.mark.parametrize("include", range(1, 16))
def test_every_include_mask_over_every_verdict(hip, include):
    n, task_cap = 90, 40
    rng = np.random.default_rng([SEED, 1, include])
    rows, lens, res, seeds = make_case(rng, n, task_cap)
    res["verdict"] = [VERDICTS[r % len(VERDICTS)] for r in range(n)]
    lens[np.asarray(res["verdict"]) >= 4] = 1 << 50                                 # runner rows: a count that would run far behind the array
    want = R.census(rows, lens, res, seeds, include, task_cap)
    assert want.n_runner == sum(1 for r in range(n) if VERDICTS[r % len(VERDICTS)] >= 4) and sum(want.n_counted) > 0
    a, b = K.census(rows, lens, res, seeds, include, 4096, 4096)
    check_pass(a[0], want.sites, (SEED, include, "sites"))
    check_pass(b[0], want.shapes, (SEED, include, "shapes"))
    assert tuple(int(x) for x in a[0][1][2:6]) == want.n_counted and int(a[0][1][12]) == want.n_runner


def test_every_state_byte_and_the_field_extremes(hip):
    """255 rows, row s - 1 a single record of state s with program 255 at pc 65 535: 255 distinct sites and 255 distinct shapes; then the same
    rows with other loop registers added below: the same sites, the same shapes, twice the seeds."""
    recs = np.array([R.word(s, 255, 65535, s, 65535 - s) for s in range(1, 256)], dtype=np.uint64)
    again = np.array([R.word(s, 255, 65535, 7, 9) for s in range(1, 256)], dtype=np.uint64)
    rows = np.concatenate([recs, again]).reshape(-1, 1)
    n = len(rows)
    lens, res = np.ones(n, dtype=np.uint64), np.zeros(n, dtype=A.RESULT_DTYPE)
    res["verdict"] = A.DEADLOCK
    seeds = np.arange(1000, 1000 + n, dtype=np.uint64)
    srows, shp, _ = K.sites(rows, lens, res)
    assert [int(x) for x in srows[:255, 0]] == [R.site_of(s, 255, 65535) for s in range(1, 256)]
    assert srows[:255].tobytes() == srows[255:].tobytes() and shp[:255].tobytes() == shp[255:].tobytes()
    assert [int(x) for x in shp[:255]] == [R.mix(R.site_of(s, 255, 65535)) for s in range(1, 256)] and len(set(shp[:255].tolist())) == 255
    want = R.census(rows, lens, res, seeds, 1 << A.DEADLOCK, 1)
    a, b = K.census(rows, lens, res, seeds, 1 << A.DEADLOCK, 255, 255)
    check_pass(a[0], want.sites, "sites"); check_pass(b[0], want.shapes, "shapes")
    assert (a[0][0]["n_seeds"][:, A.DEADLOCK] == 2).all() and (b[0][0]["n_seeds"][:, A.DEADLOCK] == 2).all()
    assert [int(x) for x in a[0][0]["first_seed"]] == list(range(1000, 1255))


def test_sizes_the_launcher_refuses():
    assert K.refused(0, 1) == -1 and K.refused(A.MAX_LIVE_TASKS + 1, 1) == -1 and K.refused(1, 0) == -1
    assert K.refused(254, (1 << 32) // 254 + 1) == -1 and K.refused(1, (1 << 31) + 1) == -1
    assert K.refused(8, 8) == -1                                                   # (a missing array)
