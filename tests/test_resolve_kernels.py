"""The resolving campaign's kernels alone, on the MI355X, over synthetic result arrays (tests/resolve_kernels.py drives the exported launchers):
the list pair against numpy's nonzero — the count word, the seed list and the index list, in order, nothing behind them written — and the
scatter against a host copy.  Sizes: one seed, a wave minus / exactly / plus one, a workgroup's four waves likewise, more than one workgroup with
a last piece of one result (4 097), and 262 209 — the 1 024-wave cap with pieces of 320 results, the last piece in use ragged."""
import numpy as np
import pytest

from madsim_amd import _abi as A
from tests import resolve_kernels as K

pytestmark = pytest.mark.gpu

SIZES = (1, 63, 64, 65, 1023, 1024, 1025, 4097, 262209)
SEED0S = (0, (1 << 40) + 7, None)                                   # None: 2^64 - count, the last seeds there are
VERDICTS = (0, 1, 2, 3, 4, 5, 6, 7, 0xFFFFFFFF)


def synthetic(rng, n, verdicts):
    """n results with verdicts drawn from `verdicts` and every other field random (the kernels must read the verdict word alone)."""
    r = np.zeros(n, dtype=A.RESULT_DTYPE)
    r["verdict"] = rng.choice(np.array(verdicts, dtype=np.uint32), size=n)
    r["steps"] = rng.integers(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32)
    for f in ("clock_ns", "msg_count", "rng_calls", "trace_hash", "obs_hash"):
        r[f] = rng.integers(0, 1 << 63, size=n, dtype=np.uint64) * 2 + rng.integers(0, 2, size=n, dtype=np.uint64)
    return r


def cases(rng, n):
    """name -> results: no re-runnable seed; every seed; one, in the last lane of the last piece; a mix of every verdict value."""
    none = synthetic(rng, n, (0, 1, 2, 3, 6, 7, 0xFFFFFFFF))
    every = synthetic(rng, n, (A.OVERFLOW,))
    last = none.copy()
    last["verdict"][n - 1] = A.OVERFLOW
    steps = synthetic(rng, n, (A.STEP_LIMIT, A.PASS))                # re-runnable only while the step cap can grow
    return {"none": none, "every": every, "last": last, "mix": synthetic(rng, n, VERDICTS), "step limits": steps}


def cut(n):
    """(waves, piece) of the launcher's cut for n results: collect's."""
    waves = 4 * min((n + 1023) // 1024, 256)
    return waves, ((n + waves - 1) // waves + 63) // 64 * 64


def test_the_sizes_mean_what_the_docstring_says():
    assert cut(262209) == (1024, 320) and 262209 - 819 * 320 == 129           # the wave cap; 820 pieces in use, the last one ragged, 204 waves idle
    assert cut(4097) == (20, 256) and 4097 - 16 * 256 == 1                    # five workgroups; the 17th piece holds one result
    assert cut(1025) == (8, 192) and cut(1024) == (4, 256) and cut(65) == (4, 64)


@pytest.mark.parametrize("n", SIZES)
def test_the_lists_are_numpys(hip, n):
    rng = np.random.default_rng(n)
    for k, (name, res) in enumerate(cases(rng, n).items()):
        d = K.upload(res)
        for steps_maxed in (0, 1):
            seed0 = SEED0S[(k + steps_maxed) % 3]
            seed0 = (1 << 64) - n if seed0 is None else seed0
            want = np.nonzero(K.rerunnable(res["verdict"], steps_maxed))[0]
            m, seeds, idx = K.resolve_list(d, n, seed0, steps_maxed)
            what = (name, n, steps_maxed, seed0)
            assert m == len(want), (what, m, len(want))
            assert idx.dtype == np.uint32 and (idx == want).all(), what
            assert seeds.dtype == np.uint64 and [int(s) for s in seeds[:4]] == [seed0 + int(i) for i in want[:4]], what
            assert (seeds == (np.uint64(seed0) + want.astype(np.uint64))).all(), what
            if name == "none":
                assert m == 0
            if name == "every":
                assert m == n
            if name == "last":
                assert m == 1 and int(idx[0]) == n - 1 and int(seeds[0]) == seed0 + n - 1
            if name == "step limits":
                assert (m == 0) == bool(steps_maxed) or not (res["verdict"] == A.STEP_LIMIT).any()


def test_every_seed0_with_every_case(hip):
    """The three seed0 values against one size that spans several workgroups, with both settings of steps_maxed."""
    n = 4097
    rng = np.random.default_rng(7)
    res = synthetic(rng, n, VERDICTS)
    d = K.upload(res)
    for seed0 in (0, (1 << 40) + 7, (1 << 64) - n):
        for steps_maxed in (0, 1):
            want = np.nonzero(K.rerunnable(res["verdict"], steps_maxed))[0]
            m, seeds, idx = K.resolve_list(d, n, seed0, steps_maxed)
            assert m == len(want) and (idx == want).all() and [int(s) for s in seeds] == [seed0 + int(i) for i in want], (seed0, steps_maxed)
    both = np.nonzero(K.rerunnable(res["verdict"], 0))[0]
    assert len(both) > len(np.nonzero(K.rerunnable(res["verdict"], 1))[0]) > 0           # the mix holds both kinds


@pytest.mark.parametrize("n", (1, 65, 1025, 262209))
def test_scatter_moves_the_named_records_and_nothing_else(hip, n):
    rng = np.random.default_rng(1000 + n)
    out = synthetic(rng, n, VERDICTS)
    for m in sorted({0, 1, min(65, n), n}):
        idx = rng.permutation(n)[:m].astype(np.uint32)                              # random distinct indices, in no order
        rerun = synthetic(rng, m, VERDICTS)
        got = K.scatter(out, rerun, idx)
        want = out.copy()
        want[idx] = rerun
        assert got.tobytes() == want.tobytes(), (n, m)
        if m:
            assert got[idx].tobytes() == rerun.tobytes()
        untouched = np.ones(n, dtype=bool)
        untouched[idx] = False
        assert got[untouched].tobytes() == out[untouched].tobytes(), (n, m)
