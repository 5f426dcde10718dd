"""The host-side truth of the campaign report kernels (summary_kernel, summary6_kernel, collect_count_kernel + collect_write_kernel,
stats_fold_kernel + stats_top_kernel in madsim_amd/csrc/sim_kernel.hip) over ANY madsim_result_t array: numpy filters, sums and sorts, a
restatement of the launchers' cut of a batch, and the layout of a statistics truth as the device's words.  Independent of the library:
tests/test_report_kernels.py holds every function here against plain Python ints first (no GPU), then the kernels against these.
The statistics truth itself is tests/stats_ref.py's stats_truth."""
import numpy as np

from madsim_amd import _abi as A
from tests import stats_ref as R
from tests.test_collect_gpu import listed

NONE = (1 << 64) - 1
COLLECT_WORDS, STATS_WORDS = 15, 657                       # MADSIM_K_COLLECT_WORDS, MADSIM_K_STATS_WORDS
HIST_OFF, TOP_OFF = 17, 17 + 4 * 256 // 2                  # srep: 17 words, hist[4][256] as 32-bit counters, top[4][16] {value, seed}


def cut(count):
    """(workgroups, results per wave) of the collect / statistics launchers: at most 256 workgroups of 4 waves, wave W owns the piece
    [W * piece, (W + 1) * piece) of the batch, a multiple of 64 results."""
    grid = min(max((count + 1023) // 1024, 1), 256)
    waves = 4 * grid
    return grid, ((count + waves - 1) // waves + 63) // 64 * 64


def wrapping_sum(a):
    """Sum mod 2^64 (the kernels' 64-bit adds wrap)."""
    return int(np.asarray(a).astype(np.uint64).sum(dtype=np.uint64))


def summary_truth(results, seed0):
    """(summary_kernel's four words, summary6_kernel's six): {first failing seed, n failing, steps, clock_ns, first seed with a genuine
    verdict, n runner verdicts}; 2^64 - 1 where there is no such seed."""
    v = results["verdict"]
    failing = np.nonzero(v != A.PASS)[0]
    genuine = np.nonzero((v != A.PASS) & (v < A.OVERFLOW))[0]
    four = [seed0 + int(failing[0]) if len(failing) else NONE, len(failing), wrapping_sum(results["steps"]), wrapping_sum(results["clock_ns"])]
    return four, four + [seed0 + int(genuine[0]) if len(genuine) else NONE, len(failing) - len(genuine)]


def listed_mask(results, list_runner):
    v = results["verdict"]
    return (v != A.PASS) & ((v < A.OVERFLOW) | bool(list_runner))


def collect_truth(results, seed0, cap, list_runner):
    """(the 15 words: summary6's six, by_verdict[8] — a verdict of 7 or more counts as 7 —, n listed; the bytes of the min(cap, n listed)
    records)."""
    _, six = summary_truth(results, seed0)
    by_verdict = np.bincount(np.minimum(results["verdict"], 7), minlength=8)
    words = np.array(six + [int(c) for c in by_verdict] + [int(listed_mask(results, list_runner).sum())], dtype=np.uint64)
    return words, listed(results, np.uint64(seed0), cap, bool(list_runner)).tobytes()


def wave_counts(results, list_runner):
    """wave_cnt[W], W < 4 * workgroups: the listed seeds of wave W's piece."""
    grid, piece = cut(len(results))
    m = listed_mask(results, list_runner)
    return np.pad(m, (0, 4 * grid * piece - len(m))).reshape(4 * grid, piece).sum(axis=1).astype(np.uint32)


def stats_words(truth):
    """A stats_truth as the device's 657 words: n, ~min[4], max[4], low half-sums[4], high half-sums[4], hist[4][256] as 32-bit counters,
    top[4][16] {value, seed} (zero from n_top on)."""
    w = np.zeros(STATS_WORDS, dtype=np.uint64)
    w[0] = truth["n"]
    hist = np.zeros((4, R.N_BUCKETS), dtype=np.uint32)
    for m, name in enumerate(R.METRICS):
        t = truth[name]
        w[1 + m], w[5 + m], w[9 + m], w[13 + m] = NONE ^ t["min"], t["max"], t["halves"][0], t["halves"][1]
        assert int(t["hist"].max()) < 1 << 32
        hist[m] = t["hist"]
        for r, (value, seed) in enumerate(t["top"]):
            w[TOP_OFF + 2 * (16 * m + r)], w[TOP_OFF + 2 * (16 * m + r) + 1] = value, seed
    w[HIST_OFF:TOP_OFF] = hist.reshape(-1).view(np.uint64)
    return w
