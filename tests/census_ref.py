"""The observation census (include/madsim_hip.h, madsim_hip_census_range) restated in plain numpy and Python ints, from what
madsim_hip_trace_seeds returns: observation rows uint64[n, >= obs_cap], the TRUE lengths, the results and the seeds.  Test-only: the truth
tests/test_census*.py hold the kernels, the host fold and the public calls against.  Whatever a row holds at or behind min(len, obs_cap)
is ignored."""
import numpy as np

from madsim_amd import _abi as A


class Ref:
    """`values` ndarray[A.CENSUS_VALUE_DTYPE] ascending by value, the totals as Python ints / 4-tuples, `runner_seeds` ascending."""

    def __init__(self, values, n_counted, n_silent, n_truncated, n_observations, n_runner, runner_seeds):
        self.values, self.n_counted, self.n_silent = values, tuple(n_counted), tuple(n_silent)
        self.n_truncated, self.n_observations, self.n_runner, self.runner_seeds = n_truncated, n_observations, n_runner, runner_seeds

    def tobytes(self):
        """As runtime.Census.tobytes lays it out."""
        totals = np.array(self.n_counted + self.n_silent + (self.n_truncated, self.n_observations, self.n_runner), dtype=np.uint64)
        return self.values.tobytes() + totals.tobytes() + np.asarray(self.runner_seeds, dtype=np.uint64).tobytes()


def census(rows, lens, results, seeds, include, obs_cap):
    """The census of the seeds `seeds` (any order, distinct).  rows: uint64[n, c] with c >= obs_cap (or c >= every length), lens: n true
    lengths, results: ndarray[A.RESULT_DTYPE] or anything with a "verdict" column, include: the bit mask."""
    rows, lens = np.asarray(rows, dtype=np.uint64), [int(x) for x in lens]
    verdicts, seeds = [int(v) for v in results["verdict"]], [int(s) for s in seeds]
    n = len(seeds)
    assert rows.shape[0] == n == len(lens) == len(verdicts)
    n_counted, n_silent, n_truncated, n_observations, runner = [0] * 4, [0] * 4, 0, 0, []
    vals, row_of, count = [], [], []                       # one entry per (row, distinct visible value): the value, the row, its occurrences in the row
    for i in range(n):
        v = verdicts[i]
        if v >= 4:
            runner.append(seeds[i])
            continue
        if not (include >> v) & 1:
            continue
        vis = min(lens[i], obs_cap)
        n_counted[v] += 1
        n_silent[v] += vis == 0
        n_truncated += lens[i] > obs_cap
        n_observations += vis
        if vis:
            u, c = np.unique(rows[i, :vis], return_counts=True)
            vals.append(u); count.append(c); row_of.append(np.full(len(u), i))
    out = np.zeros(0, dtype=A.CENSUS_VALUE_DTYPE)
    if vals:
        vals, row_of, count = np.concatenate(vals), np.concatenate(row_of), np.concatenate(count).astype(np.uint64)
        uniq, inv = np.unique(vals, return_inverse=True)
        out = np.zeros(len(uniq), dtype=A.CENSUS_VALUE_DTYPE)
        out["value"] = uniq
        vd, sd = np.array(verdicts)[row_of], np.array(seeds, dtype=np.uint64)[row_of]
        for k in range(4):
            out["n_seeds"][:, k] = np.bincount(inv[vd == k], minlength=len(uniq))
        np.add.at(out["n_total"], inv, count)                                         # (uint64 sums: exact)
        out["first_seed"] = np.uint64(A.U64_MAX)
        np.minimum.at(out["first_seed"], inv, sd)
        np.maximum.at(out["max_per_seed"], inv, count)
    return Ref(out, n_counted, n_silent, int(n_truncated), int(n_observations), len(runner), sorted(runner))


def census_of_lists(obs_lists, verdicts, seeds, include, obs_cap):
    """The same from Python lists of observations (as oracle.observe_seed returns them), one per seed."""
    width = max([1] + [min(len(o), obs_cap) for o in obs_lists])
    rows = np.zeros((len(obs_lists), width), dtype=np.uint64)
    for i, o in enumerate(obs_lists):
        k = min(len(o), width)
        rows[i, :k] = np.array([int(x) for x in o[:k]], dtype=np.uint64)
    res = np.zeros(len(obs_lists), dtype=A.RESULT_DTYPE)
    res["verdict"] = verdicts
    return census(rows, [len(o) for o in obs_lists], res, seeds, include, obs_cap)


def census_by_dict(obs_lists, verdicts, seeds, include, obs_cap):
    """The definition once more, with a dict and no numpy: {value: [n_seeds[4], n_total, first_seed, max_per_seed]} and the totals —
    what the tests hold census() against on small inputs."""
    table, n_counted, n_silent, n_truncated, n_observations, runner = {}, [0] * 4, [0] * 4, 0, 0, []
    for o, v, s in zip(obs_lists, verdicts, seeds):
        if v >= 4:
            runner.append(int(s))
            continue
        if not (include >> v) & 1:
            continue
        seen = [int(x) for x in o[:obs_cap]]
        n_counted[v] += 1
        n_silent[v] += not seen
        n_truncated += len(o) > obs_cap
        n_observations += len(seen)
        for x in set(seen):
            e = table.setdefault(x, [[0] * 4, 0, int(s), 0])
            e[0][v] += 1
            e[1] += seen.count(x)
            e[2] = min(e[2], int(s))
            e[3] = max(e[3], seen.count(x))
    return table, tuple(n_counted), tuple(n_silent), n_truncated, n_observations, sorted(runner)
