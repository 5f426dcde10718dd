"""Task post-mortems and the stall-site census (include/madsim_hip.h, madsim_hip_task_states / madsim_hip_stall_census_range) restated in
plain numpy and Python ints, from what madsim_hip_task_states returns: task rows uint64[n, >= task_cap], the TRUE counts, the results and
the seeds.  Test-only: the truth tests/test_stall*.py hold the kernels, the host fold and the public calls against.  Whatever a row holds
at or behind min(len, task_cap) is ignored."""
import numpy as np

from madsim_amd import _abi as A
from tests import census_ref

M64 = (1 << 64) - 1
PARKED, QUEUED, PANICKED, CANCELLED = 1, 2, 3, 4


def word(state, prog, pc, cnt0=0, cnt1=0):
    """bits 63-56 state | 55-48 prog | 47-32 pc | 31-16 cnt0 | 15-0 cnt1"""
    assert 1 <= state <= 255 and 0 <= prog <= 255 and 0 <= pc <= 0xFFFF and 0 <= cnt0 <= 0xFFFF and 0 <= cnt1 <= 0xFFFF
    return (state << 56) | (prog << 48) | (pc << 32) | (cnt0 << 16) | cnt1


def state(w):
    return int(w) >> 56


def prog(w):
    return (int(w) >> 48) & 0xFF


def pc(w):
    return (int(w) >> 32) & 0xFFFF


def cnt0(w):
    return (int(w) >> 16) & 0xFFFF


def cnt1(w):
    return int(w) & 0xFFFF


def site(w):
    """MADSIM_TASK_SITE: state | prog | pc"""
    return int(w) >> 32


def site_of(state_, prog_, pc_):
    return (state_ << 24) | (prog_ << 16) | pc_


def mix(z):
    """splitmix64's finaliser, as the header writes it out"""
    z &= M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def shape(records):
    """madsim_hip_stall_shape: the sum of mix(site) over the records, mod 2^64; 0 for none"""
    s = 0
    for w in records:
        s = (s + mix(site(w))) & M64
    return s


def sites_and_shapes(rows, lens, results, task_cap):
    """What stall_sites_kernel writes: (site rows uint64[n, task_cap], shape words uint64[n], ones uint64[n]).  The visible records of row i
    are the first min(len, task_cap); of a row with a runner verdict none."""
    rows = np.asarray(rows, dtype=np.uint64)
    n = rows.shape[0]
    out, shp = np.zeros((n, task_cap), dtype=np.uint64), np.zeros(n, dtype=np.uint64)
    for i in range(n):
        vis = min(int(lens[i]), task_cap) if int(results["verdict"][i]) < 4 else 0
        out[i, :vis] = rows[i, :vis] >> np.uint64(32)
        shp[i] = shape(rows[i, :vis])
    return out, shp, np.ones(n, dtype=np.uint64)


class Ref:
    """`sites` / `shapes` ndarray[A.CENSUS_VALUE_DTYPE] ascending by value, the totals as Python ints / 4-tuples, `runner_seeds` ascending."""

    def __init__(self, sites, shapes, n_counted, n_idle, n_truncated, n_tasks, n_runner, runner_seeds):
        self.sites, self.shapes, self.n_counted, self.n_idle = sites, shapes, tuple(n_counted), tuple(n_idle)
        self.n_truncated, self.n_tasks, self.n_runner, self.runner_seeds = n_truncated, n_tasks, n_runner, runner_seeds

    def tobytes(self):
        """As runtime.StallCensus.tobytes lays it out."""
        totals = np.array(self.n_counted + self.n_idle + (self.n_truncated, self.n_tasks, self.n_runner), dtype=np.uint64)
        return self.sites.tobytes() + self.shapes.tobytes() + totals.tobytes() + np.asarray(self.runner_seeds, dtype=np.uint64).tobytes()


def census(rows, lens, results, seeds, include, task_cap, want_shapes=True):
    """The stall census of the seeds `seeds` (any order, distinct): the observation census (tests/census_ref.py) over the site rows, and over
    the shape words as rows of one."""
    srows, shp, ones = sites_and_shapes(rows, lens, results, task_cap)
    a = census_ref.census(srows, lens, results, seeds, include, task_cap)
    b = census_ref.census(shp.reshape(-1, 1), ones, results, seeds, include, 1)
    shapes = b.values if want_shapes else np.zeros(0, dtype=A.CENSUS_VALUE_DTYPE)
    return Ref(a.values, shapes, a.n_counted, a.n_silent, a.n_truncated, a.n_observations, a.n_runner, a.runner_seeds)


def census_of_lists(tables, verdicts, seeds, include, task_cap, want_shapes=True):
    """The same from Python lists of task records, one per seed."""
    width = max([1, task_cap] + [len(t) for t in tables])
    rows = np.zeros((len(tables), width), dtype=np.uint64)
    for i, t in enumerate(tables):
        rows[i, :len(t)] = np.array([int(x) for x in t], dtype=np.uint64)
    res = np.zeros(len(tables), dtype=A.RESULT_DTYPE)
    res["verdict"] = verdicts
    return census(rows, [len(t) for t in tables], res, seeds, include, task_cap, want_shapes)


def census_by_dict(tables, verdicts, seeds, include, task_cap):
    """The definition once more, with dicts and no numpy: ({site: [n_seeds[4], n_total, first_seed, max_per_seed]}, {shape: [n_seeds[4],
    first_seed]}, n_counted, n_idle, n_truncated, n_tasks, runner seeds) — what the tests hold census() against on small inputs."""
    sites, shapes, n_counted, n_idle, n_truncated, n_tasks, runner = {}, {}, [0] * 4, [0] * 4, 0, 0, []
    for t, v, s in zip(tables, verdicts, seeds):
        if v >= 4:
            runner.append(int(s))
            continue
        if not (include >> v) & 1:
            continue
        seen = [site(x) for x in t[:task_cap]]
        n_counted[v] += 1
        n_idle[v] += not seen
        n_truncated += len(t) > task_cap
        n_tasks += len(seen)
        for x in set(seen):
            e = sites.setdefault(x, [[0] * 4, 0, int(s), 0])
            e[0][v] += 1
            e[1] += seen.count(x)
            e[2] = min(e[2], int(s))
            e[3] = max(e[3], seen.count(x))
        h = shapes.setdefault(shape(t[:task_cap]), [[0] * 4, int(s)])
        h[0][v] += 1
        h[1] = min(h[1], int(s))
    return sites, shapes, tuple(n_counted), tuple(n_idle), n_truncated, n_tasks, sorted(runner)
