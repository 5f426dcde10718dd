"""The probe-order census (include/madsim_hip.h, madsim_hip_probe_order_range) restated in plain numpy and Python ints, from what
madsim_hip_trace_seeds returns: observation rows uint64[n, >= obs_cap], the TRUE lengths, the results and the seeds.  Test-only: the truth
tests/test_probe_order*.py hold the kernels, the host fold and the public calls against.  Whatever a row holds at or behind
min(len, obs_cap) is ignored."""
import numpy as np

from madsim_amd import _abi as A

UNDEF = np.iinfo(np.int64).max


class Ref:
    """`pairs` ndarray[A.PROBE_ORDER_PAIR_DTYPE] ascending by (a, b), `n_counted` / `n_none` 4-tuples of Python ints, `runner_seeds` ascending."""

    def __init__(self, pairs, n_counted, n_none, n_truncated, n_runner, runner_seeds):
        self.pairs, self.n_counted, self.n_none = pairs, tuple(int(x) for x in n_counted), tuple(int(x) for x in n_none)
        self.n_truncated, self.n_runner, self.runner_seeds = int(n_truncated), int(n_runner), runner_seeds

    def tobytes(self):
        """As runtime.ProbeOrder.tobytes lays it out."""
        totals = np.array(self.n_counted + self.n_none + (self.n_truncated, self.n_runner), dtype=np.uint64)
        return self.pairs.tobytes() + totals.tobytes() + np.asarray(self.runner_seeds, dtype=np.uint64).tobytes()

    def words(self):
        """The chunk's words as the device writes them (csrc/sim_kernel.h)."""
        w = np.zeros(12, dtype=np.uint64)
        w[0], w[2:6], w[6:10], w[10], w[11] = len(self.pairs), self.n_counted, self.n_none, self.n_truncated, self.n_runner
        return w


def firsts(rows, lens, vocab, obs_cap):
    """first(j) of every row (counted or not), int64[n, m], UNDEF where vocab[j] is not visible."""
    rows, lens = np.asarray(rows, dtype=np.uint64), np.asarray(lens, dtype=np.uint64)
    assert 1 <= len(vocab) <= A.PROBE_ORDER_MAX_VOCAB and len(set(int(v) for v in vocab)) == len(vocab)
    vis = np.minimum(lens, np.uint64(obs_cap)).astype(np.int64)
    assert rows.shape[1] >= int(vis.max(initial=0))
    visible = np.arange(rows.shape[1])[None, :] < vis[:, None]
    out = np.full((len(rows), len(vocab)), UNDEF, dtype=np.int64)
    for j, v in enumerate(vocab):
        hit = (rows == np.uint64(int(v))) & visible
        out[:, j] = np.where(hit.any(axis=1), hit.argmax(axis=1), UNDEF)
    return out


def fold(first, lens, verdicts, seeds, include, obs_cap):
    """The report of per-seed first-occurrence rows (only those of counted seeds are looked at), true lengths, verdicts and seeds (any
    order, distinct)."""
    first, lens = np.asarray(first, dtype=np.int64), np.asarray(lens, dtype=np.uint64)
    verdicts, seeds = np.asarray(verdicts, dtype=np.uint64), np.asarray(seeds, dtype=np.uint64)
    m = first.shape[1]
    runner = verdicts >= 4
    counted = ~runner & (((np.uint64(include) >> np.minimum(verdicts, np.uint64(63))) & np.uint64(1)) == 1)
    f, vd, sd = first[counted], verdicts[counted], seeds[counted]
    have = f != UNDEF
    rel = have[:, :, None] & have[:, None, :] & (f[:, :, None] < f[:, None, :])      # [seed, a, b]: both defined, a first
    rel[:, np.arange(m), np.arange(m)] = have
    n_seeds, first_seed = np.zeros((m, m, 4), dtype=np.uint64), np.zeros((m, m, 4), dtype=np.uint64)
    for k in range(4):
        r = rel[vd == k]
        n_seeds[:, :, k] = r.sum(axis=0)
        s = np.where(r, sd[vd == k][:, None, None], np.uint64(A.U64_MAX))
        first_seed[:, :, k] = np.where(n_seeds[:, :, k] > 0, s.min(axis=0, initial=np.uint64(A.U64_MAX)), np.uint64(0))
    a, b = np.nonzero(n_seeds.any(axis=2))                                           # row-major: ascending by (a, b)
    out = np.zeros(len(a), dtype=A.PROBE_ORDER_PAIR_DTYPE)
    out["a"], out["b"], out["n_seeds"], out["first_seed"] = a, b, n_seeds[a, b], first_seed[a, b]
    n_counted = tuple(int((vd == k).sum()) for k in range(4))
    n_none = tuple(int(((vd == k) & ~have.any(axis=1)).sum()) for k in range(4))
    return Ref(out, n_counted, n_none, int((lens[counted] > np.uint64(obs_cap)).sum()), int(runner.sum()), sorted(int(s) for s in seeds[runner]))


def probe_order(rows, lens, results, seeds, include, obs_cap, vocab):
    """The report of the seeds `seeds`.  rows: uint64[n, c] with c >= min(len, obs_cap) for every row, lens: n true lengths, results:
    ndarray[A.RESULT_DTYPE] or anything with a "verdict" column, include: the bit mask, vocab: the vocabulary."""
    return fold(firsts(rows, lens, vocab, obs_cap), lens, results["verdict"], seeds, include, obs_cap)


def probe_order_of_lists(obs_lists, verdicts, seeds, include, obs_cap, vocab):
    """The same from Python lists of observations (as oracle.observe_seed returns them), one per seed."""
    width = max([1] + [min(len(o), obs_cap) for o in obs_lists])
    rows = np.zeros((len(obs_lists), width), dtype=np.uint64)
    for i, o in enumerate(obs_lists):
        k = min(len(o), width)
        rows[i, :k] = np.array([int(x) for x in o[:k]], dtype=np.uint64)
    res = np.zeros(len(obs_lists), dtype=A.RESULT_DTYPE)
    res["verdict"] = verdicts
    return probe_order(rows, [len(o) for o in obs_lists], res, seeds, include, obs_cap, vocab)


def seed_firsts(o, obs_cap, vocab):
    """The definition once more for one seed: {vocabulary index: first(index)} of the values visible, with list.index and no numpy."""
    seen = [int(x) for x in o[:obs_cap]]
    return {j: seen.index(int(v)) for j, v in enumerate(vocab) if int(v) in seen}


def probe_order_by_dict(obs_lists, verdicts, seeds, include, obs_cap, vocab):
    """({(a, b): [n_seeds[4], first_seed[4]]}, n_counted, n_none, n_truncated, sorted runner seeds) with a dict and no numpy — what the
    tests hold probe_order() against on small inputs."""
    table, n_counted, n_none, n_truncated, runner = {}, [0] * 4, [0] * 4, 0, []
    for o, v, s in zip(obs_lists, verdicts, seeds):
        if v >= 4:
            runner.append(int(s))
            continue
        if not (include >> v) & 1:
            continue
        n_counted[v] += 1
        n_truncated += len(o) > obs_cap
        f = seed_firsts(o, obs_cap, vocab)
        n_none[v] += not f
        for a in f:
            for b in f:
                if a == b or f[a] < f[b]:
                    e = table.setdefault((a, b), [[0] * 4, [0] * 4])
                    e[1][v] = int(s) if not e[0][v] else min(e[1][v], int(s))
                    e[0][v] += 1
    return table, tuple(n_counted), tuple(n_none), n_truncated, sorted(runner)
