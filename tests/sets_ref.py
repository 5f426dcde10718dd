"""The probe-set census (include/madsim_hip.h, madsim_hip_probe_sets_range) restated in plain numpy and Python ints, from what
madsim_hip_trace_seeds returns: observation rows uint64[n, >= obs_cap], the TRUE lengths, the results and the seeds.  Test-only: the truth
tests/test_probe_sets*.py hold the kernels, the host fold and the public calls against.  Whatever a row holds at or behind
min(len, obs_cap) is ignored."""
import numpy as np

from madsim_amd import _abi as A

OTHER, TRUNCATED = 1 << 62, 1 << 63


class Ref:
    """`sets` ndarray[A.PROBE_SET_DTYPE] ascending by set word, `n_counted` a 4-tuple of Python ints, `runner_seeds` ascending."""

    def __init__(self, sets, n_counted, n_runner, runner_seeds):
        self.sets, self.n_counted, self.n_runner, self.runner_seeds = sets, tuple(int(x) for x in n_counted), int(n_runner), runner_seeds

    def tobytes(self):
        """As runtime.ProbeSets.tobytes lays it out."""
        totals = np.array(self.n_counted + (self.n_runner,), dtype=np.uint64)
        return self.sets.tobytes() + totals.tobytes() + np.asarray(self.runner_seeds, dtype=np.uint64).tobytes()


def set_words(rows, lens, vocab, obs_cap):
    """The set word of every row (counted or not), uint64[n]: rows uint64[n, c], the true lengths, the vocabulary."""
    rows, lens = np.asarray(rows, dtype=np.uint64), np.asarray(lens, dtype=np.uint64)
    assert 1 <= len(vocab) <= 62 and len(set(int(v) for v in vocab)) == len(vocab)
    vis = np.minimum(lens, np.uint64(obs_cap)).astype(np.int64)
    assert rows.shape[1] >= int(vis.max(initial=0))
    visible = np.arange(rows.shape[1])[None, :] < vis[:, None]
    words, known = np.zeros(len(rows), dtype=np.uint64), np.zeros(rows.shape, dtype=bool)
    for j, v in enumerate(vocab):
        hit = (rows == np.uint64(int(v))) & visible
        known |= hit
        words[hit.any(axis=1)] |= np.uint64(1 << j)
    words[(visible & ~known).any(axis=1)] |= np.uint64(OTHER)
    words[lens > np.uint64(obs_cap)] |= np.uint64(TRUNCATED)
    return words


def fold(words, verdicts, seeds, include):
    """The report of per-seed set words (only those of counted seeds are looked at), verdicts and seeds (any order, distinct)."""
    words, verdicts, seeds = np.asarray(words, dtype=np.uint64), np.asarray(verdicts, dtype=np.uint64), np.asarray(seeds, dtype=np.uint64)
    runner = verdicts >= 4
    counted = ~runner & (((np.uint64(include) >> np.minimum(verdicts, np.uint64(63))) & np.uint64(1)) == 1)
    uniq, inv = np.unique(words[counted], return_inverse=True)
    out = np.zeros(len(uniq), dtype=A.PROBE_SET_DTYPE)
    out["set"] = uniq
    vd, sd = verdicts[counted], seeds[counted]
    for k in range(4):
        out["n_seeds"][:, k] = np.bincount(inv[vd == k], minlength=len(uniq))
        first = np.full(len(uniq), A.U64_MAX, dtype=np.uint64)
        np.minimum.at(first, inv[vd == k], sd[vd == k])
        out["first_seed"][:, k] = np.where(out["n_seeds"][:, k] > 0, first, np.uint64(0))
    n_counted = tuple(int((vd == k).sum()) for k in range(4))
    return Ref(out, n_counted, int(runner.sum()), sorted(int(s) for s in seeds[runner]))


def probe_sets(rows, lens, results, seeds, include, obs_cap, vocab):
    """The report of the seeds `seeds`.  rows: uint64[n, c] with c >= min(len, obs_cap) for every row, lens: n true lengths, results:
    ndarray[A.RESULT_DTYPE] or anything with a "verdict" column, include: the bit mask, vocab: the vocabulary."""
    return fold(set_words(rows, lens, vocab, obs_cap), results["verdict"], seeds, include)


def probe_sets_of_lists(obs_lists, verdicts, seeds, include, obs_cap, vocab):
    """The same from Python lists of observations (as oracle.observe_seed returns them), one per seed."""
    width = max([1] + [min(len(o), obs_cap) for o in obs_lists])
    rows = np.zeros((len(obs_lists), width), dtype=np.uint64)
    for i, o in enumerate(obs_lists):
        k = min(len(o), width)
        rows[i, :k] = np.array([int(x) for x in o[:k]], dtype=np.uint64)
    res = np.zeros(len(obs_lists), dtype=A.RESULT_DTYPE)
    res["verdict"] = verdicts
    return probe_sets(rows, [len(o) for o in obs_lists], res, seeds, include, obs_cap, vocab)


def seed_set_word(o, obs_cap, vocab):
    """The definition once more for one seed, with a Python set and no numpy."""
    seen, vocab = set(int(x) for x in o[:obs_cap]), [int(v) for v in vocab]
    word = sum(1 << j for j, v in enumerate(vocab) if v in seen)
    return word | (OTHER if seen - set(vocab) else 0) | (TRUNCATED if len(o) > obs_cap else 0)


def probe_sets_by_dict(obs_lists, verdicts, seeds, include, obs_cap, vocab):
    """({set word: [n_seeds[4], first_seed[4]]}, n_counted, sorted runner seeds) with a dict and no numpy — what the tests hold
    probe_sets() against on small inputs."""
    table, n_counted, runner = {}, [0] * 4, []
    for o, v, s in zip(obs_lists, verdicts, seeds):
        if v >= 4:
            runner.append(int(s))
            continue
        if not (include >> v) & 1:
            continue
        n_counted[v] += 1
        e = table.setdefault(seed_set_word(o, obs_cap, vocab), [[0] * 4, [0] * 4])
        e[1][v] = int(s) if not e[0][v] else min(e[1][v], int(s))
        e[0][v] += 1
    return table, tuple(n_counted), sorted(runner)
