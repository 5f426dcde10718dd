"""Probe spans (include/madsim_hip.h, madsim_hip_probe_spans_range) restated in numpy, from what madsim_hip_timeline_seeds returns:
observation rows and time rows uint64[n, >= obs_cap], the TRUE lengths, the results' verdicts and the seeds — and a second time in dicts
and Python ints straight from the definition (report_of_lists), which tests/test_spans.py holds the first against.  Test-only: the truth
the kernels, the host fold and the public calls are held against.  Whatever a row holds at or behind min(len, obs_cap) is ignored."""
import numpy as np

from madsim_amd import _abi as A

U64 = (1 << 64) - 1
ABSENT, CLOSED, OPEN, CUT, UNCOUNTED = A.SPAN_ABSENT, A.SPAN_CLOSED, A.SPAN_OPEN, A.SPAN_CUT, 4


class Ref:
    """`defs` ndarray[A.SPAN_DEF_DTYPE], `spans` ndarray[A.SPAN_DTYPE], `n_counted` a 4-tuple of Python ints, `runner_seeds` ascending."""

    def __init__(self, defs, spans, n_counted, n_truncated, n_runner, runner_seeds):
        self.defs, self.spans, self.n_counted = defs, spans, tuple(int(x) for x in n_counted)
        self.n_truncated, self.n_runner, self.runner_seeds = int(n_truncated), int(n_runner), runner_seeds

    def tobytes(self):
        """As runtime.ProbeSpans.tobytes lays it out."""
        totals = np.array(self.n_counted + (self.n_truncated, self.n_runner), dtype=np.uint64)
        return self.defs.tobytes() + self.spans.tobytes() + totals.tobytes() + np.asarray(self.runner_seeds, dtype=np.uint64).tobytes()

    def words(self):
        """The chunk's words as the device writes them (csrc/sim_kernel.h)."""
        w = np.zeros(8, dtype=np.uint64)
        w[0], w[2:6], w[6], w[7] = len(self.spans), self.n_counted, self.n_truncated, self.n_runner
        return w

    def records(self):
        """The chunk's records as the device writes them (csrc/sim_kernel.h), uint64[n_spans, 280]: ~min, the two half-sums, ~seed."""
        out = np.zeros((len(self.spans), A.SPAN_REC_WORDS), dtype=np.uint64)
        for s, sp in enumerate(self.spans):
            out[s, 0:16] = sp["n_state"].reshape(-1)
            n = int(sp["n"])
            if n:
                total = int(sp["sum_hi"]) << 64 | int(sp["sum_lo"])
                hi = min(total >> 32, n * 0xffffffff)          # one of the splits into half-sums a device can produce: any is the same sum
                lo = total - (hi << 32)
                assert 0 <= lo <= n * 0xffffffff and 0 <= hi <= n * 0xffffffff and lo + (hi << 32) == total
                out[s, 16:23] = (n, U64 ^ int(sp["min"]), int(sp["max"]), lo, hi, U64 ^ int(sp["min_seed"]), U64 ^ int(sp["max_seed"]))
            if int(sp["n_state"][:, OPEN].sum()):
                out[s, 23] = U64 ^ int(sp["first_open_seed"])
            out[s, 24:] = sp["hist"]
        return out


def defs_of(spans):
    """ndarray[A.SPAN_DEF_DTYPE] of (from, to) pairs, from=None for the start of the run (runtime.span_defs, without the library)."""
    d = np.zeros(len(spans), dtype=A.SPAN_DEF_DTYPE)
    for k, (a, b) in enumerate(spans):
        d[k] = (0 if a is None else int(a), int(b), A.SPAN_FROM_START if a is None else 0, 0)
    return d


def states(rows, times, lens, defs, obs_cap):
    """(state int64[n, m], duration uint64[n, m]) of every row (counted or not), by the definition."""
    rows, times, lens = np.asarray(rows, dtype=np.uint64), np.asarray(times, dtype=np.uint64), np.asarray(lens, dtype=np.uint64)
    n, width = rows.shape
    vis = np.minimum(lens, np.uint64(obs_cap)).astype(np.int64)
    assert width >= int(vis.max(initial=0)) and times.shape == rows.shape
    col = np.arange(width)[None, :]
    visible = col < vis[:, None]
    cut = lens > np.uint64(obs_cap)
    st, du = np.zeros((n, len(defs)), dtype=np.int64), np.zeros((n, len(defs)), dtype=np.uint64)
    r = np.arange(n)
    for s, d in enumerate(defs):
        if int(d["flags"]) & A.SPAN_FROM_START:
            has_i, i, t_i = np.ones(n, dtype=bool), np.full(n, -1, dtype=np.int64), np.zeros(n, dtype=np.uint64)
        else:
            hit = (rows == np.uint64(int(d["from"]))) & visible
            has_i, i = hit.any(axis=1), hit.argmax(axis=1)
            t_i = times[r, i] if width else np.zeros(n, dtype=np.uint64)
        hit = (rows == np.uint64(int(d["to"]))) & visible & (col > i[:, None])
        has_j, j = has_i & hit.any(axis=1), hit.argmax(axis=1)
        st[:, s] = np.where(~has_i, ABSENT, np.where(has_j, CLOSED, np.where(cut, CUT, OPEN)))
        t_j = times[r, j] if width else np.zeros(n, dtype=np.uint64)
        du[:, s] = np.where(has_j, t_j - t_i, np.uint64(0))                            # (unsigned, wrapping as the device's subtraction does)
    return st, du


def fold(st, du, lens, verdicts, seeds, defs, include, obs_cap):
    """The report of per-seed states and durations (only those of counted seeds are looked at), true lengths, verdicts and seeds (any order)."""
    st, du, lens = np.asarray(st), np.asarray(du, dtype=np.uint64), np.asarray(lens, dtype=np.uint64)
    verdicts, seeds = np.asarray(verdicts, dtype=np.uint64), np.asarray(seeds, dtype=np.uint64)
    runner = verdicts >= 4
    counted = ~runner & (((np.uint64(include) >> np.minimum(verdicts, np.uint64(63))) & np.uint64(1)) == 1)
    spans = np.zeros(len(defs), dtype=A.SPAN_DTYPE)
    vd, sd = verdicts[counted].astype(np.int64), seeds[counted]
    for s in range(len(defs)):
        q, d = st[counted, s], du[counted, s]
        sp = spans[s]
        for v in range(4):
            sp["n_state"][v] = np.bincount(q[vd == v], minlength=4)[:4]
        c = q == CLOSED
        dc, sc = d[c], sd[c]
        sp["n"] = len(dc)
        sp["min"], sp["max"] = (dc.min(), dc.max()) if len(dc) else (U64, 0)
        sp["min_seed"] = sc[dc == dc.min()].min() if len(dc) else U64
        sp["max_seed"] = sc[dc == dc.max()].min() if len(dc) else U64
        total = int((dc & np.uint64(0xffffffff)).sum(dtype=np.uint64)) + (int((dc >> np.uint64(32)).sum(dtype=np.uint64)) << 32)
        sp["sum_lo"], sp["sum_hi"] = total & U64, total >> 64
        sp["hist"] = np.bincount([A.stat_bucket(int(x)) for x in dc], minlength=A.STAT_BUCKETS)
        o = sd[q == OPEN]
        sp["first_open_seed"] = o.min() if len(o) else U64
    n_counted = [int((vd == v).sum()) for v in range(4)]
    return Ref(defs, spans, n_counted, int((lens[counted] > np.uint64(obs_cap)).sum()), int(runner.sum()), np.sort(seeds[runner]))


def report(rows, times, lens, verdicts, seeds, spans, include=0xf, obs_cap=256):
    defs = defs_of(spans) if not isinstance(spans, np.ndarray) else spans
    st, du = states(rows, times, lens, defs, obs_cap)
    return fold(st, du, lens, verdicts, seeds, defs, include, obs_cap)


def pad(lists, width=None):
    """uint64[n, width] of lists of Python ints, zeros behind each, and their lengths."""
    width = max([len(x) for x in lists] + [1]) if width is None else width
    out = np.zeros((len(lists), width), dtype=np.uint64)
    for i, x in enumerate(lists):
        out[i, :min(len(x), width)] = np.array([int(v) for v in x[:width]], dtype=np.uint64)
    return out, np.array([len(x) for x in lists], dtype=np.uint64)


def report_of_lists(obs, times, verdicts, seeds, spans, include=0xf, obs_cap=256):
    """The second statement: dicts and Python ints, seed by seed from the definition; returns the same Ref."""
    defs = defs_of(spans)
    recs = [dict(n_state=[[0] * 4 for _ in range(4)], d=[], open=[]) for _ in spans]
    n_counted, n_trunc, runner = [0] * 4, 0, []
    for o, t, v, seed in zip(obs, times, verdicts, seeds):
        v, seed = int(v), int(seed)
        if v >= 4:
            runner.append(seed)
            continue
        if not (include >> v) & 1:
            continue
        n_counted[v] += 1
        n_trunc += len(o) > obs_cap
        vo, vt = [int(x) for x in o[:obs_cap]], [int(x) for x in t[:obs_cap]]
        for rec, (a, b) in zip(recs, spans):
            i = -1 if a is None else next((k for k, x in enumerate(vo) if x == int(a)), None)
            if i is None:
                rec["n_state"][v][ABSENT] += 1
                continue
            j = next((k for k in range(i + 1, len(vo)) if vo[k] == int(b)), None)
            if j is None:
                state = CUT if len(o) > obs_cap else OPEN
                rec["n_state"][v][state] += 1
                if state == OPEN:
                    rec["open"].append(seed)
                continue
            rec["n_state"][v][CLOSED] += 1
            rec["d"].append(((vt[j] - (0 if i < 0 else vt[i])) & U64, seed))
    out = np.zeros(len(spans), dtype=A.SPAN_DTYPE)
    for sp, rec in zip(out, recs):
        sp["n_state"] = rec["n_state"]
        d = rec["d"]
        sp["n"] = len(d)
        mn, mx = (min(x for x, _ in d), max(x for x, _ in d)) if d else (U64, 0)
        sp["min"], sp["max"] = mn, mx
        sp["min_seed"] = min(s for x, s in d if x == mn) if d else U64
        sp["max_seed"] = min(s for x, s in d if x == mx) if d else U64
        total = sum(x for x, _ in d)
        sp["sum_lo"], sp["sum_hi"] = total & U64, total >> 64
        hist = [0] * A.STAT_BUCKETS
        for x, _ in d:
            hist[A.stat_bucket(x)] += 1
        sp["hist"] = hist
        sp["first_open_seed"] = min(rec["open"]) if rec["open"] else U64
    return Ref(defs, out, n_counted, n_trunc, len(runner), np.array(sorted(runner), dtype=np.uint64))
