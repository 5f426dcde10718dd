"""The host-side truth of a paired campaign (madsim_hip_run_paired_campaign): a classification, a subtraction, a lexsort and a bincount over
two arrays of per-seed results.  Shared by tests/test_campaign_paired.py (which holds its arithmetic against plain-Python loops, and the
library's host fold against it), tests/test_paired_kernels.py and tests/test_campaign_paired_gpu.py (which hold the GPU's answers against
it) — a plain restatement of include/madsim_hip.h, independent of the library and of madsim_amd/_abi.py's helpers."""
import numpy as np

from tests.stats_ref import METRICS, N_BUCKETS, U64_MAX, buckets

UP, DOWN = 0, 1                                                    # MADSIM_PAIRED_UP, MADSIM_PAIRED_DOWN
HEAD_WORDS, MAX_TOP = 58, 16                                       # MADSIM_K_PAIRED_HEAD_WORDS, MADSIM_STAT_MAX_TOP
WORDS = HEAD_WORDS + 8 * N_BUCKETS // 2 + 8 * MAX_TOP * 3          # MADSIM_K_PAIRED_WORDS
LOW = np.uint64(0xffffffff)


def _halves(v):
    """(sum of the low halves, sum of the high halves) of a uint64 array, each in uint64: exact below 2^32 elements."""
    return int((v & LOW).sum(dtype=np.uint64)), int((v >> np.uint64(32)).sum(dtype=np.uint64))


def classify(a, b, include_a, include_b):
    """(paired, incomparable): boolean arrays over the seeds of the result arrays `a` and `b`."""
    va, vb = a["verdict"].astype(np.uint64), b["verdict"].astype(np.uint64)
    inc = (va >= 4) | (vb >= 4)
    ok_a = ((np.uint64(include_a) >> np.minimum(va, np.uint64(31))) & np.uint64(1)) != 0
    ok_b = ((np.uint64(include_b) >> np.minimum(vb, np.uint64(31))) & np.uint64(1)) != 0
    return ~inc & ok_a & ok_b, inc


def paired_truth(a, b, seeds, include_a, include_b, top_k):
    """The report over the result arrays `a` and `b` of the seeds `seeds` (a uint64 array, or seed0 for a range):
    {n_paired, n_unpaired, n_incomparable, metric name: {n_equal, sum_a, sum_b, halves_a, halves_b,
    dir: [{n, min, max, sum, halves, hist, top: [(seed, a, b)] in order}] * 2}}."""
    count = len(a)
    if not isinstance(seeds, np.ndarray):
        seeds = (np.uint64(seeds) + np.arange(count, dtype=np.uint64)).astype(np.uint64)
    paired, inc = classify(a, b, include_a, include_b)
    idx = np.nonzero(paired)[0]
    s = seeds[idx]
    out = {"n_paired": len(idx), "n_incomparable": int(inc.sum()), "n_unpaired": count - len(idx) - int(inc.sum())}
    for name in METRICS:
        x, y = a[name][idx].astype(np.uint64), b[name][idx].astype(np.uint64)
        ha, hb = _halves(x), _halves(y)
        m = {"n_equal": int((x == y).sum()), "halves_a": ha, "halves_b": hb, "sum_a": ha[0] + (ha[1] << 32), "sum_b": hb[0] + (hb[1] << 32), "dir": []}
        for d in (UP, DOWN):
            on = y > x if d == UP else x > y
            mag = (y[on] - x[on]) if d == UP else (x[on] - y[on])             # unsigned: never wraps where `on`
            sd, xd, yd = s[on], x[on], y[on]
            order = np.lexsort((sd, ~mag))[:top_k]                           # magnitude descending, then seed ascending
            h = _halves(mag)
            m["dir"].append({
                "n": int(on.sum()), "min": int(mag.min()) if len(mag) else U64_MAX, "max": int(mag.max()) if len(mag) else 0,
                "sum": h[0] + (h[1] << 32), "halves": h, "hist": np.bincount(buckets(mag), minlength=N_BUCKETS).astype(np.uint64),
                "top": [(int(sd[i]), int(xd[i]), int(yd[i])) for i in order],
            })
        out[name] = m
    return out


def _mag(e, d):
    return e[2] - e[1] if d == UP else e[1] - e[2]


def fold(truths, top_k):
    """The truth of a seed set from the truths of the batches it was cut into (the host fold of the library, restated)."""
    out = {k: sum(t[k] for t in truths) for k in ("n_paired", "n_unpaired", "n_incomparable")}
    for name in METRICS:
        m = {k: sum(t[name][k] for t in truths) for k in ("n_equal", "sum_a", "sum_b")}
        m["dir"] = []
        for d in (UP, DOWN):
            parts = [t[name]["dir"][d] for t in truths]
            m["dir"].append({
                "n": sum(p["n"] for p in parts), "min": min([p["min"] for p in parts] + [U64_MAX]), "max": max([p["max"] for p in parts] + [0]),
                "sum": sum(p["sum"] for p in parts), "hist": sum((p["hist"] for p in parts), np.zeros(N_BUCKETS, dtype=np.uint64)),
                "top": sorted((e for p in parts for e in p["top"]), key=lambda e: (-_mag(e, d), e[0]))[:top_k],
            })
        out[name] = m
    return out


def words_of(truth, top_k):
    """A batch's truth as the MADSIM_K_PAIRED_WORDS the report kernels leave (csrc/sim_kernel.h): uint64[WORDS]."""
    w = np.zeros(WORDS, dtype=np.uint64)
    w[0], w[1] = truth["n_paired"], truth["n_incomparable"]
    hist = np.zeros((8, N_BUCKETS), dtype=np.uint32)
    top = np.zeros((8, MAX_TOP, 3), dtype=np.uint64)
    for m, name in enumerate(METRICS):
        M = truth[name]
        w[42 + m], w[46 + m] = M["halves_a"]
        w[50 + m], w[54 + m] = M["halves_b"]
        for d in (UP, DOWN):
            j, D = 2 * m + d, M["dir"][d]
            w[2 + j] = D["n"]
            w[10 + j] = U64_MAX - D["min"]                                   # kept inverted: zero when there is none
            w[18 + j] = D["max"]
            w[26 + j], w[34 + j] = D["halves"]
            hist[j] = D["hist"]
            for r, e in enumerate(D["top"][:top_k]):
                top[j, r] = e
    w[HEAD_WORDS:HEAD_WORDS + 8 * N_BUCKETS // 2] = hist.reshape(-1).view(np.uint64)
    w[HEAD_WORDS + 8 * N_BUCKETS // 2:] = top.reshape(-1)
    return w


def of_words(w, count, top_k):
    """The reverse of words_of, for a batch of `count` seeds: what the device words say, in the shape of paired_truth's answer (without the
    half-sums' split)."""
    w = np.asarray(w, dtype=np.uint64)
    hist = w[HEAD_WORDS:HEAD_WORDS + 8 * N_BUCKETS // 2].view(np.uint32).reshape(8, N_BUCKETS)
    top = w[HEAD_WORDS + 8 * N_BUCKETS // 2:].reshape(8, MAX_TOP, 3)
    out = {"n_paired": int(w[0]), "n_incomparable": int(w[1]), "n_unpaired": count - int(w[0]) - int(w[1])}
    for m, name in enumerate(METRICS):
        M = {"n_equal": int(w[0]) - int(w[2 + 2 * m]) - int(w[3 + 2 * m]), "sum_a": int(w[42 + m]) + (int(w[46 + m]) << 32),
             "sum_b": int(w[50 + m]) + (int(w[54 + m]) << 32), "dir": []}
        for d in (UP, DOWN):
            j = 2 * m + d
            n = int(w[2 + j])
            M["dir"].append({"n": n, "min": U64_MAX - int(w[10 + j]), "max": int(w[18 + j]), "sum": int(w[26 + j]) + (int(w[34 + j]) << 32),
                             "hist": hist[j].astype(np.uint64), "top": [tuple(int(x) for x in top[j, r]) for r in range(min(top_k, n))]})
        out[name] = M
    return out


def of_struct(pr, top):
    """A filled A.Paired and its top array (ndarray[PAIRED_EXTREME_DTYPE] of shape (4, 2, top_k)) in the shape of paired_truth's answer."""
    out = {"n_paired": int(pr.n_paired), "n_unpaired": int(pr.n_unpaired), "n_incomparable": int(pr.n_incomparable)}
    for m, name in enumerate(METRICS):
        M = {"n_equal": int(pr.n_equal[m]), "sum_a": (int(pr.sum_a_hi[m]) << 64) | int(pr.sum_a_lo[m]),
             "sum_b": (int(pr.sum_b_hi[m]) << 64) | int(pr.sum_b_lo[m]), "dir": []}
        for d in (UP, DOWN):
            j = 2 * m + d
            D = pr.delta[j]
            M["dir"].append({"n": int(pr.n[j]), "min": int(D.min), "max": int(D.max), "sum": (int(D.sum_hi) << 64) | int(D.sum_lo),
                             "hist": np.ctypeslib.as_array(D.hist).astype(np.uint64),
                             "top": [(int(e["seed"]), int(e["a"]), int(e["b"])) for e in top[m, d, :int(pr.n_top[j])]]})
        out[name] = M
    return out


def of_report(p):
    """A runtime.CampaignPaired in the shape of paired_truth's answer."""
    out = {"n_paired": p.n_paired, "n_unpaired": p.n_unpaired, "n_incomparable": p.n_incomparable}
    for name in METRICS:
        M = {"n_equal": p.n_equal[name], "sum_a": p.sum_a[name], "sum_b": p.sum_b[name], "dir": []}
        for d, rows in ((UP, p.regressions(name)), (DOWN, p.improvements(name))):
            M["dir"].append({"n": p.n[name][d], "min": p.min[name][d], "max": p.max[name][d], "sum": p.sum[name][d], "hist": p.hist[name][d],
                             "top": [(int(e["seed"]), int(e["a"]), int(e["b"])) for e in rows]})
        out[name] = M
    return out


def differences(got, want):
    """The paths at which two answers differ ([] = the same): every count, sum, bound, bucket and top entry."""
    bad = [k for k in ("n_paired", "n_unpaired", "n_incomparable") if got[k] != want[k]]
    for name in METRICS:
        bad += [f"{name}.{k}" for k in ("n_equal", "sum_a", "sum_b") if got[name][k] != want[name][k]]
        for d in (UP, DOWN):
            g, t = got[name]["dir"][d], want[name]["dir"][d]
            bad += [f"{name}.{'up' if d == UP else 'down'}.{k}" for k in ("n", "min", "max", "sum", "top") if g[k] != t[k]]
            if not (np.asarray(g["hist"]) == np.asarray(t["hist"])).all():
                bad.append(f"{name}.{'up' if d == UP else 'down'}.hist")
    return bad
