"""The host-side truth of a statistics campaign (madsim_hip_run_campaign_stats): a filter, a lexsort and a bincount over per-seed results.
Shared by tests/test_campaign_stats.py (which tests it, and the fold of per-batch truths) and tests/test_campaign_stats_gpu.py (which holds
the GPU's answer against it) — a plain restatement of include/madsim_hip.h, independent of the library and of madsim_amd/_abi.py's helpers."""
import functools
import math

import numpy as np

import oracle
from madsim_amd import _abi as A
from madsim_amd import workload as W

U64_MAX = (1 << 64) - 1
METRICS = ("clock_ns", "steps", "msg_count", "rng_calls")          # MADSIM_STAT_CLOCK, _STEPS, _MSGS, _RNG
N_BUCKETS = 256
SEED0, TOTAL = 5_000_000, 40_000                                    # the lossy ping-pong range of tests/test_collect_gpu.py


def bucket(v):
    v = int(v)
    if v < 4:
        return v
    e = v.bit_length() - 1
    return 4 * (e - 1) + ((v >> (e - 2)) & 3)


def bucket_floor(b):
    if b < 4:
        return b
    return U64_MAX if b >= 252 else (4 + b % 4) << (b // 4 - 1)


def buckets(v):
    """bucket() over a uint64 array, in integer arithmetic (no float logarithm)."""
    v = np.asarray(v, dtype=np.uint64)
    e = np.zeros(len(v), dtype=np.uint64)
    t = v.copy()
    for s in (32, 16, 8, 4, 2, 1):
        big = t >> np.uint64(s) != 0
        e[big] += np.uint64(s)
        t[big] >>= np.uint64(s)
    shift = np.where(e >= 2, e - np.uint64(2), np.uint64(0)).astype(np.uint64)
    b = np.uint64(4) * (np.maximum(e, np.uint64(1)) - np.uint64(1)) + ((v >> shift) & np.uint64(3))
    return np.where(v < 4, v, b).astype(np.int64)


def mask(*verdicts):
    m = 0
    for v in verdicts:
        m |= 1 << v
    return m


def stats_truth(results, seed0, include, top_k):
    """{n, n_top, metric name: {min, max, sum, hist, top}} of per-seed `results` of [seed0, seed0 + len): top = [(value, seed)] in order."""
    verdict = results["verdict"]
    counted = (verdict < 4) & (((include >> np.minimum(verdict, 31)) & 1) != 0)
    idx = np.nonzero(counted)[0]
    seeds = seed0 + idx.astype(np.uint64)
    n = len(idx)
    out = {"n": n, "n_top": min(top_k, n)}
    for name in METRICS:
        v = results[name][idx].astype(np.uint64)
        order = np.lexsort((seeds, ~v))[:top_k]           # value descending, then seed ascending
        # the sum as two half-sums in uint64 (exact below 2^32 seeds; tests/test_report_kernels.py holds it against plain Python ints)
        halves = (int((v & np.uint64(0xffffffff)).sum(dtype=np.uint64)), int((v >> np.uint64(32)).sum(dtype=np.uint64)))
        out[name] = {
            "min": int(v.min()) if n else U64_MAX, "max": int(v.max()) if n else 0,
            "sum": halves[0] + (halves[1] << 32), "halves": halves,
            "hist": np.bincount(buckets(v), minlength=N_BUCKETS).astype(np.uint64),
            "top": [(int(v[i]), int(seeds[i])) for i in order],
        }
    return out


def fold(truths, top_k):
    """The truth of a range from the truths of the batches it was cut into (the host fold of the library, restated)."""
    out = {"n": sum(t["n"] for t in truths)}
    out["n_top"] = min(top_k, out["n"])
    for name in METRICS:
        top = sorted((e for t in truths for e in t[name]["top"]), key=lambda e: (-e[0], e[1]))[:top_k]
        out[name] = {
            "min": min([t[name]["min"] for t in truths] + [U64_MAX]), "max": max([t[name]["max"] for t in truths] + [0]),
            "sum": sum(t[name]["sum"] for t in truths),
            "hist": sum((t[name]["hist"] for t in truths), np.zeros(N_BUCKETS, dtype=np.uint64)),
            "top": top,
        }
    return out


def same(a, b):
    return a["n"] == b["n"] and a["n_top"] == b["n_top"] and all(
        a[m][f] == b[m][f] for m in METRICS for f in ("min", "max", "sum", "top")) and all((a[m]["hist"] == b[m]["hist"]).all() for m in METRICS)


def quantile_bounds(truth, name, q):
    """(lo, hi) of the bucket that holds the element of rank ceil(q * n), clipped to [min, max] — from the truth's histogram."""
    rank = min(max(math.ceil(q * truth["n"]), 1), truth["n"])
    b = int(np.nonzero(np.cumsum(truth[name]["hist"]) >= rank)[0][0])
    hi = U64_MAX if b >= 251 else bucket_floor(b + 1) - 1
    return max(bucket_floor(b), truth[name]["min"]), min(hi, truth[name]["max"])


def of_stats(stats):
    """A runtime.CampaignStats in the shape of stats_truth's answer."""
    out = {"n": stats.n, "n_top": stats.n_top}
    for name in METRICS:
        t = stats.top(name)
        out[name] = {"min": stats.min[name], "max": stats.max[name], "sum": stats.sum[name], "hist": stats.hist[name],
                     "top": [(int(v), int(s)) for v, s in zip(t["value"], t["seed"])]}
    return out


@functools.lru_cache(maxsize=None)
def lossy_pingpong():
    """(workload, config, the oracle's results — read-only) of the 40 000 lossy ping-pong seeds: 35 330 pass, 4 670 deadlock."""
    w, cfg = W.pingpong(4, 16), A.Config.default(packet_loss_rate=0.002)
    want, _ = oracle.run_batch(w, SEED0, TOTAL, cfg)
    want.setflags(write=False)
    return w, cfg, want
