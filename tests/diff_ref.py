"""The host-side truth of a differential campaign (madsim_hip_run_campaign_diff): given the per-seed results of the two sides, everything
madsim_diff_t holds afterwards — a plain numpy restatement of include/madsim_hip.h, independent of the library.  Shared by
tests/test_campaign_diff.py (which holds it against plain Python ints, and the library's host fold against it), tests/test_diff_kernels.py and
tests/test_campaign_diff_gpu.py (which hold the GPU's answers against it)."""
import functools

import numpy as np

import oracle
from madsim_amd import _abi as A
from madsim_amd import workload as W

U64_MAX = (1 << 64) - 1
FIELDS = ("verdict", "steps", "clock_ns", "msg_count", "rng_calls", "trace_hash", "obs_hash")      # bit i of the mask = FIELDS[i]
WIDE = FIELDS[2:]                                                                                # the 64-bit ones
ALL = 127
RUNNER = 4                                                                                       # verdicts at or above it are runner verdicts
WORDS = 74                                                                                       # MADSIM_K_DIFF_WORDS


def incomparable(a, b):
    return (a["verdict"] >= RUNNER) | (b["verdict"] >= RUNNER)


def masks(a, b, fields):
    """Per seed: the bits of `fields` whose field differs between the sides; 0 for an incomparable seed."""
    d = np.zeros(len(a), dtype=np.uint32)
    for i, name in enumerate(FIELDS):
        if fields >> i & 1:
            d |= (a[name] != b[name]).astype(np.uint32) << np.uint32(i)
    d[incomparable(a, b)] = 0
    return d


def transitions(a, b):
    t = np.zeros((8, 8), dtype=np.uint64)
    np.add.at(t, (np.minimum(a["verdict"], 7), np.minimum(b["verdict"], 7)), 1)
    return t


def records_of(a, b, seed0, idx):
    """The records of the seeds at `idx` (ascending indices), as an ndarray[A.DIFF_RECORD_DTYPE]."""
    r = np.zeros(len(idx), dtype=A.DIFF_RECORD_DTYPE)
    r["seed"] = (np.asarray(idx, dtype=np.uint64) + np.uint64(seed0 & U64_MAX)) if len(idx) else []      # (wraps at 2^64 like the device's add)
    r["a"], r["b"] = a[idx], b[idx]
    return r


def diff_truth(a, b, seed0, fields, cap):
    """What madsim_diff_t holds after a campaign whose two sides gave `a` and `b` for the seeds [seed0, seed0 + len)."""
    assert len(a) == len(b) and 0 < fields <= ALL
    d, inc = masks(a, b, fields), incomparable(a, b)
    idx = np.nonzero(d)[0]
    by_field = [int((d >> np.uint32(i) & 1).sum()) for i in range(7)] + [0]
    with np.errstate(over="ignore"):
        recs = records_of(a, b, seed0, idx[:cap])
    return {"n_listed": min(cap, len(idx)), "n_compared": int(len(a) - inc.sum()), "n_incomparable": int(inc.sum()), "n_differ": len(idx),
            "n_by_field": by_field, "transitions": transitions(a, b).tolist(), "records": recs.tobytes()}


def wave_counts(a, b, fields):
    """Differing seeds per wave under the cut the report kernels use: grid = min(256, ceil(count / 1024)) workgroups of 4 waves, every wave a
    contiguous piece, a multiple of 64 seeds (zeros for waves of the grid that own nothing)."""
    count = len(a)
    grid = max(1, min(256, (count + 1023) // 1024))
    waves = 4 * grid
    piece = ((count + waves - 1) // waves + 63) // 64 * 64
    d = masks(a, b, fields) != 0
    return piece, [int(d[w * piece:(w + 1) * piece].sum()) for w in range(waves)]


def words_of(a, b, fields):
    """The MADSIM_K_DIFF_WORDS words the device leaves for a batch: {n_differ, n_incomparable, n_by_field[8], transitions[8][8]}."""
    t = diff_truth(a, b, 0, fields, 0)
    w = np.array([t["n_differ"], t["n_incomparable"]] + t["n_by_field"] + [c for row in t["transitions"] for c in row], dtype=np.uint64)
    assert len(w) == WORDS
    return w


def of_struct(d, records):
    """An A.Diff after a call (and the ndarray its `records` points into) in the shape of diff_truth's answer."""
    return {"n_listed": int(d.n_listed), "n_compared": int(d.n_compared), "n_incomparable": int(d.n_incomparable), "n_differ": int(d.n_differ),
            "n_by_field": [int(x) for x in d.n_by_field], "transitions": [[int(x) for x in row] for row in d.transitions],
            "records": records[:d.n_listed].tobytes()}


def of_report(rep):
    """A runtime.CampaignDiff in the shape of diff_truth's answer."""
    return {"n_listed": len(rep.records), "n_compared": rep.n_compared, "n_incomparable": rep.n_incomparable, "n_differ": rep.n_differ,
            "n_by_field": [int(x) for x in rep.n_by_field], "transitions": rep.transitions.astype(np.uint64).tolist(), "records": rep.records.tobytes()}


def synthetic(rng, n, p_differ=0.05, verdicts=(0, 0, 0, 0, 1, 2, 3, 4, 5, 7, 0xffffffff)):
    """Two sides of n results: B is A, except that about p_differ of the seeds get a few random fields redrawn (verdict among them)."""
    a = np.zeros(n, dtype=A.RESULT_DTYPE)
    a["verdict"] = rng.choice(np.array(verdicts, dtype=np.uint32), n)
    a["steps"] = rng.integers(0, 1 << 32, n, dtype=np.uint64)
    for name in WIDE:
        a[name] = rng.integers(0, 1 << 64, n, dtype=np.uint64)
    b = a.copy()
    for i in np.nonzero(rng.random(n) < p_differ)[0]:
        for name in rng.choice(FIELDS, rng.integers(1, 4), replace=False):
            if name == "verdict":
                b[name][i] = rng.choice(np.array(verdicts, dtype=np.uint32))
            elif name == "steps":
                b[name][i] ^= np.uint32(1) << np.uint32(rng.integers(0, 32))
            else:
                b[name][i] ^= np.uint64(1) << np.uint64(rng.integers(0, 64))
    return a, b


SEED0, TOTAL, LOSS, DEADLOCKS = 5_000_000, 10_000, 0.002, 1149


@functools.lru_cache(maxsize=None)
def two_configs():
    """(workload, config A, config B, the oracle's results of side A, of side B — read-only): the four-node ping-pong at loss 0 and at
    loss LOSS over TOTAL seeds from SEED0; DEADLOCKS of them deadlock on the lossy side (tests/test_campaign_diff.py asserts it)."""
    w, cfg_a, cfg_b = W.pingpong(4, 16), A.Config.default(), A.Config.default(packet_loss_rate=LOSS)
    a, _ = oracle.run_batch(w, SEED0, TOTAL, cfg_a)
    b, _ = oracle.run_batch(w, SEED0, TOTAL, cfg_b)
    a.setflags(write=False)
    b.setflags(write=False)
    return w, cfg_a, cfg_b, a, b
