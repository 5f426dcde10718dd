"""Divergence reports in numpy: the rules of madsim_hip_diverge_seeds (include/madsim_hip.h) restated over whole row arrays, for the tests
that hold diverge_kernel (csrc/sim_kernel.hip) and the entry points against them.  Nothing here touches a device.

One channel of n row pairs: rows of `cap` entries (uint8: the determinism log; uint64: the observations), the TRUE lengths (which may exceed
cap) and a per-row `runner` flag (either side's verdict is a runner verdict).  With L = min(len_a, len_b) and m = min(L, cap):
    INCOMPARABLE  runner                                              at = 0
    DIFFER        the smallest i < m with a[i] != b[i] exists         at = i
    SAME          no such i, L <= cap, len_a == len_b                 at = len
    PREFIX        no such i, L <= cap, len_a != len_b                 at = L
    BEYOND_CAP    no such i, L > cap                                  at = cap
Entries at or behind min(len_x, cap) are never looked at, whatever they hold."""
import numpy as np

from madsim_amd import _abi as A

SAME, DIFFER, PREFIX, BEYOND_CAP, INCOMPARABLE = range(5)
assert (SAME, DIFFER, PREFIX, BEYOND_CAP, INCOMPARABLE) == (A.DIVERGE_SAME, A.DIVERGE_DIFFER, A.DIVERGE_PREFIX, A.DIVERGE_BEYOND_CAP,
                                                           A.DIVERGE_INCOMPARABLE)
MAX_WIN = A.DIVERGE_MAX_WIN


def _take(rows, at, keep):
    """rows[i, at[i]] where at[i] < keep[i], else 0 (at may lie outside the row)."""
    n, cap = rows.shape
    out = np.zeros(n, dtype=np.uint64)
    ok = at < keep
    if cap and ok.any():
        i = np.nonzero(ok)[0]
        out[i] = rows[i, at[i].astype(np.int64)]
    return out


def channel(rows_a, rows_b, len_a, len_b, runner, win=0):
    """(status uint32[n], at uint64[n], entry_a uint64[n], entry_b uint64[n], ctx uint64[n, 3 * win]) of one channel."""
    rows_a, rows_b = np.asarray(rows_a), np.asarray(rows_b)
    assert rows_a.shape == rows_b.shape and rows_a.ndim == 2 and rows_a.dtype == rows_b.dtype and 0 <= win <= MAX_WIN
    n, cap = rows_a.shape
    len_a, len_b, runner = np.asarray(len_a, dtype=np.uint64), np.asarray(len_b, dtype=np.uint64), np.asarray(runner, dtype=bool)
    L = np.minimum(len_a, len_b)
    m = np.minimum(L, np.uint64(cap))
    cols = np.arange(cap, dtype=np.uint64)[None, :]
    ne = (rows_a != rows_b) & (cols < m[:, None])
    hit = ne.any(axis=1) if cap else np.zeros(n, dtype=bool)
    first = ne.argmax(axis=1).astype(np.uint64) if cap else np.zeros(n, dtype=np.uint64)
    status = np.where(hit, DIFFER, np.where(L > np.uint64(cap), BEYOND_CAP, np.where(len_a == len_b, SAME, PREFIX))).astype(np.uint32)
    at = np.where(hit, first, np.where(L > np.uint64(cap), np.uint64(cap), L)).astype(np.uint64)
    status[runner], at[runner] = INCOMPARABLE, 0
    keep_a, keep_b = np.minimum(len_a, np.uint64(cap)), np.minimum(len_b, np.uint64(cap))
    keep_a[runner], keep_b[runner] = 0, 0                                    # nothing of an incomparable row is reported
    ent_a, ent_b = _take(rows_a, at, keep_a), _take(rows_b, at, keep_b)
    ctx = np.zeros((n, 3 * win), dtype=np.uint64)
    for j in range(win):
        back = at + np.uint64(j)                                             # shared[j] = a[at - win + j] where that index exists
        ok = (back >= np.uint64(win)) & ~runner
        ctx[:, j] = _take(rows_a, np.where(ok, back - np.uint64(win), 0).astype(np.uint64), np.where(ok, at, 0).astype(np.uint64))
        ctx[:, win + j] = _take(rows_a, at + np.uint64(j), keep_a)
        ctx[:, 2 * win + j] = _take(rows_b, at + np.uint64(j), keep_b)
    return status, at, ent_a, ent_b, ctx


def is_runner(results):
    return np.asarray(results)["verdict"] >= A.OVERFLOW


def records(seeds, logs_a, logs_b, log_len_a, log_len_b, obs_a, obs_b, obs_len_a, obs_len_b, res_a, res_b, win=0):
    """(ndarray[A.DIVERGENCE_DTYPE] of n records, uint64[n, 3 * win] context rows): what madsim_hip_diverge_seeds returns for these rows."""
    n = len(seeds)
    runner = is_runner(res_a) | is_runner(res_b)
    ls, la, ea, eb, _ = channel(logs_a, logs_b, log_len_a, log_len_b, runner)
    os_, oa, xa, xb, ctx = channel(obs_a, obs_b, obs_len_a, obs_len_b, runner, win)
    r = np.zeros(n, dtype=A.DIVERGENCE_DTYPE)
    r["seed"], r["log_status"], r["obs_status"], r["log_at"], r["obs_at"] = np.asarray(seeds, dtype=np.uint64), ls, os_, la, oa
    r["log_len_a"], r["log_len_b"], r["obs_len_a"], r["obs_len_b"] = log_len_a, log_len_b, obs_len_a, obs_len_b
    r["obs_a"], r["obs_b"], r["log_a"], r["log_b"] = xa, xb, ea.astype(np.uint8), eb.astype(np.uint8)
    r["a"], r["b"] = res_a, res_b
    return r, ctx


def rows_of(lists, cap, dtype):
    """(rows [n, cap] zero-filled, true lengths) of n Python lists / bytes: what madsim_hip_trace_seeds leaves in a row."""
    rows, lens = np.zeros((len(lists), cap), dtype=dtype), np.zeros(len(lists), dtype=np.uint64)
    for i, v in enumerate(lists):
        v = np.frombuffer(v, dtype=np.uint8) if isinstance(v, (bytes, bytearray)) else np.asarray(v, dtype=dtype)
        lens[i] = len(v)
        k = min(len(v), cap)
        rows[i, :k] = v[:k]
    return rows, lens


def one(a, b, len_a, len_b, runner, cap, win=0):
    """The same rules for ONE row pair as a plain loop over Python lists `a`, `b` (the rows, `cap` entries each): (status, at, entry_a,
    entry_b, ctx list).  tests/test_diverge.py holds channel() against it."""
    if runner:
        return INCOMPARABLE, 0, 0, 0, [0] * (3 * win)
    L = min(len_a, len_b)
    m = min(L, cap)
    status, at = None, None
    for i in range(m):
        if a[i] != b[i]:
            status, at = DIFFER, i
            break
    if status is None:
        if L > cap:
            status, at = BEYOND_CAP, cap
        elif len_a == len_b:
            status, at = SAME, len_a
        else:
            status, at = PREFIX, L
    ka, kb = min(len_a, cap), min(len_b, cap)
    ent_a, ent_b = (a[at] if at < ka else 0), (b[at] if at < kb else 0)
    shared = [a[at - win + j] if at - win + j >= 0 else 0 for j in range(win)]
    nxt_a = [a[at + j] if at + j < ka else 0 for j in range(win)]
    nxt_b = [b[at + j] if at + j < kb else 0 for j in range(win)]
    return status, at, ent_a, ent_b, shared + nxt_a + nxt_b
