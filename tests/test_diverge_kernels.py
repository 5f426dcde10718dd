"""diverge_kernel (csrc/sim_kernel.hip) on SYNTHETIC rows, launched directly (tests/diverge_kernels.py): every record word and every context
word is held against tests/diverge_ref.py, exactly, for 1-byte and 8-byte entries in the same launch.  Row pairs the simulator rarely or
never produces: a first difference at entry 0, 15, 16, inside the unaligned head of a row, at the last entry before the walk ends, on both
sides of a wave trip's edge (bytes 1 023 / 1 024 of the row and of its aligned body), in byte 7 of a word only and in byte 0 of the next
word only, with a later second difference; one side a prefix of the other, empty sides, lengths beyond the cap with and without a
difference inside it; every runner verdict on either side over garbage rows — and, always, DIFFERENT garbage on the two sides behind
min(len_x, cap): a kernel that compares what lies behind a row's end fails here and nowhere else.
Every array comes from numpy.random.default_rng([SEED, ...]); SEED is in every assertion message."""
import numpy as np
import pytest

from madsim_amd import _abi as A
from tests import diverge_kernels as K
from tests import diverge_ref as R

pytestmark = pytest.mark.gpu

SEED = 20261019
ROWS = (1, 3, 64, 65, 257, 1025)              # the last: more rows than the grid has waves, so waves stride
CAPS = (0, 1, 15, 16, 17, 63, 64, 1023, 1024, 1025, 4099)
WINS = (0, 1, 4, 8)
N_KINDS = 24
RUNNER_VERDICTS = (A.OVERFLOW, A.STEP_LIMIT, A.UNSUPPORTED, A.INTERNAL, 8, 0x7fffffff, 0x80000000, 0xffffffff)


def _flip(rng, dtype, where):
    """A non-zero XOR mask: any byte, byte 7 of a word only, or byte 0 only."""
    if dtype == np.uint8:
        return np.uint8(rng.integers(1, 256))
    if where == "hi":
        return np.uint64(int(rng.integers(1, 256)) << 56)
    if where == "lo":
        return np.uint64(int(rng.integers(1, 256)))
    return np.uint64(int(rng.integers(1, 1 << 63)) | 1 << int(rng.integers(0, 64)))


def channel_case(rng, n, cap, dtype):
    """(rows_a, rows_b, len_a, len_b) of n synthetic row pairs, row r of kind r % N_KINDS; garbage behind min(len_x, cap) on both sides."""
    esize = np.dtype(dtype).itemsize
    top = 256 if dtype == np.uint8 else 1 << 64
    a = rng.integers(0, top, (n, cap), dtype=dtype)
    b = a.copy()
    la, lb = np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.uint64)
    over = lambda: cap + int(rng.integers(1, 1000))                            # noqa: E731
    below = lambda: int(rng.integers(0, cap + 1))                              # noqa: E731
    for r in range(n):
        kind = r % N_KINDS
        head = (-(r * cap * esize)) % 16                                       # bytes of row r in front of its 16-byte aligned body
        x, y, at, where = cap, cap, [], "any"                                  # lengths, entries to flip (dropped when >= m), which byte
        if kind == 0: x = y = below()
        elif kind == 1: at = [0]
        elif kind == 2: at = [15]
        elif kind == 3: at = [16]
        elif kind == 4: at = [max(head // esize - 1, 0)]                       # the last entry of the unaligned head
        elif kind == 5: at = [head // esize]                                   # the first entry of the aligned body
        elif kind == 6: x = y = below(); at = [max(x, 1) - 1]                  # the last entry before m
        elif kind == 7: at, where = [1023 // esize], "hi"                      # byte 1 023 of the row
        elif kind == 8: at, where = [1024 // esize], "lo"                      # byte 1 024
        elif kind == 9: at, where = [(head + 1023) // esize], "hi"             # the last byte of the body's first wave trip
        elif kind == 10: at, where = [(head + 1024) // esize], "lo"            # the first byte of its second
        elif kind == 11: at, where = [int(rng.integers(0, max(cap, 1)))], "hi"
        elif kind == 12: at, where = [int(rng.integers(0, max(cap, 1)))], "lo"
        elif kind == 13: p = int(rng.integers(0, max(cap, 1))); at = [p, p + 1, p + int(rng.integers(1, 2000)), cap - 1]      # later ones: ignored
        elif kind == 14: y = below(); x = int(rng.integers(0, y + 1))          # A a prefix of B (or equal)
        elif kind == 15: x = below(); y = int(rng.integers(0, x + 1))          # the reverse
        elif kind == 16: x, y = 0, below()
        elif kind == 17: x, y = below(), 0
        elif kind == 18: x = y = 0
        elif kind == 19: x, y = over(), over()                                 # both beyond the cap, the kept parts equal
        elif kind == 20: x, y = over(), over(); at = [int(rng.integers(0, max(cap, 1)))]
        elif kind == 21: x, y = over(), below()                                # one beyond the cap: a prefix, possibly at == cap
        elif kind == 22: x, y = below(), below(); at = [int(rng.integers(0, max(cap, 1)))]
        else: x = y = over(); at = [cap - 1]
        la[r], lb[r] = x, y
        m = min(x, y, cap)
        for p in at:
            if 0 <= p < m:
                b[r, p] = a[r, p] ^ _flip(rng, dtype, where)
        ka, kb = min(x, cap), min(y, cap)
        if ka < cap:
            a[r, ka:] = rng.integers(0, top, cap - ka, dtype=dtype)
        if kb < cap:
            b[r, kb:] = a[r, kb:] ^ dtype(0x5A)                                # never what side A holds there
    return a, b, la, lb


def results(rng, n, runner_rows=()):
    """Two result arrays of n rows with reference verdicts; `runner_rows`: {row: (verdict_a, verdict_b)}."""
    out = []
    for _ in range(2):
        r = np.zeros(n, dtype=A.RESULT_DTYPE)
        r["verdict"] = rng.integers(0, 4, n, dtype=np.uint32)
        r["steps"] = rng.integers(0, 1 << 32, n, dtype=np.uint64)
        for name in ("clock_ns", "msg_count", "rng_calls", "trace_hash", "obs_hash"):
            r[name] = rng.integers(0, 1 << 64, n, dtype=np.uint64)
        out.append(r)
    for row, (va, vb) in dict(runner_rows).items():
        out[0]["verdict"][row], out[1]["verdict"][row] = va, vb
    return out


def check(rng, n, cap, win, what, runner_rows=(), case=None):
    """One launch against the truth; returns the truth's records."""
    logs = case[0] if case else channel_case(rng, n, cap, np.uint8)
    obs = case[1] if case else channel_case(rng, n, cap, np.uint64)
    ra, rb = results(rng, n, runner_rows)
    seeds = rng.integers(0, 1 << 64, n, dtype=np.uint64)
    got, ctx = K.diverge(logs[0], logs[1], logs[2], logs[3], obs[0], obs[1], obs[2], obs[3], ra, rb, seeds, win)
    want, want_ctx = R.records(seeds, logs[0], logs[1], logs[2], logs[3], obs[0], obs[1], obs[2], obs[3], ra, rb, win)
    print(what, "log statuses", np.bincount(want["log_status"], minlength=5).tolist(), "obs statuses", np.bincount(want["obs_status"], minlength=5).tolist())
    if got.tobytes() != want.tobytes():
        bad = [i for i in range(n) if got[i].tobytes() != want[i].tobytes()]
        raise AssertionError((SEED, what, "rows", bad[:8], "kind", [i % N_KINDS for i in bad[:8]], got[bad[0]], want[bad[0]]))
    assert ctx.tobytes() == want_ctx.tobytes(), (SEED, what, "context", np.nonzero((ctx != want_ctx).any(axis=1))[0][:8].tolist())
    return want


@pytest.mark.parametrize("cap", CAPS)
def test_every_row_count_at_every_cap(hip, cap):
    """All 24 kinds of row pair at every row count, every window across the row counts; from 65 rows on every status is present."""
    for k, n in enumerate(ROWS):
        rng = np.random.default_rng([SEED, cap, n])
        runner = {r: (A.STEP_LIMIT, A.PASS) for r in range(7, n, 29)}
        want = check(rng, n, cap, WINS[(k + CAPS.index(cap)) % 4], ("rows", n, "cap", cap), runner)
        if n >= 65 and cap >= 17:
            for ch in ("log_status", "obs_status"):
                assert set(want[ch].tolist()) == {R.SAME, R.DIFFER, R.PREFIX, R.BEYOND_CAP, R.INCOMPARABLE}, (SEED, cap, n, ch)
        if n >= 65 and cap == 0:
            assert set(want["log_status"].tolist()) == {R.SAME, R.PREFIX, R.BEYOND_CAP, R.INCOMPARABLE} and not want["log_at"].any()


@pytest.mark.parametrize("win", WINS)
def test_every_window(hip, win):
    """Every window at caps around it: `at` below the window (zero-filled on the left), at + win beyond one side's end and beyond the cap."""
    for cap in (1, 7, 8, 9, 17, 1025):
        rng = np.random.default_rng([SEED, 1, win, cap])
        want = check(rng, 257, cap, win, ("win", win, "cap", cap))
        at, ka = want["obs_at"], np.minimum(want["obs_len_a"], cap)
        if win:
            assert (at < win).any() and (at + win > ka).any() and (at + win > cap).any(), (SEED, win, cap)
            if cap == 1025:
                assert ((at >= win) & (at + win <= ka) & (want["obs_status"] == R.DIFFER)).any()


def test_garbage_behind_the_lengths_is_never_compared(hip):
    """Equal prefixes, unequal lengths, and behind each side's end bytes that differ from the other side's everywhere: PREFIX at L, never a
    later DIFFER; with equal lengths SAME.  A kernel that walks to `cap` fails here."""
    rng = np.random.default_rng([SEED, 2])
    n, cap = 130, 1025
    cases = []
    for dtype in (np.uint8, np.uint64):
        a = rng.integers(1, 256, (n, cap)).astype(dtype)
        b = a.copy()
        la = rng.integers(0, cap + 1, n).astype(np.uint64)
        lb = np.where(np.arange(n) % 2 == 0, la, rng.integers(0, cap + 1, n)).astype(np.uint64)
        for r in range(n):
            a[r, int(la[r]):] = 0x11
            b[r, int(lb[r]):] = 0xEE
        cases.append((a, b, la, lb))
    want = check(rng, n, cap, 4, "garbage", case=cases)
    for ch in ("log", "obs"):
        st, at = want[ch + "_status"], want[ch + "_at"]
        assert set(st.tolist()) == {R.SAME, R.PREFIX} and (st[::2] == R.SAME).all(), (SEED, ch)
        assert (at == np.minimum(want[ch + "_len_a"], want[ch + "_len_b"])).all()


def test_every_runner_verdict_on_either_side(hip):
    """Every runner verdict on A only, on B only and on both, over garbage rows and lengths: INCOMPARABLE, at 0, no entry, an all-zero
    context row — and the rows beside them compared as ever."""
    rng = np.random.default_rng([SEED, 3])
    n, cap = 3 * len(RUNNER_VERDICTS) * 3, 65
    runner, row = {}, 0
    for v in RUNNER_VERDICTS:
        for va, vb in ((v, A.PASS), (A.DEADLOCK, v), (v, RUNNER_VERDICTS[(RUNNER_VERDICTS.index(v) + 1) % len(RUNNER_VERDICTS)])):
            runner[row] = (va, vb)
            row += 3                                                           # two compared rows between any two
    cases = []
    for dtype in (np.uint8, np.uint64):
        a, b, la, lb = channel_case(rng, n, cap, dtype)
        for r in runner:
            top = 256 if dtype == np.uint8 else 1 << 64
            a[r], b[r] = rng.integers(0, top, cap, dtype=dtype), rng.integers(0, top, cap, dtype=dtype)
            la[r], lb[r] = rng.integers(0, 1 << 40), rng.integers(0, 1 << 40)
        cases.append((a, b, la, lb))
    want = check(rng, n, cap, 8, "runner verdicts", runner, cases)
    rows = sorted(runner)
    for ch in ("log", "obs"):
        assert (want[ch + "_status"][rows] == R.INCOMPARABLE).all() and not want[ch + "_at"][rows].any()
        assert not want[ch + "_a"][rows].any() and not want[ch + "_b"][rows].any()
        others = np.setdiff1d(np.arange(n), rows)
        assert (want[ch + "_status"][others] != R.INCOMPARABLE).all()


def test_the_launcher_refuses_what_the_kernel_is_not_written_for(hip):
    """Nothing is launched for no rows, 2^32 rows, a window above MADSIM_DIVERGE_MAX_WIN, a window without context rows (or the reverse), a
    missing array or a row array that is not 16-byte aligned."""
    import torch
    L = K._lib()
    n, cap = 4, 32
    buf = lambda nb: torch.zeros(nb + 16, dtype=torch.uint8, device="cuda")    # noqa: E731
    logs, obs, lens, res, seeds = buf(n * cap), buf(8 * n * cap), buf(8 * n), buf(48 * n), buf(8 * n)
    recs, ctx = torch.full((184 * n,), 0xA5, dtype=torch.uint8, device="cuda"), torch.full((24 * 8 * n,), 0xA5, dtype=torch.uint8, device="cuda")
    lp, op, ln, rs, sd, rp, cp = (t.data_ptr() for t in (logs, obs, lens, res, seeds, recs, ctx))
    good = [lp, lp, cap, op, op, cap, ln, ln, ln, ln, rs, rs, sd, n, 4, rp, cp, None]
    def call(**kw):
        args = list(good)
        for i, v in kw.items():
            args[int(i[1:])] = v
        return L.madsim_k_launch_diverge(*args)
    assert call(a13=0) == -1 and call(a13=1 << 32) == -1
    assert call(a14=9) == -1 and call(a14=0) == -1 and call(a16=None) == -1
    for i in (0, 1, 3, 4, 6, 7, 8, 9, 10, 11, 12, 15):
        assert call(**{f"a{i}": None}) == -1, i
    for i in (0, 1, 3, 4):
        assert call(**{f"a{i}": good[i] + 8}) == -1, i
    torch.cuda.synchronize()
    assert bool((recs == 0xA5).all()) and bool((ctx == 0xA5).all())
    assert call() == 0
    torch.cuda.synchronize()
    assert not bool((recs == 0xA5).all())
