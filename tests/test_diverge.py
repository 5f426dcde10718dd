"""Divergence reports (madsim_hip_diverge_seeds and its _ctx_ form) without a GPU: tests/diverge_ref.py — the numpy restatement of the status
rules — against a plain-Python loop on random small cases and hand-written ones; the struct, the prototypes and the constants against the
header, the ctypes mirror, the Rust sys file and the C++ mirror; the argument errors and the MADSIM_TRACE_MAX_BYTES bound, which need no
device; and, from the CPU oracle alone, the proof that the end-to-end blocks tests/test_diverge_gpu.py runs hold the statuses they are
there for (at least three seeds each).  What the GPU answers is tests/test_diverge_kernels.py's and tests/test_diverge_gpu.py's business."""
import ctypes as C
import functools
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import oracle
from madsim_amd import _abi as A
from madsim_amd import runtime, workload
from tests import cheader as H
from tests import diverge_ref as R
from tests import groups_ref as G
from tests import parity as P
from tests import test_observe as T

E_ARG, E_HIP, E_NOINIT, E_WORKLOAD, E_LIMITS = -1, -2, -3, -4, -5
SEED = 20261019
U64_MAX = (1 << 64) - 1
NEW = ("madsim_hip_diverge_seeds", "madsim_hip_ctx_diverge_seeds")


# ---- the rules: numpy against a plain loop ---------------------------------------------------------------------------------------------------
def _against_the_loop(a, b, la, lb, runner, win, what):
    st, at, ea, eb, ctx = R.channel(a, b, la, lb, runner, win)
    for i in range(len(a)):
        want = R.one(a[i].tolist(), b[i].tolist(), int(la[i]), int(lb[i]), bool(runner[i]), a.shape[1], win)
        got = (int(st[i]), int(at[i]), int(ea[i]), int(eb[i]), ctx[i].tolist())
        assert got == want, (SEED, what, i, got, want)
    return st, at, ea, eb, ctx


@pytest.mark.parametrize("dtype", [np.uint8, np.uint64])
def test_the_numpy_rules_are_the_plain_loop_on_random_small_cases(dtype):
    """A few hundred row pairs per cap over a two-letter alphabet (so that equal prefixes are long), random lengths on both sides of the cap,
    garbage behind the lengths, a runner flag on some, every window."""
    rng = np.random.default_rng([SEED, np.dtype(dtype).itemsize])
    seen = set()
    for cap in (0, 1, 2, 5, 16, 33):
        for win in (0, 1, 4, 8):
            n = 100
            a = rng.integers(0, 2, (n, cap)).astype(dtype)
            b = np.where(rng.random((n, cap)) < 0.08, 1 - a, a).astype(dtype)
            la, lb = rng.integers(0, cap + 4, n).astype(np.uint64), rng.integers(0, cap + 4, n).astype(np.uint64)
            same_len = rng.random(n) < 0.5
            lb[same_len] = la[same_len]
            for r in range(n):                                                  # garbage behind min(len, cap), different on the two sides
                a[r, min(int(la[r]), cap):] = 7
                b[r, min(int(lb[r]), cap):] = 9
            runner = rng.random(n) < 0.1
            st = _against_the_loop(a, b, la, lb, runner, win, (cap, win))[0]
            seen |= set(st.tolist())
    assert seen == {R.SAME, R.DIFFER, R.PREFIX, R.BEYOND_CAP, R.INCOMPARABLE}


def test_the_rules_on_hand_written_cases():
    """The status table of include/madsim_hip.h, line by line, cap = 4 and a window of 2."""
    X = 0xEE                                                                        # garbage behind a row's end
    rows = [   # a,               b,               len_a, len_b, runner -> status, at, entry_a, entry_b, shared, next_a, next_b
        ([1, 2, 3, 4], [1, 2, 3, 4], 4, 4, False, R.SAME, 4, 0, 0, [3, 4], [0, 0], [0, 0]),
        ([1, 2, X, X], [1, 2, 9, 9], 2, 2, False, R.SAME, 2, 0, 0, [1, 2], [0, 0], [0, 0]),
        ([X, X, X, X], [9, 9, 9, 9], 0, 0, False, R.SAME, 0, 0, 0, [0, 0], [0, 0], [0, 0]),
        ([5, 2, 3, 4], [6, 2, 3, 4], 4, 4, False, R.DIFFER, 0, 5, 6, [0, 0], [5, 2], [6, 2]),
        ([1, 2, 3, 4], [1, 2, 3, 5], 4, 4, False, R.DIFFER, 3, 4, 5, [2, 3], [4, 0], [5, 0]),
        ([1, 7, 3, 4], [1, 8, 3, 9], 9, 4, False, R.DIFFER, 1, 7, 8, [0, 1], [7, 3], [8, 3]),          # the second difference is ignored
        ([1, 2, X, X], [1, 2, 3, 4], 2, 4, False, R.PREFIX, 2, 0, 3, [1, 2], [0, 0], [3, 4]),          # A ended where B went on
        ([1, 2, 3, 9], [1, 2, 3, X], 4, 3, False, R.PREFIX, 3, 9, 0, [2, 3], [9, 0], [0, 0]),
        ([X, X, X, X], [1, 2, 3, 4], 0, 7, False, R.PREFIX, 0, 0, 1, [0, 0], [0, 0], [1, 2]),
        ([1, 2, 3, 4], [1, 2, 3, 4], 4, 5, False, R.PREFIX, 4, 0, 0, [3, 4], [0, 0], [0, 0]),          # L == cap: nothing of B at index 4 was kept
        ([1, 2, 3, 4], [1, 2, 3, 4], 5, 5, False, R.BEYOND_CAP, 4, 0, 0, [3, 4], [0, 0], [0, 0]),
        ([1, 2, 3, 4], [1, 2, 3, 4], 5, 900, False, R.BEYOND_CAP, 4, 0, 0, [3, 4], [0, 0], [0, 0]),
        ([1, 2, 3, 4], [1, 2, 0, 4], 5, 900, False, R.DIFFER, 2, 3, 0, [1, 2], [3, 4], [0, 4]),
        ([1, 2, 3, 4], [5, 6, 7, 8], 4, 4, True, R.INCOMPARABLE, 0, 0, 0, [0, 0], [0, 0], [0, 0]),
    ]
    for dtype in (np.uint8, np.uint64):
        a, b = np.array([r[0] for r in rows], dtype=dtype), np.array([r[1] for r in rows], dtype=dtype)
        la, lb, runner = [r[2] for r in rows], [r[3] for r in rows], [r[4] for r in rows]
        st, at, ea, eb, ctx = _against_the_loop(a, b, la, lb, np.array(runner), 2, "hand-written")
        for i, r in enumerate(rows):
            assert (int(st[i]), int(at[i]), int(ea[i]), int(eb[i]), ctx[i].tolist()) == (r[5], r[6], r[7], r[8], r[9] + r[10] + r[11]), (i, r)
    # cap == 0 needs no special case
    e = np.zeros((3, 0), dtype=np.uint8)
    st, at, _, _, _ = R.channel(e, e, [0, 0, 3], [0, 2, 3], [False] * 3)
    assert st.tolist() == [R.SAME, R.PREFIX, R.BEYOND_CAP] and at.tolist() == [0, 0, 0]


# ---- the surface -----------------------------------------------------------------------------------------------------------------------------
def _struct():
    joined = re.sub(r"\bstruct\s+(madsim_divergence)\s*\{([^{}]*)\}\s*;\s*typedef\s+struct\s+\1\s+(\w+)\s*;", r"typedef struct \1 {\2} \3;", H.header_text())
    return H.structs(joined)["madsim_divergence_t"]


def test_struct_constants_and_prototypes_match_the_header():
    S = _struct()
    offs, size = H.layout(S, {"madsim_result_t": (48, 8)})
    assert size == 184 == C.sizeof(A.Divergence) == np.dtype(A.DIVERGENCE_DTYPE).itemsize
    assert [f[0] for f in S] == [f[0] for f in A.Divergence._fields_] == list(np.dtype(A.DIVERGENCE_DTYPE).names)
    dt = np.dtype(A.DIVERGENCE_DTYPE)
    for name, _, _, _ in S:
        assert getattr(A.Divergence, name).offset == offs[name] == dt.fields[name][1], name
    assert (offs["log_a"], offs["log_b"], offs["pad"], offs["a"], offs["b"]) == (80, 81, 82, 88, 136)
    D = {k: int(v.rstrip("u")) for k, v in H.defines().items() if k.startswith("MADSIM_DIVERGE_")}
    assert D == {"MADSIM_DIVERGE_SAME": 0, "MADSIM_DIVERGE_DIFFER": 1, "MADSIM_DIVERGE_PREFIX": 2, "MADSIM_DIVERGE_BEYOND_CAP": 3,
                 "MADSIM_DIVERGE_INCOMPARABLE": 4, "MADSIM_DIVERGE_MAX_WIN": 8}
    assert (A.DIVERGE_SAME, A.DIVERGE_DIFFER, A.DIVERGE_PREFIX, A.DIVERGE_BEYOND_CAP, A.DIVERGE_INCOMPARABLE, A.DIVERGE_MAX_WIN) == (0, 1, 2, 3, 4, 8)
    assert len(A.DIVERGE_NAMES) == 5
    assert A.ABI_VERSION == 7 == int(H.defines()["MADSIM_HIP_ABI_VERSION"].rstrip("u"))          # additive: the version stays
    fns = H.functions()
    side = ["const madsim_workload_t*", "const madsim_config_t*", "const madsim_limits_t*"]
    tail = side + side + ["const uint64_t*", "uint64_t", "uint64_t", "uint64_t", "uint32_t", "madsim_divergence_t*", "uint64_t*"]
    assert fns["madsim_hip_diverge_seeds"] == ("int", tail)
    assert fns["madsim_hip_ctx_diverge_seeds"] == ("int", ["madsim_hip_ctx_t*"] + tail)
    L = runtime.lib()
    for fn in NEW + ("madsim_k_launch_diverge",):
        assert hasattr(L, fn), fn
    assert len(L.madsim_hip_diverge_seeds.argtypes) == len(tail) and len(L.madsim_hip_ctx_diverge_seeds.argtypes) == len(tail) + 1


def test_the_mirrors_declare_the_call():
    for fn in (runtime.diverge_seeds, runtime.Context.diverge_seeds):
        p = inspect.signature(fn).parameters
        names = [k for k in p if k != "self"]
        assert names == ["workload", "seeds", "other", "config", "other_config", "limits", "other_limits", "log_cap", "obs_cap", "window", "resolve"]
        assert [p[k].default for k in names[2:]] == [None, None, None, None, None, 1 << 16, 256, 4, True]
    assert runtime.Divergence.__slots__[-3:] == ("shared", "next_a", "next_b")
    assert runtime.SeedTrace.__slots__ == ("seed", "result", "observations", "n_observations", "log", "log_len")      # untouched
    sys_rs = open(os.path.join(H.ROOT, "bindings", "rust", "madsim-hip-sys", "src", "lib.rs")).read()
    m = re.search(r"pub struct madsim_divergence_t \{(.*?)\n\}", sys_rs, flags=re.S)
    assert [f for f, _ in re.findall(r"pub (\w+): ([^,\n]+),", m.group(1))] == [f[0] for f in A.Divergence._fields_]
    for fn in NEW:
        assert re.search(r"pub fn %s\([^;]*recs: \*mut madsim_divergence_t, obs_ctx: \*mut u64\) -> c_int;" % fn, sys_rs), fn
    assert "pub const MADSIM_DIVERGE_INCOMPARABLE: u32 = 4;" in sys_rs and "pub const MADSIM_DIVERGE_MAX_WIN: u32 = 8;" in sys_rs
    high = open(os.path.join(H.ROOT, "bindings", "rust", "madsim-hip", "src", "builder.rs")).read()
    assert "pub fn diverge_seeds(&self, workload: &Workload, other: &Builder, other_workload: &Workload, seeds: &[u64]" in high
    assert "madsim_hip_ctx_diverge_seeds" in high
    hpp = open(os.path.join(H.ROOT, "include", "madsim_hip.hpp")).read()
    assert re.search(r"diverge_against\(const Builder& other, const std::vector<uint64_t>& seeds, const Workload& wl, const Workload& other_wl,", hpp)


def test_the_cpp_mirror_builds():
    exe = os.path.join(H.ROOT, "examples", "diverge_test")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", os.path.join(H.ROOT, "examples", "diverge_test.cpp"), "-o", exe,
                           "-L" + os.path.join(H.ROOT, "madsim_amd"), "-lmadsim_hip", "-Wl,-rpath," + os.path.join(H.ROOT, "madsim_amd")])
    entry = open(os.path.join(H.ROOT, "__graft_entry__.py")).read()
    assert '"diverge_test"' in entry


def _call(n=4, log_cap=64, obs_cap=8, win=4, seeds=True, recs=True, ctx=True, wl_b=None, ctx_handle=False):
    """The C entry itself with host buffers of the right sizes: (rc, last error)."""
    L = runtime.lib()
    w = workload.pingpong(2, 4)
    wb = wl_b or w
    cfg, lim = A.Config.default(), A.Limits()
    s = np.arange(max(n, 1), dtype=np.uint64)
    r = np.full(max(n, 1), 0xAA, dtype=np.uint8).repeat(184)
    x = np.full(max(n, 1) * 3 * max(win, 1), 0xAAAAAAAAAAAAAAAA, dtype=np.uint64)
    args = [w.ref(), C.byref(cfg), C.byref(lim), wb.ref(), C.byref(cfg), C.byref(lim), s.ctypes.data_as(C.POINTER(C.c_uint64)) if seeds else None, n,
            log_cap, obs_cap, win, r.ctypes.data_as(C.c_void_p) if recs else None, x.ctypes.data_as(C.c_void_p) if ctx else None]
    rc = L.madsim_hip_ctx_diverge_seeds(None, *args) if ctx_handle else L.madsim_hip_diverge_seeds(*args)
    assert (r == 0xAA).all() and (x == 0xAAAAAAAAAAAAAAAA).all(), "an argument error wrote to the caller's memory"
    return rc, L.madsim_hip_last_error().decode()


def test_argument_errors_need_no_device():
    """Every argument check comes before the context is looked at: without a GPU (and with a null context handle) the answer is still the
    argument error, not MADSIM_E_NOINIT."""
    for handle in (False, True):
        assert _call(n=0, ctx_handle=handle)[0] == 0                                           # touches nothing
        assert _call(seeds=False, ctx_handle=handle)[0] == E_ARG
        assert _call(recs=False, ctx_handle=handle)[0] == E_ARG
        rc, why = _call(win=9, ctx_handle=handle)
        assert rc == E_ARG and "MADSIM_DIVERGE_MAX_WIN" in why
        assert _call(win=0, ctx=True, ctx_handle=handle)[0] == E_ARG                           # context rows without a window
        assert _call(win=4, ctx=False, ctx_handle=handle)[0] == E_ARG                          # a window without context rows
        rc, why = _call(win=4, obs_cap=0, ctx_handle=handle)
        assert rc == E_ARG and "obs_cap" in why
        bad = workload.WorkloadBuilder(); bad.main().jmp(500)
        rc, why = _call(wl_b=bad.build(), ctx_handle=handle)
        assert rc == E_ARG and why.startswith("side B: ") and "jump target" in why
    # the bound: n * (2 * (log_cap + 8 * obs_cap + 72) + 184 + 24 * win) <= MADSIM_TRACE_MAX_BYTES, named in the message, never split
    per_seed = 2 * (1000 + 8 * 8 + 72) + 184 + 24 * 4
    n_max = A.TRACE_MAX_BYTES // per_seed
    L = runtime.lib()
    w, cfg, lim = workload.pingpong(2, 4), A.Config.default(), A.Limits()
    one = (C.c_uint64 * 1)(0)
    rec = (A.Divergence * 1)()
    ctx = (C.c_uint64 * 12)()
    for n, log_cap, obs_cap, want in ((n_max + 1, 1000, 8, E_LIMITS), (2, A.TRACE_MAX_BYTES // 4, 8, E_LIMITS), (2, 0, A.TRACE_MAX_BYTES // 32, E_LIMITS),
                                      (1 << 40, 0, 1, E_LIMITS), (1, A.TRACE_MAX_BYTES + 1, 1, E_LIMITS)):
        rc = L.madsim_hip_diverge_seeds(w.ref(), C.byref(cfg), C.byref(lim), w.ref(), C.byref(cfg), C.byref(lim), one, n, log_cap, obs_cap, 4, rec, ctx)
        assert rc == want and "MADSIM_TRACE_MAX_BYTES" in L.madsim_hip_last_error().decode(), (n, log_cap, obs_cap, rc)
    import torch
    if not torch.cuda.is_available():                                                        # what fits is refused only for want of a device
        rc = L.madsim_hip_diverge_seeds(w.ref(), C.byref(cfg), C.byref(lim), w.ref(), C.byref(cfg), C.byref(lim), one, 1, 1000, 8, 4, rec, ctx)
        assert rc == E_NOINIT
    with pytest.raises(runtime.MadsimHipError, match="resolve"):
        runtime._diverge_seeds(None, w, [1], None, None, None, None, None, 64, 8, 4, 99)


# ---- the end-to-end blocks, and that they hold what they are there for -------------------------------------------------------------------
LOSS = 0.01
N_BLOCK = 300
WINDOW = 4


def limits_like(lim=None, **kw):
    out = A.Limits()
    if lim is not None:
        for f, _ in A.Limits._fields_:
            setattr(out, f, getattr(lim, f))
    for k, v in kw.items():
        setattr(out, k, v)
    return out


@functools.lru_cache(maxsize=None)
def blocks():
    """name -> (workload A, config A, limits A, workload B, config B, limits B, seed0, n, log_cap, obs_cap): the traced two-pair ping-pong
    without loss against the same body under loss (gen_bool draws at p = 0 too: the logs agree until the first lost message); the lossy
    body against the body with a timeout and a resend; the first block at caps that cut most rows; side B under a step cap too small for
    most seeds."""
    w = G.traced_pingpong_workload()
    fixed, fixed_lim = T.fixed_pingpong()
    quiet, lossy = A.Config.default(packet_loss_rate=0.0), A.Config.default(packet_loss_rate=LOSS)
    return {
        "loss": (w, quiet, A.Limits(), w, lossy, A.Limits(), G.SEED0, N_BLOCK, 1024, 8),
        "bodies": (w, lossy, A.Limits(), fixed, lossy, fixed_lim, G.SEED0, N_BLOCK, 1024, 8),
        "small_caps": (w, quiet, A.Limits(), w, lossy, A.Limits(), G.SEED0, N_BLOCK, 300, 1),
        "steps": (w, quiet, A.Limits(), w, lossy, limits_like(max_steps=200), G.SEED0, N_BLOCK, 1024, 8),
    }


def side_truth(w, cfg, lim, seed0, n, log_cap, obs_cap):
    """(log rows, log lengths, observation rows, observation counts, results) of one side by the oracle; the results by tests/parity.py's
    expected() convention, which the oracle's own replays must agree with."""
    want = P.expected(w, seed0, n, cfg, lim)
    logs, obs = [], []
    for i in range(n):
        log, r1 = oracle.trace_seed(w, seed0 + i, cfg, lim)
        vals, r2 = oracle.observe_seed(w, seed0 + i, cfg, lim)
        assert r1.astuple() == r2.astuple() == tuple(int(x) for x in want[i]), (seed0 + i, r1.astuple(), want[i])
        logs.append(log); obs.append(vals)
    return R.rows_of(logs, log_cap, np.uint8) + R.rows_of(obs, obs_cap, np.uint64) + (want,)


@functools.lru_cache(maxsize=None)
def block_truth(name, unlimited_b=False):
    """(records, context rows) of a block by the oracle and tests/diverge_ref.py; read-only.  unlimited_b: side B without its step cap —
    what the block's seeds give once resolve rounds have grown it."""
    wa, ca, la, wb, cb, lb, seed0, n, log_cap, obs_cap = blocks()[name]
    if unlimited_b:
        lb = limits_like(lb, max_steps=0)
    a, b = side_truth(wa, ca, la, seed0, n, log_cap, obs_cap), side_truth(wb, cb, lb, seed0, n, log_cap, obs_cap)
    recs, ctx = R.records(np.arange(seed0, seed0 + n, dtype=np.uint64), a[0], b[0], a[1], b[1], a[2], b[2], a[3], b[3], a[4], b[4], WINDOW)
    recs.setflags(write=False); ctx.setflags(write=False)
    return recs, ctx


def count(recs, channel, status):
    return int((recs[channel + "_status"] == status).sum())


def test_the_blocks_hold_the_statuses_they_are_there_for():
    loss, _ = block_truth("loss")
    print("loss", np.bincount(loss["log_status"], minlength=5), np.bincount(loss["obs_status"], minlength=5))
    for st in (R.SAME, R.DIFFER, R.PREFIX):
        assert count(loss, "log", st) >= 3, st
    assert count(loss, "obs", R.SAME) >= 3 and (count(loss, "obs", R.DIFFER) >= 3 or count(loss, "obs", R.PREFIX) >= 3)
    assert count(loss, "obs", R.DIFFER) >= 3 and count(loss, "obs", R.PREFIX) >= 3                 # (this block has both)
    differ = loss[loss["log_status"] == R.DIFFER]
    assert (differ["log_at"] > 0).all() and (differ["log_a"] != differ["log_b"]).all()            # the logs agree up to the first lost message
    bodies, ctx = block_truth("bodies")
    print("bodies", np.bincount(bodies["log_status"], minlength=5), np.bincount(bodies["obs_status"], minlength=5))
    assert count(bodies, "log", R.DIFFER) >= 3 and count(bodies, "obs", R.DIFFER) >= 3
    assert ctx[bodies["obs_status"] == R.DIFFER].any()
    small, _ = block_truth("small_caps")
    print("small_caps", np.bincount(small["log_status"], minlength=5), np.bincount(small["obs_status"], minlength=5))
    assert count(small, "log", R.BEYOND_CAP) >= 3 and count(small, "obs", R.BEYOND_CAP) >= 3 and count(small, "log", R.DIFFER) >= 3
    steps, sctx = block_truth("steps")
    print("steps", np.bincount(steps["log_status"], minlength=5), np.bincount(steps["obs_status"], minlength=5))
    inc = steps["log_status"] == R.INCOMPARABLE
    assert inc.sum() >= 3 and (~inc).sum() >= 3 and (steps["obs_status"][inc] == R.INCOMPARABLE).all()
    assert (steps["b"]["verdict"][inc] == A.STEP_LIMIT).all() and (steps["a"]["verdict"] < A.OVERFLOW).all() and not sctx[inc].any()
    grown, _ = block_truth("steps", True)                                           # ... and resolved they are the first block's seeds
    assert grown.tobytes() == loss.tobytes()
