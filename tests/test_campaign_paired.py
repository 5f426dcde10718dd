"""Paired campaigns (madsim_hip_run_paired_campaign and its _ctx_ / _multi / _seeds_ forms) without a GPU: the two structs, the prototypes
and the constants against the header, the ctypes mirror and the Rust sys file; the host-side truth (tests/paired_ref.py) against plain
Python loops; the library's host fold (madsim_k_fold_paired, csrc/madsim_hip.cpp: no device involved) against that truth, whatever the cut;
the argument errors that need no device; the Python helpers against Fractions computed from the truth.  What the GPU answers is
tests/test_paired_kernels.py's and tests/test_campaign_paired_gpu.py's business."""
import ctypes as C
import inspect
import math
import os
import re
from fractions import Fraction

import numpy as np
import pytest

from madsim_amd import _abi as A
from madsim_amd import runtime, workload
from tests import cheader as H
from tests import paired_ref as R
from tests import stats_ref

E_ARG, E_HIP, E_NOINIT = -1, -2, -3
U64_MAX = (1 << 64) - 1
SEED = 20261019
FORMS = ("madsim_hip_run_paired_campaign", "madsim_hip_ctx_run_paired_campaign", "madsim_hip_run_paired_campaign_multi",
         "madsim_hip_run_seeds_campaign_paired", "madsim_hip_ctx_run_seeds_campaign_paired", "madsim_hip_run_seeds_campaign_paired_multi")


def _no_gpu():
    import torch
    return not torch.cuda.is_available()


def synthetic(rng, n, p_verdict=0.1, p_equal=0.3, wide=False):
    """Two result arrays of n seeds: side B is side A with some metrics moved up or down, some verdicts changed, some runner verdicts."""
    a = np.zeros(n, dtype=A.RESULT_DTYPE)
    top = (1 << 64) if wide else (1 << 40)
    for name in ("clock_ns", "msg_count", "rng_calls", "trace_hash", "obs_hash"):
        a[name] = rng.integers(0, top, n, dtype=np.uint64, endpoint=False)
    a["steps"] = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    b = a.copy()
    for name in ("clock_ns", "msg_count", "rng_calls"):
        move = rng.random(n) >= p_equal
        b[name][move] = rng.integers(0, top, int(move.sum()), dtype=np.uint64, endpoint=False)
    move = rng.random(n) >= p_equal
    b["steps"][move] = rng.integers(0, 1 << 32, int(move.sum()), dtype=np.uint64).astype(np.uint32)
    for side in (a, b):
        ch = rng.random(n) < p_verdict
        side["verdict"][ch] = rng.choice(np.array([1, 2, 3, 4, 5, 6, 7, 9, 0xffffffff], dtype=np.uint32), int(ch.sum()))
    return a, b


# ---- the ABI -------------------------------------------------------------------------------------------------------------------
def _paired_structs():
    """madsim_paired_t is declared in two statements (it holds madsim_metric_t by value): joined here, and laid out with the inner size given."""
    joined = re.sub(r"\bstruct\s+(madsim_paired\w*)\s*\{([^{}]*)\}\s*;\s*typedef\s+struct\s+\1\s+(\w+)\s*;", r"typedef struct \1 {\2} \3;", H.header_text())
    return H.structs(joined)


def test_structs_and_constants_match_the_header():
    S = _paired_structs()
    assert S["madsim_paired_extreme_t"] == [("seed", "uint64_t", 0, False), ("a", "uint64_t", 0, False), ("b", "uint64_t", 0, False)]
    assert S["madsim_paired_t"] == [
        ("include_a", "uint32_t", 0, False), ("include_b", "uint32_t", 0, False), ("top_k", "uint32_t", 0, False), ("reserved", "uint32_t", 0, False),
        ("top", "madsim_paired_extreme_t", 0, True), ("n_paired", "uint64_t", 0, False), ("n_unpaired", "uint64_t", 0, False),
        ("n_incomparable", "uint64_t", 0, False), ("n_top", "uint64_t", 8, False), ("n", "uint64_t", 8, False), ("n_equal", "uint64_t", 4, False),
        ("sum_a_lo", "uint64_t", 4, False), ("sum_a_hi", "uint64_t", 4, False), ("sum_b_lo", "uint64_t", 4, False), ("sum_b_hi", "uint64_t", 4, False),
        ("delta", "madsim_metric_t", 8, False)]
    inner = {"madsim_metric_t": (2080, 8)}
    for name, cls, want_size in (("madsim_paired_extreme_t", A.PairedExtreme, 24), ("madsim_paired_t", A.Paired, 16976)):
        offs, size = H.layout(S[name], inner)
        assert size == want_size == C.sizeof(cls), (name, size, C.sizeof(cls))
        assert [f[0] for f in cls._fields_] == [f[0] for f in S[name]], name
        for fname, _, _, _ in S[name]:
            assert getattr(cls, fname).offset == offs[fname], (name, fname)
    assert A.HEADER_STRUCTS["madsim_paired_extreme_t"] is A.PairedExtreme
    dt = np.dtype(A.PAIRED_EXTREME_DTYPE)
    assert dt.itemsize == 24 and dt.names == ("seed", "a", "b")
    D = {k: int(v.rstrip("u")) for k, v in H.defines().items() if k.startswith(("MADSIM_PAIRED_", "MADSIM_STAT_")) or k == "MADSIM_HIP_ABI_VERSION"}
    assert (D["MADSIM_PAIRED_UP"], D["MADSIM_PAIRED_DOWN"]) == (A.PAIRED_UP, A.PAIRED_DOWN) == (R.UP, R.DOWN) == (0, 1)
    assert D["MADSIM_STAT_MAX_TOP"] == A.STAT_MAX_TOP == R.MAX_TOP and D["MADSIM_STAT_BUCKETS"] == stats_ref.N_BUCKETS
    assert D["MADSIM_HIP_ABI_VERSION"] == A.ABI_VERSION == 7                            # additive: the version stays
    assert A.STAT_NAMES == stats_ref.METRICS
    # the header comment carries the classification, the magnitude rule, the order and the invariants
    raw = open(H.HEADER_PATH).read()
    section = raw[raw.index("---- Paired campaigns"):raw.index("#define MADSIM_PAIRED_UP")]
    for phrase in ("INCOMPARABLE", "PAIRED", "UNPAIRED", "n_paired + n_unpaired + n_incomparable = seeds_run", "b - a", "a - b", "n_equal",
                   "magnitude descending, then seed ascending", "No atomic", "batches launched beyond a stopping one contribute nothing"):
        assert phrase in section, phrase


def test_library_exports_the_entry_points():
    L = runtime.lib()
    fns = H.functions()
    for form, twin in zip(FORMS, ("madsim_hip_run_campaign_diff", "madsim_hip_ctx_run_campaign_diff", "madsim_hip_run_campaign_diff_multi",
                                  "madsim_hip_run_seeds_campaign_diff", "madsim_hip_ctx_run_seeds_campaign_diff", "madsim_hip_run_seeds_campaign_diff_multi")):
        assert fns[form] == ("int", fns[twin][1] + ["madsim_paired_t*"]), form         # the diff twin's arguments plus a trailing madsim_paired_t*
        assert hasattr(L, form), form
        assert len(getattr(L, form).argtypes) == len(fns[form][1]), form
    for name in ("madsim_k_launch_paired", "madsim_k_launch_paired_list", "madsim_k_fold_paired"):
        assert hasattr(L, name), name
    k_h = open(os.path.join(H.ROOT, "madsim_amd", "csrc", "sim_kernel.h")).read()
    K = {k: int(v) for k, v in re.findall(r"^#define MADSIM_K_PAIRED_(\w+) (\d+)u", k_h, re.M)}
    assert K == {"HEAD_WORDS": R.HEAD_WORDS, "WORDS": R.WORDS, "CAND_WORDS": 8 * 256 * 16 * 2}
    assert R.WORDS == 58 + 1024 + 384


def test_the_rust_sys_file_and_the_mirrors_declare_them():
    sys_rs = open(os.path.join(H.ROOT, "bindings", "rust", "madsim-hip-sys", "src", "lib.rs")).read()
    m = re.search(r"pub struct madsim_paired_extreme_t \{(.*?)\n\}", sys_rs, flags=re.S)
    assert re.findall(r"pub (\w+): ([^,\n]+),", m.group(1)) == [("seed", "u64"), ("a", "u64"), ("b", "u64")]
    m = re.search(r"pub struct madsim_paired_t \{(.*?)\n\}", sys_rs, flags=re.S)
    assert re.findall(r"pub (\w+): ([^,\n]+),", m.group(1)) == [
        ("include_a", "u32"), ("include_b", "u32"), ("top_k", "u32"), ("reserved", "u32"), ("top", "*const madsim_paired_extreme_t"), ("n_paired", "u64"),
        ("n_unpaired", "u64"), ("n_incomparable", "u64"), ("n_top", "[u64; 8]"), ("n", "[u64; 8]"), ("n_equal", "[u64; 4]"), ("sum_a_lo", "[u64; 4]"),
        ("sum_a_hi", "[u64; 4]"), ("sum_b_lo", "[u64; 4]"), ("sum_b_hi", "[u64; 4]"), ("delta", "[madsim_metric_t; 8]")]
    for name, val in (("MADSIM_PAIRED_UP", 0), ("MADSIM_PAIRED_DOWN", 1)):
        assert f"pub const {name}: u32 = {val};" in sys_rs, name
    for fn in FORMS:
        assert re.search(r"pub fn %s\([^;]*diff: \*mut madsim_diff_t, pr: \*mut madsim_paired_t\) -> c_int;" % fn, sys_rs), fn
    high = open(os.path.join(H.ROOT, "bindings", "rust", "madsim-hip", "src", "builder.rs")).read()
    assert "pub fn paired_campaign(" in high and "pub fn paired_campaign_seeds(" in high
    assert "madsim_hip_ctx_run_paired_campaign" in high and "madsim_hip_ctx_run_seeds_campaign_paired" in high
    hpp = open(os.path.join(H.ROOT, "include", "madsim_hip.hpp")).read()
    assert re.search(r"paired_against\(const Builder& other, const Workload& wl, const Workload& other_wl", hpp)
    assert "madsim_hip_run_paired_campaign" in hpp and "madsim_hip_run_seeds_campaign_paired" in hpp


def test_the_mirror_has_every_form():
    want = ["workload", "seed0", "total", "other", "config", "other_config", "limits", "other_limits", "include", "other_include", "top_k", "fields",
            "max_listed", "resolve", "batch", "in_flight"]
    assert list(inspect.signature(runtime.run_campaign_paired).parameters) == want
    assert list(inspect.signature(runtime.Context.run_campaign_paired).parameters) == ["self"] + want
    assert list(inspect.signature(runtime.run_campaign_paired_multi).parameters) == ["contexts"] + want
    seeds = [("seeds" if p == "seed0" else p) for p in want if p != "total"]
    assert list(inspect.signature(runtime.run_campaign_paired_seeds).parameters) == seeds
    assert list(inspect.signature(runtime.Context.run_campaign_paired_seeds).parameters) == ["self"] + seeds
    assert list(inspect.signature(runtime.run_campaign_paired_seeds_multi).parameters) == ["contexts"] + seeds
    for fn in (runtime.run_campaign_paired, runtime.run_campaign_paired_seeds, runtime.run_campaign_paired_multi, runtime.Context.run_campaign_paired):
        p = inspect.signature(fn).parameters
        assert (p["include"].default, p["other_include"].default, p["top_k"].default, p["fields"].default, p["max_listed"].default, p["resolve"].default,
                p["batch"].default, p["in_flight"].default) == ((A.PASS,), None, 0, None, 0, None, 0, 0)
    # the existing wrappers keep their parameter lists
    assert list(inspect.signature(runtime.run_campaign_diff).parameters) == [
        "workload", "seed0", "total", "other", "config", "other_config", "limits", "other_limits", "fields", "max_listed", "stop_at_diffs", "batch", "in_flight"]


# ---- the truth against plain Python loops ----------------------------------------------------------------------------------------
def plain_truth(a, b, seeds, include_a, include_b, top_k):
    """paired_truth restated with Python ints, one seed at a time."""
    t = {"n_paired": 0, "n_unpaired": 0, "n_incomparable": 0}
    for name in R.METRICS:
        t[name] = {"n_equal": 0, "sum_a": 0, "sum_b": 0,
                   "dir": [{"n": 0, "min": U64_MAX, "max": 0, "sum": 0, "hist": [0] * 256, "all": []} for _ in range(2)]}
    for i in range(len(a)):
        va, vb = int(a["verdict"][i]), int(b["verdict"][i])
        if va >= 4 or vb >= 4:
            t["n_incomparable"] += 1
            continue
        if not (include_a >> va & 1 and include_b >> vb & 1):
            t["n_unpaired"] += 1
            continue
        t["n_paired"] += 1
        for name in R.METRICS:
            x, y = int(a[name][i]), int(b[name][i])
            M = t[name]
            M["sum_a"] += x
            M["sum_b"] += y
            if x == y:
                M["n_equal"] += 1
                continue
            D, mag = (M["dir"][R.UP], y - x) if y > x else (M["dir"][R.DOWN], x - y)
            D["n"] += 1
            D["min"], D["max"] = min(D["min"], mag), max(D["max"], mag)
            D["sum"] += mag
            D["hist"][stats_ref.bucket(mag)] += 1
            D["all"].append((mag, int(seeds[i]), x, y))
    for name in R.METRICS:
        for D in t[name]["dir"]:
            D["top"] = [(s, x, y) for _, s, x, y in sorted(D.pop("all"), key=lambda e: (-e[0], e[1]))[:top_k]]
            D["hist"] = np.array(D["hist"], dtype=np.uint64)
    return t


def _seeds_of(seed0, n):
    return np.array([(seed0 + i) & U64_MAX for i in range(n)], dtype=np.uint64)


@pytest.mark.parametrize("n", [1, 7, 64, 300])
def test_the_truth_is_the_plain_restatement(n):
    for case, (p, wide) in enumerate(((0.0, False), (0.1, True), (0.6, True))):
        a, b = synthetic(np.random.default_rng([SEED, n, case]), n, p, wide=wide)
        for inc_a, inc_b in ((1, 1), (1, 6), (15, 15), (2, 15)):
            for seed0 in (0, (1 << 40) + 7, (1 << 64) - n):
                for k in (0, 1, 16):
                    want = plain_truth(a, b, _seeds_of(seed0, n), inc_a, inc_b, k)
                    got = R.paired_truth(a, b, seed0, inc_a, inc_b, k)
                    assert R.differences(got, want) == [], (SEED, n, case, inc_a, inc_b, seed0, k)
                    assert got["n_paired"] + got["n_unpaired"] + got["n_incomparable"] == n
                    for name in R.METRICS:
                        assert got[name]["dir"][0]["n"] + got[name]["dir"][1]["n"] + got[name]["n_equal"] == got["n_paired"]
                        assert got[name]["dir"][0]["hist"][0] == got[name]["dir"][1]["hist"][0] == 0           # bucket 0 stays empty
                        for D in got[name]["dir"]:
                            assert int(D["hist"].sum()) == D["n"] and D["sum"] == D["halves"][0] + (D["halves"][1] << 32)
                    # the device words carry the same answer
                    assert R.differences(R.of_words(R.words_of(got, k), n, k), want) == []


# ---- the host fold ---------------------------------------------------------------------------------------------------------------
def _fold_lib():
    L = runtime.lib()
    L.madsim_k_fold_paired.restype, L.madsim_k_fold_paired.argtypes = None, [C.POINTER(A.Paired), C.c_void_p, C.c_uint64]
    return L


def _fresh(inc_a, inc_b, top_k):
    """A madsim_paired_t in the state the campaign starts with, its top array with one guard record behind it."""
    pr = A.Paired()
    pr.include_a, pr.include_b, pr.top_k = inc_a, inc_b, top_k
    raw = np.full((8 * top_k + 1) * 24, 0xA5, dtype=np.uint8)
    pr.top = C.cast(raw.ctypes.data, C.POINTER(A.PairedExtreme)) if top_k else None
    for j in range(8):
        pr.delta[j].min = U64_MAX
    return pr, raw


def fold(a, b, seeds, inc_a, inc_b, top_k, cuts):
    """madsim_k_fold_paired over the device-format words of `a`, `b` cut at `cuts`, from the state the campaign starts with."""
    L = _fold_lib()
    pr, raw = _fresh(inc_a, inc_b, top_k)
    edges = [0] + list(cuts) + [len(a)]
    for lo, hi in zip(edges, edges[1:]):
        words = np.ascontiguousarray(R.words_of(R.paired_truth(a[lo:hi], b[lo:hi], seeds[lo:hi], inc_a, inc_b, top_k), top_k))
        L.madsim_k_fold_paired(C.byref(pr), words.ctypes.data, hi - lo)
    assert raw[8 * top_k * 24:].tobytes() == b"\xa5" * 24, "the fold wrote behind the caller's array"
    top = raw[:8 * top_k * 24].view(A.PAIRED_EXTREME_DTYPE).reshape(4, 2, top_k)
    return R.of_struct(pr, top), pr, top


@pytest.mark.parametrize("p", [0.0, 0.15, 0.7])
def test_fold_gives_the_truth_whatever_the_cut(p):
    n = 1000
    a, b = synthetic(np.random.default_rng([SEED, int(p * 100)]), n, p, wide=True)
    seeds = np.unique(np.random.default_rng([SEED, 5]).integers(0, 1 << 62, 2 * n, dtype=np.uint64))[:n] * np.uint64(3)
    assert len(seeds) == n
    seeds[-1] = U64_MAX
    for inc_a, inc_b in ((1, 1), (15, 6), (15, 15)):
        for k in (0, 1, 2, 15, 16):
            want = R.paired_truth(a, b, seeds, inc_a, inc_b, k)
            for cuts in ((), (1,), (999,), (64, 65, 300, 301, 700), tuple(range(7, n, 7))):
                got, _, _ = fold(a, b, seeds, inc_a, inc_b, k, cuts)
                assert R.differences(got, want) == [], (SEED, p, inc_a, inc_b, k, cuts)
                # ... and the reference's own fold of the batches' truths agrees
                edges = [0] + list(cuts) + [n]
                parts = [R.paired_truth(a[lo:hi], b[lo:hi], seeds[lo:hi], inc_a, inc_b, k) for lo, hi in zip(edges, edges[1:])]
                assert R.differences(R.fold(parts, k), want) == []


def test_fold_merges_ties_by_seed_across_batches():
    """Equal magnitudes everywhere: the K smallest seeds win, whichever batch they came in, and a full row never grows."""
    n = 40
    a = np.zeros(n, dtype=A.RESULT_DTYPE)
    b = a.copy()
    b["clock_ns"] += np.uint64(5)                                                          # all up by 5
    a["rng_calls"] += np.uint64(9)                                                         # all down by 9
    seeds = np.arange(100, 100 + n, dtype=np.uint64)
    for cuts in ((), (3, 20), tuple(range(1, n))):
        got, pr, _ = fold(a, b, seeds, 1, 1, 4, cuts)
        assert got["clock_ns"]["dir"][R.UP]["top"] == [(100 + i, 0, 5) for i in range(4)]
        assert got["rng_calls"]["dir"][R.DOWN]["top"] == [(100 + i, 9, 0) for i in range(4)]
        assert list(pr.n_top) == [4, 0, 0, 0, 0, 0, 0, 4] and got["steps"]["n_equal"] == n
        assert got["clock_ns"]["dir"][R.UP]["sum"] == 5 * n and got["clock_ns"]["dir"][R.DOWN]["min"] == U64_MAX


def test_fold_carries_128_bit_sums():
    n = 50
    a = np.zeros(n, dtype=A.RESULT_DTYPE)
    b = a.copy()
    b["msg_count"] = np.uint64(U64_MAX)                                                    # magnitude 2^64 - 1 in every seed
    got, _, _ = fold(a, b, np.arange(n, dtype=np.uint64), 1, 1, 2, (10, 30))
    D = got["msg_count"]["dir"][R.UP]
    assert D["sum"] == n * U64_MAX and D["sum"] >> 64 != 0 and D["min"] == D["max"] == U64_MAX and int(D["hist"][251]) == n
    assert got["msg_count"]["sum_b"] == n * U64_MAX and got["msg_count"]["sum_a"] == 0


# ---- argument errors ---------------------------------------------------------------------------------------------------------------
def _paired(include_a=1, include_b=1, top_k=0, with_array=True, reserved=0):
    pr = A.Paired()
    pr.include_a, pr.include_b, pr.top_k, pr.reserved = include_a, include_b, top_k, reserved
    pr._keep = (A.PairedExtreme * max(8 * top_k, 1))()
    if with_array and top_k:
        pr.top = C.cast(pr._keep, C.POINTER(A.PairedExtreme))
    return pr


def _diff(fields=A.DIFF_ALL, cap=0, reserved=0):
    d = A.Diff()
    d.fields, d.reserved, d.cap = fields, reserved, cap
    return d


def _call(pr, d=None, flags=0, in_flight=0, reports=(True, True), seeds=None):
    """Every form of the call with the same arguments: the default context, an explicit (null) context, a list of contexts — range and list."""
    L = runtime.lib()
    w, cfg, lim, rep_a, rep_b = workload.pingpong(4, 8), A.Config.default(), A.Limits(), A.Campaign(), A.Campaign()
    arr = (C.c_void_p * 1)(None)
    side = (w.ref(), C.byref(cfg), C.byref(lim))
    tail = (flags, C.byref(rep_a) if reports[0] else None, C.byref(rep_b) if reports[1] else None, C.byref(d) if d is not None else None,
            C.byref(pr) if pr is not None else None)
    lst = np.arange(10, 110, dtype=np.uint64) if seeds is None else seeds
    rng = side + side + (0, 100, 0, in_flight) + tail
    lis = side + side + (lst.ctypes.data_as(C.POINTER(C.c_uint64)), len(lst), 0, in_flight) + tail
    return (L.madsim_hip_run_paired_campaign(*rng), L.madsim_hip_ctx_run_paired_campaign(None, *rng), L.madsim_hip_run_paired_campaign_multi(arr, 1, *rng),
            L.madsim_hip_run_seeds_campaign_paired(*lis), L.madsim_hip_ctx_run_seeds_campaign_paired(None, *lis),
            L.madsim_hip_run_seeds_campaign_paired_multi(arr, 1, *lis))


def test_argument_errors_need_no_gpu():
    """Told before any context is looked at, so these hold with and without a device (the contexts here are null)."""
    bad = (E_ARG,) * 6
    assert _call(None) == bad                                                              # null madsim_paired_t
    assert _call(None, d=_diff()) == bad
    for inc in (0, 16, 1 | 16, 1 << 31):
        assert _call(_paired(include_a=inc)) == bad, inc                                   # nothing included, or a bit at or above 4
        assert _call(_paired(include_b=inc)) == bad, inc
    assert _call(_paired(reserved=1)) == bad
    assert _call(_paired(top_k=17)) == bad                                                 # above MADSIM_STAT_MAX_TOP
    assert _call(_paired(top_k=4, with_array=False)) == bad                                # top_k > 0 without top
    assert _call(_paired(), reports=(False, True)) == bad and _call(_paired(), reports=(True, False)) == bad
    assert _call(_paired(), in_flight=9) == bad
    # diff's own argument errors, when a diff report is asked for
    assert _call(_paired(), d=_diff(fields=0)) == bad and _call(_paired(), d=_diff(fields=128)) == bad
    assert _call(_paired(), d=_diff(reserved=1)) == bad
    d = _diff(cap=4)                                                                       # cap > 0 without records
    assert _call(_paired(), d=d) == bad
    assert _call(_paired(), d=_diff(cap=0), flags=A.CAMPAIGN_STOP_AT_DIFFS) == bad
    # a list that does not ascend
    assert _call(_paired(), seeds=np.array([3, 3], dtype=np.uint64))[3:] == (E_ARG,) * 3
    # the mirror raises for the same things
    w = workload.pingpong(4, 8)
    for kw in (dict(include=()), dict(include=(4,)), dict(other_include=()), dict(top_k=17), dict(top_k=-1), dict(fields=0), dict(fields=128),
               dict(fields=1, max_listed=-1), dict(in_flight=9)):
        with pytest.raises(runtime.MadsimHipError):
            runtime.run_campaign_paired_multi([], w, 0, 100, **kw)
    with pytest.raises(runtime.MadsimHipError):
        runtime.run_campaign_paired_seeds_multi([], w, [5, 4])


def test_a_valid_call_without_a_context_fails_loudly():
    """Null contexts: never a report of nothing that looks like "nothing moved"."""
    for kw in (dict(pr=_paired()), dict(pr=_paired(15, 6, 16)), dict(pr=_paired(), d=_diff()), dict(pr=_paired(), flags=A.CAMPAIGN_STOP_AT_DIFFS)):
        rcs = _call(**kw)
        assert rcs[1] == rcs[2] == rcs[4] == rcs[5] == E_NOINIT
        assert (rcs[0] in (E_NOINIT, E_HIP) and rcs[3] in (E_NOINIT, E_HIP)) or not _no_gpu()


def test_an_empty_list_needs_no_device():
    pr = _paired(15, 15, 2)
    pr.n_paired = pr.n_equal[0] = 7                                                        # (stale outputs are reset)
    rcs = _call(pr, seeds=np.zeros(0, dtype=np.uint64))
    assert rcs[4] == 0 and (pr.n_paired, pr.n_unpaired, pr.n_incomparable, pr.n_equal[0]) == (0, 0, 0, 0)
    assert all(pr.delta[j].min == U64_MAX and pr.delta[j].max == 0 for j in range(8)) and list(pr.n_top) == [0] * 8


# ---- the Python helpers ------------------------------------------------------------------------------------------------------------
def test_the_helpers_are_the_truths_fractions():
    n, k = 600, 5
    a, b = synthetic(np.random.default_rng([SEED, 77]), n, 0.1, wide=True)
    seeds = _seeds_of(1 << 50, n)
    want = R.paired_truth(a, b, seeds, 1, 7, k)
    _, pr, top = fold(a, b, seeds, 1, 7, k, (100, 333))
    rep = runtime.CampaignPaired(pr, top)
    assert R.differences(R.of_report(rep), want) == []
    assert (rep.n_paired, rep.n_unpaired, rep.n_incomparable) == (want["n_paired"], want["n_unpaired"], want["n_incomparable"])
    paired, _ = R.classify(a, b, 1, 7)
    for name in R.METRICS:
        x = [int(v) for v in a[name][paired]]
        y = [int(v) for v in b[name][paired]]
        net = sum(q - p for p, q in zip(x, y))
        assert rep.net_sum(name) == net and isinstance(rep.net_sum(name), int)
        assert rep.mean_delta(name) == Fraction(net, len(x)) and isinstance(rep.mean_delta(name), Fraction)
        assert rep.means(name) == (Fraction(sum(x), len(x)), Fraction(sum(y), len(y)))
        assert rep.means(name)[1] - rep.means(name)[0] == rep.mean_delta(name)
        for d, mags in ((A.PAIRED_UP, sorted(q - p for p, q in zip(x, y) if q > p)), (A.PAIRED_DOWN, sorted(p - q for p, q in zip(x, y) if p > q))):
            for q in (0.01, 0.5, 0.9, 1):
                v = mags[min(max(math.ceil(Fraction(q) * len(mags)), 1), len(mags)) - 1]
                lo, hi = rep.quantile_bounds(name, d, q)
                assert lo <= v <= hi and stats_ref.bucket(lo) == stats_ref.bucket(v) == stats_ref.bucket(hi), (name, d, q)
                assert lo >= mags[0] and hi <= mags[-1]
        assert [tuple(int(v) for v in e) for e in rep.regressions(name)] == want[name]["dir"][R.UP]["top"]
        assert [tuple(int(v) for v in e) for e in rep.improvements(name)] == want[name]["dir"][R.DOWN]["top"]
    empty = runtime.CampaignPaired(*_fresh(1, 1, 0)[:1], np.zeros((4, 2, 0), dtype=A.PAIRED_EXTREME_DTYPE))
    with pytest.raises(ValueError):
        empty.mean_delta("clock_ns")
    with pytest.raises(ValueError):
        empty.quantile_bounds("clock_ns", A.PAIRED_UP, 0.5)
