"""Failure-mode grouping (madsim_hip_run_campaign_groups and its _ctx_ / _multi forms) without a GPU: the two structs, the prototypes and
the constants against the header, the ctypes mirror and the Rust sys file; the host-side truth (tests/groups_ref.py) against a plain-Python
dict; the library's host fold (madsim_k_fold_groups, csrc/madsim_hip.cpp: no device involved) against that truth; the argument errors that
need no device.  What the GPU answers is tests/test_group_kernels.py's and tests/test_campaign_groups_gpu.py's business."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from madsim_amd import _abi as A
from madsim_amd import runtime, workload
from tests import cheader as H
from tests import groups_ref as G

E_ARG, E_HIP, E_NOINIT = -1, -2, -3
U64_MAX = (1 << 64) - 1
SEED = 20261018


def _no_gpu():
    import torch
    return not torch.cuda.is_available()


# ---- the ABI -------------------------------------------------------------------------------------------------------------------
def test_structs_and_constants_match_the_header():
    S = H.structs()
    assert [f[:3] for f in S["madsim_group_t"]] == [("key", "uint64_t", 0), ("verdict", "uint32_t", 0), ("reserved", "uint32_t", 0),
                                                    ("count", "uint64_t", 0), ("first_seed", "uint64_t", 0)]
    assert S["madsim_groups_t"] == [("include", "uint32_t", 0, False), ("key_field", "uint32_t", 0, False), ("groups", "madsim_group_t", 0, True),
                                    ("cap", "uint64_t", 0, False), ("n_groups", "uint64_t", 0, False), ("n_grouped", "uint64_t", 0, False),
                                    ("n_ungrouped", "uint64_t", 0, False)]
    for name, cls, want_size in (("madsim_group_t", A.Group, 32), ("madsim_groups_t", A.Groups, 48)):
        offs, size = H.layout(S[name])
        assert size == want_size == C.sizeof(cls), (name, size, C.sizeof(cls))
        assert [f[0] for f in cls._fields_] == [f[0] for f in S[name]], name
        for fname, _, _, _ in S[name]:
            assert getattr(cls, fname).offset == offs[fname], (name, fname)
    assert (A.Group.verdict.offset, A.Group.count.offset, A.Group.first_seed.offset) == (8, 16, 24)
    assert (A.Groups.groups.offset, A.Groups.cap.offset, A.Groups.n_ungrouped.offset) == (8, 16, 40)
    dt = np.dtype(A.GROUP_DTYPE)
    assert dt.itemsize == 32 and dt.names == ("key", "verdict", "reserved", "count", "first_seed")
    assert all(dt.fields[n][1] == getattr(A.Group, n).offset for n in dt.names)
    D = {k: int(v.rstrip("u")) for k, v in H.defines().items() if k.startswith(("MADSIM_GROUP_", "MADSIM_CAMPAIGN_")) or k == "MADSIM_HIP_ABI_VERSION"}
    assert [D["MADSIM_GROUP_KEY_" + k] for k in ("OBS", "TRACE", "MSGS", "CLOCK", "RNG", "STEPS")] == [0, 1, 2, 3, 4, 5]
    assert (A.GROUP_KEY_OBS, A.GROUP_KEY_TRACE, A.GROUP_KEY_MSGS, A.GROUP_KEY_CLOCK, A.GROUP_KEY_RNG, A.GROUP_KEY_STEPS) == (0, 1, 2, 3, 4, 5)
    assert D["MADSIM_GROUP_KEYS"] == A.GROUP_KEYS == len(A.GROUP_KEY_NAMES) == len(A.GROUP_KEY_FIELDS) == 6
    assert A.GROUP_KEY_FIELDS == G.KEY_FIELDS and A.GROUP_KEY_NAMES == ("obs", "trace", "msgs", "clock", "rng", "steps")
    assert D["MADSIM_GROUP_MAX_BATCH"] == A.GROUP_MAX_BATCH == 1 << 20
    assert D["MADSIM_CAMPAIGN_STOP_AT_GROUPS"] == A.CAMPAIGN_STOP_AT_GROUPS == 8
    flags = [D["MADSIM_CAMPAIGN_" + k] for k in ("STOP_AT_FAILURE", "LIST_RUNNER", "STOP_AT_CAP", "STOP_AT_GROUPS")]
    assert flags == [1, 2, 4, 8]                                                        # distinct bits: the stop flags combine
    assert D["MADSIM_HIP_ABI_VERSION"] == A.ABI_VERSION == 7                            # additive: the version stays


def test_library_exports_the_entry_points():
    L = runtime.lib()
    fns = H.functions()
    stats = fns["madsim_hip_run_campaign_stats"][1]
    assert fns["madsim_hip_run_campaign_groups"] == ("int", stats + ["madsim_groups_t*"])
    assert fns["madsim_hip_ctx_run_campaign_groups"] == ("int", ["madsim_hip_ctx_t*"] + stats + ["madsim_groups_t*"])
    assert fns["madsim_hip_run_campaign_groups_multi"] == ("int", ["madsim_hip_ctx_t* const*", "int"] + stats + ["madsim_groups_t*"])
    for name in ("madsim_hip_run_campaign_groups", "madsim_hip_ctx_run_campaign_groups", "madsim_hip_run_campaign_groups_multi",
                 "madsim_k_launch_groups", "madsim_k_group_slot", "madsim_k_group_slots", "madsim_k_fold_groups", "madsim_k_group_state_new",
                 "madsim_k_group_state_free"):
        assert hasattr(L, name), name
    assert len(L.madsim_hip_run_campaign_groups.argtypes) == len(stats) + 1


def test_the_rust_sys_file_declares_them():
    sys_rs = open(os.path.join(H.ROOT, "bindings", "rust", "madsim-hip-sys", "src", "lib.rs")).read()
    m = re.search(r"pub struct madsim_group_t \{(.*?)\n\}", sys_rs, flags=re.S)
    assert re.findall(r"pub (\w+): ([^,\n]+),", m.group(1)) == [("key", "u64"), ("verdict", "u32"), ("reserved", "u32"), ("count", "u64"), ("first_seed", "u64")]
    m = re.search(r"pub struct madsim_groups_t \{(.*?)\n\}", sys_rs, flags=re.S)
    assert re.findall(r"pub (\w+): ([^,\n]+),", m.group(1)) == [("include", "u32"), ("key_field", "u32"), ("groups", "*const madsim_group_t"), ("cap", "u64"),
                                                                ("n_groups", "u64"), ("n_grouped", "u64"), ("n_ungrouped", "u64")]
    for name, val in (("MADSIM_CAMPAIGN_STOP_AT_GROUPS", 8), ("MADSIM_GROUP_KEY_OBS", 0), ("MADSIM_GROUP_KEY_STEPS", 5), ("MADSIM_GROUP_MAX_BATCH", 1 << 20)):
        assert f"pub const {name}: u32 = {val};" in sys_rs, name
    for fn in ("madsim_hip_run_campaign_groups", "madsim_hip_ctx_run_campaign_groups", "madsim_hip_run_campaign_groups_multi"):
        assert re.search(r"pub fn %s\([^;]*st: \*mut madsim_stats_t, grp: \*mut madsim_groups_t\) -> c_int;" % fn, sys_rs), fn
    high = open(os.path.join(H.ROOT, "bindings", "rust", "madsim-hip", "src", "builder.rs")).read()
    assert "pub fn failure_groups(&self, workload: &Workload, max_groups: usize, include: u32, key_field: u32)" in high
    assert "madsim_hip_ctx_run_campaign_groups" in high
    hpp = open(os.path.join(H.ROOT, "include", "madsim_hip.hpp")).read()
    assert re.search(r"failure_groups\(const Workload& wl, size_t max_groups,\s*uint32_t include = [^,]+,\s*uint32_t key_field = MADSIM_GROUP_KEY_OBS\)", hpp)


def test_the_mirror_has_the_three_forms():
    for fn in (runtime.run_campaign_groups, runtime.run_campaign_groups_multi, runtime.Context.run_campaign_groups):
        p = inspect.signature(fn).parameters
        assert (p["include"].default, p["key"].default, p["stop_at_groups"].default, p["collect"].default, p["stats"].default) == (
            (A.PANIC, A.DEADLOCK, A.TIME_LIMIT), "obs", False, None, None)
        assert "max_groups" in p
    names = list(inspect.signature(runtime.run_campaign_groups).parameters)
    assert names[:8] == ["workload", "seed0", "total", "batch", "in_flight", "stop_at_failure", "config", "limits"]


# ---- the truth against a plain-Python dict ---------------------------------------------------------------------------------------
def synthetic(rng, n, n_keys, verdicts=(0, 1, 2, 3, 4, 5, 7, 0xffffffff)):
    """n results: verdicts drawn from `verdicts`, every key field from a pool of n_keys values that holds 0, 2^64 - 1 and the FNV basis."""
    r = np.zeros(n, dtype=A.RESULT_DTYPE)
    r["verdict"] = rng.choice(np.array(verdicts, dtype=np.uint32), n)
    pool = np.concatenate([np.array([0, U64_MAX, G.FNV_BASIS], dtype=np.uint64), rng.integers(0, 1 << 64, max(n_keys - 3, 0), dtype=np.uint64)])[:max(n_keys, 1)]
    for name in G.KEY_FIELDS[:5]:
        r[name] = rng.choice(pool, n)
    r["steps"] = rng.integers(0, 4, n)
    return r


def dict_groups(results, seed0, include, key_field):
    """all_groups in plain Python: a dict in insertion order."""
    seen = {}
    for i in range(len(results)):
        v = int(results["verdict"][i])
        if v < 4 and include >> v & 1:
            sig = (v, int(results[G.KEY_FIELDS[key_field]][i]))
            if sig in seen:
                seen[sig][0] += 1
            else:
                seen[sig] = [1, seed0 + i]
    return [(v, k, c, s) for (v, k), (c, s) in seen.items()]


@pytest.mark.parametrize("n", [1, 7, 64, 300, 2000])
def test_the_truth_is_a_dict_in_insertion_order(n):
    for case, n_keys in enumerate((1, 3, 5, 50, 5000)):
        results = synthetic(np.random.default_rng([SEED, n, case]), n, n_keys)
        for include in (1, 2, 4, 8, G.FAILURES, G.ALL):
            for key_field in range(6):
                at0 = dict_groups(results, 0, include, key_field)
                for seed0 in (0, (1 << 40) + 7, (1 << 64) - n):
                    want = [(v, k, c, seed0 + s) for v, k, c, s in at0]
                    assert G.all_groups(results, seed0, include, key_field) == want, (SEED, n, case, include, key_field, seed0)
                    assert [g[3] for g in want] == sorted({g[3] for g in want})            # first_seed: unique, ascending
                for cap in (0, 1, len(want), max(len(want) - 1, 0), len(want) + 5):
                    t = G.groups_truth(results, seed0, include, key_field, cap)
                    assert t["groups"] == want[:cap] and t["n_grouped"] + t["n_ungrouped"] == int(G.counted(results, include).sum())
                    assert t["n_ungrouped"] == sum(g[2] for g in want[cap:])


def test_runner_verdicts_and_same_key_two_verdicts():
    r = np.zeros(8, dtype=A.RESULT_DTYPE)
    r["verdict"] = [1, 2, 4, 1, 7, 0xffffffff, 2, 5]
    r["obs_hash"] = 42
    assert G.all_groups(r, 100, G.ALL, 0) == [(1, 42, 2, 100), (2, 42, 2, 101)]            # one key, two verdicts: two groups; 4, 5, 7, 2^32 - 1: never
    assert G.all_groups(r, 100, 0b0100, 0) == [(2, 42, 2, 101)]
    assert G.all_groups(r, 100, 0b0001, 0) == []


# ---- the host fold ---------------------------------------------------------------------------------------------------------------
def _fold_lib():
    L = runtime.lib()
    L.madsim_k_group_state_new.restype, L.madsim_k_group_state_new.argtypes = C.c_void_p, []
    L.madsim_k_group_state_free.restype, L.madsim_k_group_state_free.argtypes = None, [C.c_void_p]
    L.madsim_k_fold_groups.restype, L.madsim_k_fold_groups.argtypes = None, [C.POINTER(A.Groups), C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64]
    return L


def entries_of(results, seed0, include, key_field):
    """A batch's entries as the device leaves them (every group of the batch, any order): here ascending, the callers shuffle."""
    every = G.all_groups(results, seed0, include, key_field)
    e = np.zeros(len(every), dtype=A.GROUP_DTYPE)
    for j, (v, k, c, s) in enumerate(every):
        e[j] = (k, v, 0, c, s)
    return e


def cut(results, seed0, include, key_field, batch):
    """[(the batch's entries, its first seed)] of `results` cut into batches of `batch`."""
    return [(entries_of(results[lo:lo + batch], (seed0 + lo) & U64_MAX, include, key_field), (seed0 + lo) & U64_MAX) for lo in range(0, len(results), batch)]


def fold(results, seed0, include, key_field, cap, batch, shuffle=None, batches=None):
    """madsim_k_fold_groups over `results` cut into batches of `batch` (or over `batches`, a cut() made earlier), from the state
    run_campaign_impl starts with; (answer, raw bytes)."""
    L = _fold_lib()
    batches = batches if batches is not None else cut(results, seed0, include, key_field, batch)
    arr = np.full(cap + 1, 0xA5, dtype=np.uint8).repeat(32).view(A.GROUP_DTYPE)             # one entry of guard behind the caller's array
    grp = A.Groups()
    grp.include, grp.key_field, grp.cap = include, key_field, cap
    grp.groups = arr.ctypes.data_as(C.POINTER(A.Group)) if cap else None
    state = L.madsim_k_group_state_new()
    try:
        for e, first in batches:
            if shuffle is not None:
                e = e[shuffle.permutation(len(e))]
            e = np.ascontiguousarray(e)
            L.madsim_k_fold_groups(C.byref(grp), state, e.ctypes.data, len(e), first)
    finally:
        L.madsim_k_group_state_free(state)
    assert arr[cap:].tobytes() == b"\xa5" * 32, "the fold wrote behind the caller's array"
    assert grp.n_groups <= cap
    got = {"groups": G.of_array(arr[:grp.n_groups]), "n_grouped": int(grp.n_grouped), "n_ungrouped": int(grp.n_ungrouped)}
    return got, arr[:grp.n_groups].tobytes()


@pytest.mark.parametrize("n_keys", [1, 4, 40, 3000])
def test_fold_gives_the_truth_whatever_the_cut(n_keys):
    n = 1000
    results = synthetic(np.random.default_rng([SEED, n_keys]), n, n_keys)
    shuffle = np.random.default_rng([SEED, n_keys, 1])
    for include, key_field in ((G.FAILURES, 0), (G.ALL, 0), (G.ALL, 2), (0b0001, 5), (0b0100, 1)):
        every = G.all_groups(results, 77, include, key_field)
        cuts = {batch: cut(results, 77, include, key_field, batch) for batch in (1, 7, 100, n)}
        for cap in sorted({0, 1, len(every), max(len(every) - 1, 0), len(every) + 3}):
            want = G.groups_truth(results, 77, include, key_field, cap)
            first = None
            for batch in (1, 7, 100, n):
                got, raw = fold(results, 77, include, key_field, cap, batch, batches=cuts[batch])
                assert got == want, (SEED, n_keys, include, key_field, cap, batch)
                shuffled, raw2 = fold(results, 77, include, key_field, cap, batch, shuffle, cuts[batch])
                assert shuffled == want and raw2 == raw, (SEED, n_keys, include, key_field, cap, batch, "shuffled")
                first = first or raw
                assert raw == first                                                        # the same bytes whatever the cut
            assert want["n_grouped"] + want["n_ungrouped"] == int(G.counted(results, include).sum())


def test_fold_never_lists_a_signature_that_appears_after_the_list_is_full():
    """cap = 2; signature C first appears in batch 2, when the list is full, and recurs in batches 3 and 4: never listed, always ungrouped —
    while A and B, listed, keep collecting their later seeds."""
    r = np.zeros(40, dtype=A.RESULT_DTYPE)
    r["verdict"] = 2
    keys = {"A": 0, "B": U64_MAX, "C": G.FNV_BASIS, "D": 5}
    layout = "AAAAAAAAAA" + "ABABABABBB" + "CCACCBCCCD" + "CCCCCAAAAC"
    r["obs_hash"] = [keys[c] for c in layout]
    got, _ = fold(r, 1000, G.FAILURES, 0, 2, 10)
    assert got == {"groups": [(2, 0, layout.count("A"), 1000), (2, U64_MAX, layout.count("B"), 1011)], "n_grouped": layout.count("A") + layout.count("B"),
                   "n_ungrouped": layout.count("C") + layout.count("D")}
    assert got == G.groups_truth(r, 1000, G.FAILURES, 0, 2)
    full, _ = fold(r, 1000, G.FAILURES, 0, 4, 10)
    assert [g[1] for g in full["groups"]] == [0, U64_MAX, G.FNV_BASIS, 5] and full["n_ungrouped"] == 0


def test_fold_edge_signatures_and_seeds():
    """One key under two verdicts, keys 0 and 2^64 - 1, and a range that ends with seed 2^64 - 1."""
    n = 64
    r = np.zeros(n, dtype=A.RESULT_DTYPE)
    r["verdict"] = np.arange(n) % 4
    r["obs_hash"] = np.where(np.arange(n) % 8 < 4, 0, U64_MAX).astype(np.uint64)
    seed0 = (1 << 64) - n
    want = G.groups_truth(r, seed0, G.ALL, 0, 8)
    assert len(want["groups"]) == 8 and {g[1] for g in want["groups"]} == {0, U64_MAX} and {g[0] for g in want["groups"]} == {0, 1, 2, 3}
    assert [g[3] for g in want["groups"]] == [seed0 + j for j in range(8)] and all(g[2] == 8 for g in want["groups"])
    for batch in (1, 7, 100):
        got, _ = fold(r, seed0, G.ALL, 0, 8, batch, np.random.default_rng([SEED, batch]))
        assert got == want, batch
    last, _ = fold(r[-1:], U64_MAX, G.ALL, 0, 1, 1)
    assert last["groups"] == [(3, U64_MAX, 1, U64_MAX)]


def test_group_slot_is_a_pure_function_in_range():
    L = runtime.lib()
    L.madsim_k_group_slot.restype, L.madsim_k_group_slot.argtypes = C.c_uint64, [C.c_uint64, C.c_uint32, C.c_uint64]
    L.madsim_k_group_slots.restype, L.madsim_k_group_slots.argtypes = C.c_uint64, [C.c_uint64]
    for count, want in ((1, 128), (64, 128), (65, 256), (1025, 4096), (65_536, 131_072), (65_537, 262_144), (1 << 20, 1 << 21)):
        assert L.madsim_k_group_slots(count) == want                                    # a power of two, at least 2 x the batch: load <= 0.5
    rng = np.random.default_rng(SEED)
    for slots in (128, 4096, 1 << 21):
        keys = [0, U64_MAX, G.FNV_BASIS] + [int(k) for k in rng.integers(0, 1 << 64, 500, dtype=np.uint64)]
        at = [[L.madsim_k_group_slot(k, v, slots) for k in keys] for v in range(4)]
        assert all(0 <= s < slots for row in at for s in row)
        assert at == [[L.madsim_k_group_slot(k, v, slots) for k in keys] for v in range(4)]
        assert len({row[0] for row in at}) > 1                                          # key 0 under different verdicts starts apart
        assert len(set(at[2])) > len(keys) // 2 or slots == 128                         # and the keys spread


# ---- argument errors ---------------------------------------------------------------------------------------------------------------
def _groups(include=G.FAILURES, key_field=0, cap=4, with_array=True):
    grp = A.Groups()
    grp.include, grp.key_field, grp.cap = include, key_field, cap
    grp._keep = (A.Group * max(cap, 1))()
    if with_array:
        grp.groups = C.cast(grp._keep, C.POINTER(A.Group))
    return grp


def _stats(include=1, top_k=0):
    st = A.Stats()
    st.include, st.top_k = include, top_k
    return st


def _collect(cap, with_array=True):
    col = A.Collect()
    col.cap = cap
    col._keep = (A.Failure * max(cap, 1))()
    if with_array:
        col.failures = C.cast(col._keep, C.POINTER(A.Failure))
    return col


def _call(grp, col=None, st=None, flags=0, in_flight=0, total=100, batch=0):
    """Every form of the call with the same arguments: the default context, an explicit (null) context, a list of contexts."""
    L = runtime.lib()
    w, cfg, lim, rep = workload.pingpong(4, 8), A.Config.default(), A.Limits(), A.Campaign()
    ptr = lambda x: C.byref(x) if x is not None else None                               # noqa: E731
    arr = (C.c_void_p * 1)(None)
    tail = (w.ref(), C.byref(cfg), 0, total, batch, in_flight, flags, C.byref(lim), C.byref(rep), ptr(col), ptr(st), ptr(grp))
    return (L.madsim_hip_run_campaign_groups(*tail), L.madsim_hip_ctx_run_campaign_groups(None, *tail), L.madsim_hip_run_campaign_groups_multi(arr, 1, *tail))


def test_argument_errors_need_no_gpu():
    """Told before any context is looked at, so these hold with and without a device (the contexts here are null)."""
    assert _call(None) == (E_ARG,) * 3                                                     # null grp
    assert _call(_groups(include=0)) == (E_ARG,) * 3                                       # nothing grouped
    for bad in (16, 2 | 16, 1 << 7, 1 << 31):
        assert _call(_groups(include=bad)) == (E_ARG,) * 3, bad                            # a bit at or above 4: runner verdicts are never grouped
    for bad in (6, 7, 0xffffffff):
        assert _call(_groups(key_field=bad)) == (E_ARG,) * 3, bad                          # unknown key_field
    assert _call(_groups(cap=4, with_array=False)) == (E_ARG,) * 3                         # cap > 0 without groups
    assert _call(_groups(cap=0), flags=A.CAMPAIGN_STOP_AT_GROUPS) == (E_ARG,) * 3          # STOP_AT_GROUPS with cap == 0
    assert _call(_groups(), total=(1 << 20) + 1, batch=(1 << 20) + 1) == (E_ARG,) * 3      # min(batch, total) above 2^20 seeds
    assert _call(_groups(), total=1 << 30, batch=1 << 21) == (E_ARG,) * 3
    assert _call(_groups(), in_flight=9) == (E_ARG,) * 3
    # the collecting and statistics forms' own errors when col / st are given
    assert _call(_groups(), col=_collect(4, with_array=False)) == (E_ARG,) * 3
    assert _call(_groups(), col=_collect(0), flags=A.CAMPAIGN_STOP_AT_CAP) == (E_ARG,) * 3
    assert _call(_groups(), st=_stats(include=0)) == (E_ARG,) * 3
    assert _call(_groups(), st=_stats(top_k=4)) == (E_ARG,) * 3                            # top_k > 0 without top
    assert _call(_groups(), st=_stats(), col=_collect(4, with_array=False)) == (E_ARG,) * 3
    L = runtime.lib()
    w, cfg, lim, grp = workload.pingpong(4, 8), A.Config.default(), A.Limits(), _groups()
    assert L.madsim_hip_run_campaign_groups(w.ref(), C.byref(cfg), 0, 100, 0, 0, 0, C.byref(lim), None, None, None, C.byref(grp)) == E_ARG      # null report
    # the mirror raises for the same things
    for kw in (dict(include=()), dict(include=(A.OVERFLOW,)), dict(key="pc"), dict(max_groups=-1), dict(max_groups=0, stop_at_groups=True),
               dict(in_flight=9), dict(batch=(1 << 20) + 1, total=1 << 21), dict(stats=((), 0)), dict(collect=0, stop_at_cap=True)):
        total = kw.pop("total", 100)
        with pytest.raises(runtime.MadsimHipError):
            runtime.run_campaign_groups_multi([], w, 0, total, **kw)


def test_a_valid_call_without_a_context_fails_loudly():
    """Null contexts: never groups of nothing that look like an answer.  A batch of exactly 2^20 seeds is a valid size."""
    for kw in (dict(grp=_groups()), dict(grp=_groups(G.ALL, 5, 0)), dict(grp=_groups(), col=_collect(4), st=_stats()),
               dict(grp=_groups(), flags=A.CAMPAIGN_STOP_AT_GROUPS | A.CAMPAIGN_STOP_AT_FAILURE), dict(grp=_groups(), total=1 << 30, batch=1 << 20)):
        rcs = _call(**kw)
        assert rcs[1] == E_NOINIT and rcs[2] == E_NOINIT
        assert rcs[0] in (E_NOINIT, E_HIP) or not _no_gpu()
    if _no_gpu():
        w = workload.pingpong(4, 8)
        for kw in (dict(), dict(key="msgs", include=(A.PASS, A.DEADLOCK)), dict(collect=16, stats=((A.PASS,), 4))):
            with pytest.raises(runtime.MadsimHipError, match="HIP|context|initiali"):
                runtime.run_campaign_groups(w, 0, 1000, **kw)


# ---- the end-to-end range, on the CPU ------------------------------------------------------------------------------------------------
def test_the_traced_pingpong_range_has_the_modes():
    """What tests/test_campaign_groups_gpu.py relies on: at least three groups over both PASS and DEADLOCK, named by what was traced."""
    _, _, want = G.traced_pingpong()
    every = G.all_groups(want, G.SEED0, G.ALL, 0)
    assert len(every) >= 3 and {g[0] for g in every} >= {A.PASS, A.DEADLOCK}
    dead = G.all_groups(want, G.SEED0, G.FAILURES, 0)
    assert len(dead) == 3 and {g[0] for g in dead} == {A.DEADLOCK}                          # pair 0 stuck, pair 1 stuck, both stuck
    assert G.FNV_BASIS in {g[1] for g in dead}                                              # both stuck: nothing traced
    assert sum(g[2] for g in every) == G.TOTAL and set(want["verdict"].tolist()) == {A.PASS, A.DEADLOCK}
