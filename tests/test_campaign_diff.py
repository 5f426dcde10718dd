"""Differential campaigns (madsim_hip_run_campaign_diff and its _ctx_ / _multi forms) without a GPU: the two structs, the prototypes and the
constants against the header, the ctypes mirror and the Rust sys file; the host-side truth (tests/diff_ref.py) against plain Python ints;
the library's host fold (madsim_k_fold_diff, csrc/madsim_hip.cpp: no device involved) against that truth; the argument errors that need no
device.  What the GPU answers is tests/test_diff_kernels.py's and tests/test_campaign_diff_gpu.py's business."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from madsim_amd import _abi as A
from madsim_amd import runtime, workload
from tests import cheader as H
from tests import diff_ref as R

E_ARG, E_HIP, E_NOINIT = -1, -2, -3
U64_MAX = (1 << 64) - 1
SEED = 20261018


def _no_gpu():
    import torch
    return not torch.cuda.is_available()


# ---- the ABI -------------------------------------------------------------------------------------------------------------------
def _diff_structs():
    """The two structs are declared in two statements each (one holds madsim_result_t by value, the other a two-dimensional array): joined
    here, the matrix flattened to the 64 words it is, and laid out with the inner struct's size given."""
    joined = re.sub(r"\bstruct\s+(madsim_diff\w*)\s*\{([^{}]*)\}\s*;\s*typedef\s+struct\s+\1\s+(\w+)\s*;", r"typedef struct \1 {\2} \3;", H.header_text())
    assert "transitions[8][8]" in joined
    return H.structs(joined.replace("transitions[8][8]", "transitions[64]"))


def test_structs_and_constants_match_the_header():
    S = _diff_structs()
    assert [f[:2] for f in S["madsim_diff_record_t"]] == [("seed", "uint64_t"), ("a", "madsim_result_t"), ("b", "madsim_result_t")]
    assert S["madsim_diff_t"] == [("fields", "uint32_t", 0, False), ("reserved", "uint32_t", 0, False), ("records", "madsim_diff_record_t", 0, True),
                                  ("cap", "uint64_t", 0, False), ("n_listed", "uint64_t", 0, False), ("n_compared", "uint64_t", 0, False),
                                  ("n_incomparable", "uint64_t", 0, False), ("n_differ", "uint64_t", 0, False), ("n_by_field", "uint64_t", 8, False),
                                  ("transitions", "uint64_t", 64, False)]
    inner = {"madsim_result_t": (48, 8)}
    for name, cls, want_size in (("madsim_diff_record_t", A.DiffRecord, 104), ("madsim_diff_t", A.Diff, 632)):
        offs, size = H.layout(S[name], inner)
        assert size == want_size == C.sizeof(cls), (name, size, C.sizeof(cls))
        assert [f[0] for f in cls._fields_] == [f[0] for f in S[name]], name
        for fname, _, _, _ in S[name]:
            assert getattr(cls, fname).offset == offs[fname], (name, fname)
    assert (A.DiffRecord.a.offset, A.DiffRecord.b.offset) == (8, 56)
    assert (A.Diff.records.offset, A.Diff.n_by_field.offset, A.Diff.transitions.offset) == (8, 56, 120)
    d = A.Diff()
    assert len(d.transitions) == 8 and len(d.transitions[0]) == 8 and len(d.n_by_field) == 8
    dt = np.dtype(A.DIFF_RECORD_DTYPE)
    assert dt.itemsize == 104 and dt.names == ("seed", "a", "b") and (dt.fields["a"][1], dt.fields["b"][1]) == (8, 56)
    assert dt.fields["a"][0] == np.dtype(A.RESULT_DTYPE)
    D = {k: int(v.rstrip("u")) for k, v in H.defines().items() if k.startswith(("MADSIM_DIFF_", "MADSIM_CAMPAIGN_")) or k == "MADSIM_HIP_ABI_VERSION"}
    bits = [D["MADSIM_DIFF_" + k] for k in ("VERDICT", "STEPS", "CLOCK", "MSGS", "RNG", "TRACE", "OBS")]
    assert bits == [1, 2, 4, 8, 16, 32, 64] == [A.DIFF_VERDICT, A.DIFF_STEPS, A.DIFF_CLOCK, A.DIFF_MSGS, A.DIFF_RNG, A.DIFF_TRACE, A.DIFF_OBS]
    assert D["MADSIM_DIFF_ALL"] == A.DIFF_ALL == sum(bits) == R.ALL and D["MADSIM_DIFF_FIELDS"] == A.DIFF_FIELDS == len(A.DIFF_FIELD_NAMES) == 7
    assert A.DIFF_FIELD_NAMES == R.FIELDS == tuple(n for n, _ in A.RESULT_DTYPE)           # bit i is the result's i-th field
    assert D["MADSIM_CAMPAIGN_STOP_AT_DIFFS"] == A.CAMPAIGN_STOP_AT_DIFFS == 16
    flags = [D["MADSIM_CAMPAIGN_" + k] for k in ("STOP_AT_FAILURE", "LIST_RUNNER", "STOP_AT_CAP", "STOP_AT_GROUPS", "STOP_AT_DIFFS")]
    assert flags == [1, 2, 4, 8, 16]
    assert D["MADSIM_HIP_ABI_VERSION"] == A.ABI_VERSION == 7                            # additive: the version stays
    assert R.RUNNER == A.OVERFLOW


def test_library_exports_the_entry_points():
    L = runtime.lib()
    fns = H.functions()
    side = ["const madsim_workload_t*", "const madsim_config_t*", "const madsim_limits_t*"]
    tail = side + side + ["uint64_t", "uint64_t", "uint64_t", "uint32_t", "uint32_t", "madsim_campaign_t*", "madsim_campaign_t*", "madsim_diff_t*"]
    assert fns["madsim_hip_run_campaign_diff"] == ("int", tail)
    assert fns["madsim_hip_ctx_run_campaign_diff"] == ("int", ["madsim_hip_ctx_t*"] + tail)
    assert fns["madsim_hip_run_campaign_diff_multi"] == ("int", ["madsim_hip_ctx_t* const*", "int"] + tail)
    for name in ("madsim_hip_run_campaign_diff", "madsim_hip_ctx_run_campaign_diff", "madsim_hip_run_campaign_diff_multi", "madsim_k_launch_diff",
                 "madsim_k_fold_diff"):
        assert hasattr(L, name), name
    assert len(L.madsim_hip_run_campaign_diff.argtypes) == len(tail)
    assert len(L.madsim_hip_run_campaign_diff_multi.argtypes) == len(tail) + 2
    k_h = open(os.path.join(H.ROOT, "madsim_amd", "csrc", "sim_kernel.h")).read()
    assert re.search(r"^#define MADSIM_K_DIFF_WORDS (\d+)u", k_h, re.M).group(1) == str(R.WORDS)


def test_the_rust_sys_file_and_the_mirrors_declare_them():
    sys_rs = open(os.path.join(H.ROOT, "bindings", "rust", "madsim-hip-sys", "src", "lib.rs")).read()
    m = re.search(r"pub struct madsim_diff_record_t \{(.*?)\n\}", sys_rs, flags=re.S)
    assert re.findall(r"pub (\w+): ([^,\n]+),", m.group(1)) == [("seed", "u64"), ("a", "madsim_result_t"), ("b", "madsim_result_t")]
    m = re.search(r"pub struct madsim_diff_t \{(.*?)\n\}", sys_rs, flags=re.S)
    assert re.findall(r"pub (\w+): ([^,\n]+),", m.group(1)) == [
        ("fields", "u32"), ("reserved", "u32"), ("records", "*const madsim_diff_record_t"), ("cap", "u64"), ("n_listed", "u64"), ("n_compared", "u64"),
        ("n_incomparable", "u64"), ("n_differ", "u64"), ("n_by_field", "[u64; 8]"), ("transitions", "[[u64; 8]; 8]")]
    for name, val in (("MADSIM_CAMPAIGN_STOP_AT_DIFFS", 16), ("MADSIM_DIFF_VERDICT", 1), ("MADSIM_DIFF_OBS", 64), ("MADSIM_DIFF_ALL", 127), ("MADSIM_DIFF_FIELDS", 7)):
        assert f"pub const {name}: u32 = {val};" in sys_rs, name
    for fn in ("madsim_hip_run_campaign_diff", "madsim_hip_ctx_run_campaign_diff", "madsim_hip_run_campaign_diff_multi"):
        assert re.search(r"pub fn %s\([^;]*outA: \*mut madsim_campaign_t, outB: \*mut madsim_campaign_t, diff: \*mut madsim_diff_t\) -> c_int;" % fn, sys_rs), fn
    high = open(os.path.join(H.ROOT, "bindings", "rust", "madsim-hip", "src", "builder.rs")).read()
    assert "pub fn diff_campaign(&self, workload: &Workload, other: &Builder, other_workload: &Workload, fields: u32, max_listed: usize)" in high
    assert "madsim_hip_ctx_run_campaign_diff" in high
    hpp = open(os.path.join(H.ROOT, "include", "madsim_hip.hpp")).read()
    assert re.search(r"diff_against\(const Builder& other, const Workload& wl, const Workload& other_wl,\s*uint32_t fields = MADSIM_DIFF_ALL,\s*size_t max_listed = 0\)", hpp)


def test_the_mirror_has_the_three_forms():
    for fn in (runtime.run_campaign_diff, runtime.run_campaign_diff_multi, runtime.Context.run_campaign_diff):
        p = inspect.signature(fn).parameters
        assert (p["other"].default, p["other_config"].default, p["other_limits"].default, p["fields"].default, p["max_listed"].default,
                p["stop_at_diffs"].default, p["batch"].default, p["in_flight"].default) == (None, None, None, A.DIFF_ALL, 0, False, 0, 0)
    assert list(inspect.signature(runtime.run_campaign_diff).parameters) == [
        "workload", "seed0", "total", "other", "config", "other_config", "limits", "other_limits", "fields", "max_listed", "stop_at_diffs", "batch", "in_flight"]


# ---- the truth against plain Python ints -----------------------------------------------------------------------------------------
def plain_truth(a, b, seed0, fields, cap):
    """diff_truth restated with Python ints, one seed at a time."""
    t = {"n_listed": 0, "n_compared": 0, "n_incomparable": 0, "n_differ": 0, "n_by_field": [0] * 8, "transitions": [[0] * 8 for _ in range(8)]}
    recs = []
    for i in range(len(a)):
        va, vb = int(a["verdict"][i]), int(b["verdict"][i])
        t["transitions"][min(va, 7)][min(vb, 7)] += 1
        if va >= 4 or vb >= 4:
            t["n_incomparable"] += 1
            continue
        t["n_compared"] += 1
        d = [k for k, name in enumerate(R.FIELDS) if fields >> k & 1 and int(a[name][i]) != int(b[name][i])]
        for k in d:
            t["n_by_field"][k] += 1
        if d:
            t["n_differ"] += 1
            if len(recs) < cap:
                recs.append(((seed0 + i) & U64_MAX, a[i].tobytes(), b[i].tobytes()))
    t["n_listed"] = len(recs)
    t["records"] = b"".join(int(s).to_bytes(8, "little") + ra + rb for s, ra, rb in recs)
    return t


@pytest.mark.parametrize("n", [1, 7, 64, 300])
def test_the_truth_is_the_plain_restatement(n):
    for case, p in enumerate((0.0, 0.05, 0.5, 1.0)):
        a, b = R.synthetic(np.random.default_rng([SEED, n, case]), n, p)
        for fields in (1, 2, 4, 8, 16, 32, 64, R.ALL, R.ALL & ~32, 5):
            for seed0 in (0, (1 << 40) + 7, (1 << 64) - n):
                for cap in (0, 1, n, n + 3):
                    want = plain_truth(a, b, seed0, fields, cap)
                    got = R.diff_truth(a, b, seed0, fields, cap)
                    assert got == want, (SEED, n, case, fields, seed0, cap)
                    assert got["n_compared"] + got["n_incomparable"] == n == sum(map(sum, got["transitions"]))
        w = R.words_of(a, b, R.ALL)
        assert int(w[0]) == R.diff_truth(a, b, 0, R.ALL, 0)["n_differ"]
        assert sum(R.wave_counts(a, b, R.ALL)[1]) == int(w[0])


def test_transition_sums_are_the_sides_verdict_histograms():
    a, b = R.synthetic(np.random.default_rng([SEED, 9]), 2000, 0.3)
    t = np.array(R.diff_truth(a, b, 0, R.ALL, 0)["transitions"])
    assert t.sum(axis=1).tolist() == np.bincount(np.minimum(a["verdict"], 7), minlength=8).tolist()
    assert t.sum(axis=0).tolist() == np.bincount(np.minimum(b["verdict"], 7), minlength=8).tolist()


# ---- the host fold ---------------------------------------------------------------------------------------------------------------
def _fold_lib():
    L = runtime.lib()
    L.madsim_k_fold_diff.restype, L.madsim_k_fold_diff.argtypes = C.c_uint64, [C.POINTER(A.Diff), C.c_void_p, C.c_uint64, C.c_void_p]
    return L


def cut(a, b, seed0, fields, batch):
    """[(device-format words, every record, seeds)] of `a`, `b` cut into batches of `batch`."""
    out = []
    for lo in range(0, len(a), batch):
        sa, sb = a[lo:lo + batch], b[lo:lo + batch]
        recs = R.records_of(sa, sb, (seed0 + lo) & U64_MAX, np.nonzero(R.masks(sa, sb, fields))[0])
        out.append((np.ascontiguousarray(R.words_of(sa, sb, fields)), recs, len(sa)))
    return out


def fold(a, b, seed0, fields, cap, batch, copy_here=False, batches=None):
    """madsim_k_fold_diff over the device-format words (and records) of `a`, `b` cut into batches of `batch` (or over `batches`, a cut() made
    earlier), from the state run_variants_impl starts with; (answer, the `take` of every batch).  copy_here: the fold is given no
    records and the caller copies them, as the library does from device memory."""
    L = _fold_lib()
    arr = np.full(cap + 1, 0xA5, dtype=np.uint8).repeat(104).view(A.DIFF_RECORD_DTYPE)             # one record of guard behind the caller's array
    d = A.Diff()
    d.fields, d.cap = fields, cap
    d.records = arr.ctypes.data_as(C.POINTER(A.DiffRecord)) if cap else None
    takes = []
    for words, every, n in batches if batches is not None else cut(a, b, seed0, fields, batch):
        recs = np.ascontiguousarray(every[:min(cap, n)])                                            # what diff_write_kernel leaves: at most the flight's room
        at = int(d.n_listed)
        take = int(L.madsim_k_fold_diff(C.byref(d), words.ctypes.data, n, None if copy_here or not len(recs) else recs.ctypes.data))
        assert take == int(d.n_listed) - at and take <= len(recs)
        if copy_here and take:
            arr[at:at + take] = recs[:take]
        takes.append(take)
    assert arr[cap:].tobytes() == b"\xa5" * 104, "the fold wrote behind the caller's array"
    return R.of_struct(d, arr), takes


@pytest.mark.parametrize("p", [0.0, 0.02, 0.6])
def test_fold_gives_the_truth_whatever_the_cut(p):
    n = 1000
    a, b = R.synthetic(np.random.default_rng([SEED, int(p * 100)]), n, p)
    for fields in (R.ALL, 1, R.ALL & ~32):
        n_differ = R.diff_truth(a, b, 77, fields, 0)["n_differ"]
        cuts = {batch: cut(a, b, 77, fields, batch) for batch in (1, 7, 100_000)}
        for cap in sorted({0, 1, n_differ, max(n_differ - 1, 0), n_differ + 3}):
            want = R.diff_truth(a, b, 77, fields, cap)
            for batch in (1, 7, 100_000):
                for copy_here in (False, True):
                    got, _ = fold(a, b, 77, fields, cap, batch, copy_here, cuts[batch])
                    assert got == want, (SEED, p, fields, cap, batch, copy_here)


def test_fold_never_extends_a_full_list():
    """cap = 3: batches 0 and 1 fill the list; every later batch has differing seeds, takes nothing and leaves the records as they are, while
    the counts go on."""
    n = 60
    a, b = R.synthetic(np.random.default_rng([SEED, 7]), n, 0.0)
    a["verdict"] = b["verdict"] = A.PASS
    b["steps"][[2, 5, 11, 12, 25, 38, 39, 59]] ^= np.uint32(1)
    got, takes = fold(a, b, (1 << 64) - n, R.ALL, 3, 10)
    assert takes == [2, 1, 0, 0, 0, 0] and got["n_differ"] == 8 and got["n_listed"] == 3
    assert got == R.diff_truth(a, b, (1 << 64) - n, R.ALL, 3)
    recs = np.frombuffer(got["records"], dtype=A.DIFF_RECORD_DTYPE)
    assert recs["seed"].tolist() == [(1 << 64) - n + i for i in (2, 5, 11)]
    assert fold(a, b, 0, R.ALL, 0, 10)[1] == [0] * 6                                       # cap = 0: counts only


# ---- argument errors ---------------------------------------------------------------------------------------------------------------
def _diff(fields=A.DIFF_ALL, cap=4, with_array=True, reserved=0):
    d = A.Diff()
    d.fields, d.reserved, d.cap = fields, reserved, cap
    d._keep = (A.DiffRecord * max(cap, 1))()
    if with_array:
        d.records = C.cast(d._keep, C.POINTER(A.DiffRecord))
    return d


def _call(d, flags=0, in_flight=0, total=100, batch=0, seed0=0, reports=(True, True), w_b=None):
    """Every form of the call with the same arguments: the default context, an explicit (null) context, a list of contexts."""
    L = runtime.lib()
    w, cfg, lim, rep_a, rep_b = workload.pingpong(4, 8), A.Config.default(), A.Limits(), A.Campaign(), A.Campaign()
    arr = (C.c_void_p * 1)(None)
    tail = (w.ref(), C.byref(cfg), C.byref(lim), (w_b or w).ref(), C.byref(cfg), C.byref(lim), seed0, total, batch, in_flight, flags,
            C.byref(rep_a) if reports[0] else None, C.byref(rep_b) if reports[1] else None, C.byref(d) if d is not None else None)
    return (L.madsim_hip_run_campaign_diff(*tail), L.madsim_hip_ctx_run_campaign_diff(None, *tail), L.madsim_hip_run_campaign_diff_multi(arr, 1, *tail))


def test_argument_errors_need_no_gpu():
    """Told before any context is looked at, so these hold with and without a device (the contexts here are null)."""
    assert _call(None) == (E_ARG,) * 3                                                     # null diff
    assert _call(_diff(), reports=(False, True)) == (E_ARG,) * 3                           # null outA
    assert _call(_diff(), reports=(True, False)) == (E_ARG,) * 3                           # null outB
    for bad in (0, 128, 127 | 128, 1 << 31):
        assert _call(_diff(fields=bad)) == (E_ARG,) * 3, bad                               # nothing compared, or a bit above ALL
    assert _call(_diff(reserved=1)) == (E_ARG,) * 3
    assert _call(_diff(cap=4, with_array=False)) == (E_ARG,) * 3                           # cap > 0 without records
    assert _call(_diff(cap=0), flags=A.CAMPAIGN_STOP_AT_DIFFS) == (E_ARG,) * 3             # STOP_AT_DIFFS with cap == 0
    assert _call(_diff(), in_flight=9) == (E_ARG,) * 3
    # the mirror raises for the same things
    w = workload.pingpong(4, 8)
    for kw in (dict(fields=0), dict(fields=128), dict(max_listed=-1), dict(max_listed=0, stop_at_diffs=True), dict(in_flight=9)):
        with pytest.raises(runtime.MadsimHipError):
            runtime.run_campaign_diff_multi([], w, 0, 100, **kw)


def test_a_valid_call_without_a_context_fails_loudly():
    """Null contexts: never a report of nothing that looks like "no seed differs"."""
    for kw in (dict(d=_diff()), dict(d=_diff(A.DIFF_VERDICT, 0)), dict(d=_diff(), flags=A.CAMPAIGN_STOP_AT_DIFFS),
               dict(d=_diff(), flags=A.CAMPAIGN_STOP_AT_FAILURE | A.CAMPAIGN_STOP_AT_CAP), dict(d=_diff(), w_b=workload.pingpong(2, 4))):
        rcs = _call(**kw)
        assert rcs[1] == E_NOINIT and rcs[2] == E_NOINIT
        assert rcs[0] in (E_NOINIT, E_HIP) or not _no_gpu()
    if _no_gpu():
        w = workload.pingpong(4, 8)
        for kw in (dict(), dict(other=workload.pingpong(4, 9), fields=A.DIFF_VERDICT, max_listed=8), dict(other_config=A.Config.default(packet_loss_rate=0.01))):
            with pytest.raises(runtime.MadsimHipError, match="HIP|context|initiali"):
                runtime.run_campaign_diff(w, 0, 1000, **kw)


# ---- the end-to-end range, on the CPU ------------------------------------------------------------------------------------------------
def test_the_two_config_range_has_its_deadlocks():
    """What tests/test_campaign_diff_gpu.py relies on: loss 0 passes everywhere, loss 0.002 deadlocks 1 149 of the 10 000 seeds, and a
    deadlocked seed differs from its lossless run in every field but obs_hash (nothing is traced)."""
    _, _, _, a, b = R.two_configs()
    assert R.DEADLOCKS == 1149 and (a["verdict"] == A.PASS).all() and int((b["verdict"] == A.DEADLOCK).sum()) == R.DEADLOCKS
    t = R.diff_truth(a, b, R.SEED0, R.ALL, 4)
    assert t["transitions"][A.PASS][A.PASS] == R.TOTAL - R.DEADLOCKS and t["transitions"][A.PASS][A.DEADLOCK] == R.DEADLOCKS
    assert t["n_differ"] >= R.DEADLOCKS and t["n_by_field"][0] == R.DEADLOCKS and t["n_by_field"][6:] == [0, 0] and t["n_incomparable"] == 0
