"""Sweep campaigns (madsim_hip_run_sweep_campaign and its _ctx_ / _multi forms) without a GPU: the three structs, the prototypes and the
constants against the header, the ctypes mirror and the Rust sys file; the host-side truth (tests/sweep_ref.py) against plain Python ints;
the library's host fold (madsim_k_fold_sweep, csrc/madsim_hip.cpp: no device involved) against that truth; the argument errors, the empty
range and the empty list, none of which needs a device; CampaignSweep's helpers against brute force.  What the GPU answers is
tests/test_sweep_kernels.py's and tests/test_campaign_sweep_gpu.py's business."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from madsim_amd import _abi as A
from madsim_amd import runtime, workload
from tests import cheader as H
from tests import sweep_ref as R

E_ARG, E_HIP, E_NOINIT = -1, -2, -3
U64_MAX = (1 << 64) - 1
SEED = 20261019


def _no_gpu():
    import torch
    return not torch.cuda.is_available()


# ---- the ABI -------------------------------------------------------------------------------------------------------------------
def test_structs_and_constants_match_the_header():
    S = H.structs()
    assert S["madsim_sweep_variant_t"] == [("w", "madsim_workload_t", 0, True), ("cfg", "madsim_config_t", 0, True), ("lim", "madsim_limits_t", 0, True),
                                           ("out", "madsim_campaign_t", 0, True)]
    assert S["madsim_sweep_record_t"] == [("seed", "uint64_t", 0, False), ("fail_mask", "uint32_t", 0, False), ("differ_mask", "uint32_t", 0, False),
                                          ("verdict", "uint8_t", 8, False)]
    assert S["madsim_sweep_t"] == [("fields", "uint32_t", 0, False), ("list_rule", "uint32_t", 0, False), ("records", "madsim_sweep_record_t", 0, True),
                                   ("cap", "uint64_t", 0, False), ("n_listed", "uint64_t", 0, False), ("n_selected", "uint64_t", 0, False),
                                   ("n_settled", "uint64_t", 0, False), ("n_incomparable", "uint64_t", 0, False), ("n_runner_by_variant", "uint64_t", 8, False),
                                   ("n_differ_from_first", "uint64_t", 8, False), ("n_by_mask", "uint64_t", 256, False)]
    for name, cls, want_size in (("madsim_sweep_variant_t", A.SweepVariant, 32), ("madsim_sweep_record_t", A.SweepRecord, 24), ("madsim_sweep_t", A.Sweep, 2232)):
        offs, size = H.layout(S[name])
        assert size == want_size == C.sizeof(cls), (name, size, C.sizeof(cls))
        assert A.HEADER_STRUCTS[name] is cls
        assert [f[0] for f in cls._fields_] == [f[0] for f in S[name]], name
        for fname, _, _, _ in S[name]:
            assert getattr(cls, fname).offset == offs[fname], (name, fname)
    assert (A.Sweep.records.offset, A.Sweep.n_runner_by_variant.offset, A.Sweep.n_differ_from_first.offset, A.Sweep.n_by_mask.offset) == (8, 56, 120, 184)
    dt = np.dtype(A.SWEEP_RECORD_DTYPE)
    assert dt.itemsize == 24 and dt.names == ("seed", "fail_mask", "differ_mask", "verdict")
    assert [dt.fields[n][1] for n in dt.names] == [0, 8, 12, 16] and dt.fields["verdict"][0].shape == (8,)
    D = {k: int(v.rstrip("u")) for k, v in H.defines().items() if k.startswith(("MADSIM_SWEEP_", "MADSIM_CAMPAIGN_", "MADSIM_DIFF_")) or k == "MADSIM_HIP_ABI_VERSION"}
    assert D["MADSIM_SWEEP_MAX_VARIANTS"] == A.SWEEP_MAX_VARIANTS == 8
    assert [D["MADSIM_SWEEP_LIST_" + k] for k in ("MIXED", "FAILING", "DIFFERING")] == [0, 1, 2] \
        == [A.SWEEP_LIST_MIXED, A.SWEEP_LIST_FAILING, A.SWEEP_LIST_DIFFERING] == [R.MIXED, R.FAILING, R.DIFFERING]
    assert A.SWEEP_LIST_NAMES == ("mixed", "failing", "differing")
    assert D["MADSIM_CAMPAIGN_STOP_AT_SWEEP"] == A.CAMPAIGN_STOP_AT_SWEEP == 64
    flags = [D["MADSIM_CAMPAIGN_" + k] for k in ("STOP_AT_FAILURE", "LIST_RUNNER", "STOP_AT_CAP", "STOP_AT_GROUPS", "STOP_AT_DIFFS", "RESOLVE", "STOP_AT_SWEEP")]
    assert flags == [1, 2, 4, 8, 16, 32, 64] and not D["MADSIM_CAMPAIGN_RESOLVE_ROUNDS_MASK"] & 127
    assert D["MADSIM_DIFF_ALL"] == R.ALL and D["MADSIM_HIP_ABI_VERSION"] == A.ABI_VERSION == 7      # additive: the version stays
    assert R.RUNNER == A.OVERFLOW and R.FIELDS == A.DIFF_FIELD_NAMES


def test_library_exports_the_entry_points():
    L = runtime.lib()
    fns = H.functions()
    tail = ["const madsim_sweep_variant_t*", "uint32_t", "uint64_t", "uint64_t", "const uint64_t*", "uint64_t", "uint32_t", "uint32_t", "madsim_sweep_t*"]
    assert fns["madsim_hip_run_sweep_campaign"] == ("int", tail)
    assert fns["madsim_hip_ctx_run_sweep_campaign"] == ("int", ["madsim_hip_ctx_t*"] + tail)
    assert fns["madsim_hip_run_sweep_campaign_multi"] == ("int", ["madsim_hip_ctx_t* const*", "int"] + tail)
    for name in ("madsim_hip_run_sweep_campaign", "madsim_hip_ctx_run_sweep_campaign", "madsim_hip_run_sweep_campaign_multi", "madsim_k_launch_sweep",
                 "madsim_k_launch_sweep_list", "madsim_k_fold_sweep"):
        assert hasattr(L, name), name
    want = [C.POINTER(A.SweepVariant), C.c_uint32, C.c_uint64, C.c_uint64, C.POINTER(C.c_uint64), C.c_uint64, C.c_uint32, C.c_uint32, C.POINTER(A.Sweep)]
    assert L.madsim_hip_run_sweep_campaign.argtypes == want
    assert L.madsim_hip_ctx_run_sweep_campaign.argtypes == [C.c_void_p] + want
    assert L.madsim_hip_run_sweep_campaign_multi.argtypes == [C.POINTER(C.c_void_p), C.c_int] + want
    k_h = open(os.path.join(H.ROOT, "madsim_amd", "csrc", "sim_kernel.h")).read()
    assert re.search(r"^#define MADSIM_K_SWEEP_WORDS (\d+)u", k_h, re.M).group(1) == str(R.WORDS) == str(2 + 8 + 8 + 256)


def test_the_rust_sys_file_and_the_mirrors_declare_them():
    sys_rs = open(os.path.join(H.ROOT, "bindings", "rust", "madsim-hip-sys", "src", "lib.rs")).read()
    m = re.search(r"pub struct madsim_sweep_record_t \{(.*?)\n\}", sys_rs, flags=re.S)
    assert re.findall(r"pub (\w+): ([^,\n]+),", m.group(1)) == [("seed", "u64"), ("fail_mask", "u32"), ("differ_mask", "u32"), ("verdict", "[u8; 8]")]
    m = re.search(r"pub struct madsim_sweep_t \{(.*?)\n\}", sys_rs, flags=re.S)
    assert re.findall(r"pub (\w+): ([^,\n]+),", m.group(1)) == [
        ("fields", "u32"), ("list_rule", "u32"), ("records", "*const madsim_sweep_record_t"), ("cap", "u64"), ("n_listed", "u64"), ("n_selected", "u64"),
        ("n_settled", "u64"), ("n_incomparable", "u64"), ("n_runner_by_variant", "[u64; 8]"), ("n_differ_from_first", "[u64; 8]"), ("n_by_mask", "[u64; 256]")]
    m = re.search(r"pub struct madsim_sweep_variant_t \{(.*?)\n\}", sys_rs, flags=re.S)
    assert [n for n, _ in re.findall(r"pub (\w+): ([^,\n]+),", m.group(1))] == ["w", "cfg", "lim", "out"]
    for name, val in (("MADSIM_CAMPAIGN_STOP_AT_SWEEP", 64), ("MADSIM_SWEEP_MAX_VARIANTS", 8), ("MADSIM_SWEEP_LIST_MIXED", 0), ("MADSIM_SWEEP_LIST_FAILING", 1),
                      ("MADSIM_SWEEP_LIST_DIFFERING", 2)):
        assert f"pub const {name}: u32 = {val};" in sys_rs, name
    for fn, head in (("madsim_hip_run_sweep_campaign", ""), ("madsim_hip_ctx_run_sweep_campaign", r"ctx: \*mut madsim_hip_ctx_t, "),
                     ("madsim_hip_run_sweep_campaign_multi", r"ctxs: \*const \*mut madsim_hip_ctx_t, n_ctx: c_int, ")):
        assert re.search(r"pub fn %s\(%svariants: \*const madsim_sweep_variant_t, n_variants: u32, seed0: u64, total: u64, seeds: \*const u64, batch: u64, "
                         r"in_flight: u32, flags: u32, sweep: \*mut madsim_sweep_t\) -> c_int;" % (fn, head), sys_rs), fn
    high = open(os.path.join(H.ROOT, "bindings", "rust", "madsim-hip", "src", "builder.rs")).read()
    assert "pub fn sweep_campaign(" in high and "madsim_hip_ctx_run_sweep_campaign" in high
    hpp = open(os.path.join(H.ROOT, "include", "madsim_hip.hpp")).read()
    assert re.search(r"Sweep sweep\(const std::vector<std::pair<const Builder\*, const Workload\*>>& variants,\s*uint32_t fields", hpp)


def test_the_mirror_has_the_three_forms():
    want = ["variants", "seed0", "total", "seeds", "fields", "list_rule", "max_listed", "stop_at_listed", "batch", "in_flight", "resolve"]
    assert list(inspect.signature(runtime.run_campaign_sweep).parameters) == want
    assert list(inspect.signature(runtime.run_campaign_sweep_multi).parameters) == ["contexts"] + want
    assert list(inspect.signature(runtime.Context.run_campaign_sweep).parameters) == ["self"] + want
    for fn in (runtime.run_campaign_sweep, runtime.run_campaign_sweep_multi, runtime.Context.run_campaign_sweep):
        p = inspect.signature(fn).parameters
        assert [p[k].default for k in want[1:]] == [0, 0, None, A.DIFF_VERDICT, "mixed", 0, False, 0, 0, None]


# ---- the truth against plain Python ints -----------------------------------------------------------------------------------------
def plain_masks(results, fields):
    """[(fail, runner, differ)] per seed with Python ints, one seed and one variant at a time."""
    out = []
    for i in range(len(results[0])):
        fail = runner = differ = 0
        for v, r in enumerate(results):
            x = int(r["verdict"][i])
            fail |= (1 <= x <= 3) << v
            runner |= (x >= 4) << v
            if v and any(fields >> k & 1 and int(r[name][i]) != int(results[0][name][i]) for k, name in enumerate(R.FIELDS)):
                differ |= 1 << v
        out.append((fail, runner, 0 if runner else differ))
    return out


def plain_truth(results, seeds, fields, rule, cap):
    """sweep_truth restated with Python ints; `seeds`: the seed of every position."""
    V = len(results)
    t = {"n_listed": 0, "n_selected": 0, "n_settled": 0, "n_incomparable": 0, "n_runner_by_variant": [0] * 8, "n_differ_from_first": [0] * 8,
         "n_by_mask": [0] * 256}
    recs = []
    for i, (fail, runner, differ) in enumerate(plain_masks(results, fields)):
        if runner:
            t["n_incomparable"] += 1
            for v in range(V):
                t["n_runner_by_variant"][v] += runner >> v & 1
            continue
        t["n_settled"] += 1
        t["n_by_mask"][fail] += 1
        for v in range(V):
            t["n_differ_from_first"][v] += differ >> v & 1
        if (fail not in (0, (1 << V) - 1)) if rule == R.MIXED else fail != 0 if rule == R.FAILING else differ != 0:
            t["n_selected"] += 1
            if len(recs) < cap:
                verdicts = bytes(int(r["verdict"][i]) for r in results) + bytes(8 - V)
                recs.append(int(seeds[i]).to_bytes(8, "little") + fail.to_bytes(4, "little") + differ.to_bytes(4, "little") + verdicts)
    t["n_listed"] = len(recs)
    t["records"] = b"".join(recs)
    return t


@pytest.mark.parametrize("n", [1, 7, 64, 300])
def test_the_truth_is_the_plain_restatement(n):
    for case, (V, p) in enumerate(((2, 0.0), (3, 0.05), (5, 0.5), (8, 1.0))):
        res = R.synthetic(np.random.default_rng([SEED, n, case]), n, V, p)
        gaps = np.cumsum(np.random.default_rng([SEED, n]).integers(1, 1000, n)).astype(np.uint64)
        for fields in (0, 1, 2, 4, 8, 16, 32, 64, R.ALL, R.ALL & ~32):
            for rule in (R.MIXED, R.FAILING, R.DIFFERING):
                if rule == R.DIFFERING and not fields:
                    continue
                for src, seeds in ((0, range(n)), ((1 << 40) + 7, [(1 << 40) + 7 + i for i in range(n)]),
                                   ((1 << 64) - n, [(1 << 64) - n + i for i in range(n)]), (gaps, gaps)):
                    for cap in (0, 1, n, n + 3):
                        want = plain_truth(res, seeds, fields, rule, cap)
                        got = R.sweep_truth(res, src, fields, rule, cap)
                        assert got == want, (SEED, n, case, fields, rule, cap)
                        assert got["n_settled"] + got["n_incomparable"] == n and sum(got["n_by_mask"]) == got["n_settled"]
                        assert not any(got["n_by_mask"][1 << V:]) and got["n_differ_from_first"][0] == 0
        w = R.words_of(res, R.ALL, R.MIXED)
        assert int(w[0]) == R.sweep_truth(res, 0, R.ALL, R.MIXED, 0)["n_selected"] == sum(R.wave_counts(res, R.ALL, R.MIXED)[1])


# ---- the host fold ---------------------------------------------------------------------------------------------------------------
def _fold_lib():
    L = runtime.lib()
    L.madsim_k_fold_sweep.restype, L.madsim_k_fold_sweep.argtypes = C.c_uint64, [C.POINTER(A.Sweep), C.c_void_p, C.c_uint64, C.c_void_p]
    return L


def fold(res, seeds, fields, rule, cap, edges, copy_here=False):
    """madsim_k_fold_sweep over the device-format words (and records) of `res` cut at `edges`, from the state run_variants_impl starts
    with; (answer, the `take` of every batch).  copy_here: the fold is given no records and the caller copies them, as the library does
    from device memory."""
    L = _fold_lib()
    arr = np.full(cap + 1, 0xA5, dtype=np.uint8).repeat(24).view(A.SWEEP_RECORD_DTYPE)              # one record of guard behind the caller's array
    s = A.Sweep()
    s.fields, s.list_rule, s.cap = fields, rule, cap
    s.records = arr.ctypes.data_as(C.POINTER(A.SweepRecord)) if cap else None
    takes = []
    for lo, hi in zip(edges[:-1], edges[1:]):
        part = [r[lo:hi] for r in res]
        words = np.ascontiguousarray(R.words_of(part, fields, rule))
        every = np.frombuffer(R.sweep_truth(part, seeds[lo:hi], fields, rule, hi - lo)["records"], dtype=A.SWEEP_RECORD_DTYPE)
        recs = np.ascontiguousarray(every[:min(cap, hi - lo)])                                      # what sweep_write_kernel leaves: at most the flight's room
        at = int(s.n_listed)
        take = int(L.madsim_k_fold_sweep(C.byref(s), words.ctypes.data, hi - lo, None if copy_here or not len(recs) else recs.ctypes.data))
        assert take == int(s.n_listed) - at and take <= len(recs)
        if copy_here and take:
            arr[at:at + take] = recs[:take]
        takes.append(take)
    assert arr[cap:].tobytes() == b"\xa5" * 24, "the fold wrote behind the caller's array"
    return R.of_struct(s, arr), takes


@pytest.mark.parametrize("V,p", [(2, 0.0), (4, 0.03), (8, 0.6)])
def test_fold_gives_the_truth_whatever_the_cut(V, p):
    n = 1000
    res = R.synthetic(np.random.default_rng([SEED, V]), n, V, p)
    seeds = np.arange(77, 77 + n, dtype=np.uint64)
    for fields, rule in ((R.ALL, R.DIFFERING), (1, R.MIXED), (0, R.FAILING), (R.ALL & ~32, R.MIXED)):
        n_sel = R.sweep_truth(res, seeds, fields, rule, 0)["n_selected"]
        in_first = R.sweep_truth([r[:130] for r in res], seeds[:130], fields, rule, 0)["n_selected"]
        for cap in sorted({0, 1, n_sel, max(n_sel - 1, 0), n_sel + 3, in_first + 1}):              # in_first + 1: the cap cut falls just across a batch edge
            want = R.sweep_truth(res, seeds, fields, rule, cap)
            for edges in ([0, 130, 131, n], [0, n], [0, 7, 500, n]):                                # three uneven batches, one, three again
                for copy_here in (False, True):
                    got, takes = fold(res, seeds, fields, rule, cap, edges, copy_here)
                    assert got == want, (SEED, V, fields, rule, cap, edges, copy_here)
                    assert sum(takes) == want["n_listed"]


def test_fold_never_extends_a_full_list():
    n = 60
    res = R.synthetic(np.random.default_rng([SEED, 7]), n, 3, 0.0)
    for r in res:
        r["verdict"] = A.PASS
    res[2]["verdict"][[2, 5, 11, 12, 25, 38, 39, 59]] = A.DEADLOCK
    seeds = np.arange((1 << 64) - n, 1 << 64, dtype=np.uint64)
    got, takes = fold(res, seeds, 1, R.MIXED, 3, list(range(0, n + 1, 10)))
    assert takes == [2, 1, 0, 0, 0, 0] and got["n_selected"] == 8 and got["n_listed"] == 3 and got["n_by_mask"][4] == 8
    assert got == R.sweep_truth(res, seeds, 1, R.MIXED, 3)
    assert np.frombuffer(got["records"], dtype=A.SWEEP_RECORD_DTYPE)["seed"].tolist() == [(1 << 64) - n + i for i in (2, 5, 11)]
    assert fold(res, seeds, 1, R.MIXED, 0, list(range(0, n + 1, 10)))[1] == [0] * 6              # cap = 0: counts only


# ---- argument errors ---------------------------------------------------------------------------------------------------------------
def _sweep(fields=A.DIFF_VERDICT, rule=0, cap=4, with_array=True):
    s = A.Sweep()
    s.fields, s.list_rule, s.cap = fields, rule, cap
    s._keep = (A.SweepRecord * max(cap, 1))()
    if with_array:
        s.records = C.cast(s._keep, C.POINTER(A.SweepRecord))
    return s


def _variants(n=2, null_w=None, null_out=None, workloads=None):
    arr = (A.SweepVariant * max(n, 1))()
    keep = []
    for v in range(n):
        w, cfg, lim, rep = (workloads[v] if workloads else workload.pingpong(4, 8)), A.Config.default(), A.Limits(), A.Campaign()
        keep.append((w, cfg, lim, rep))
        if v != null_w:
            arr[v].w = C.pointer(w.struct)
        arr[v].cfg, arr[v].lim = C.pointer(cfg), C.pointer(lim)
        if v != null_out:
            arr[v].out = C.pointer(rep)
    arr._keep = keep
    return arr


def _call(s, variants=None, n=2, flags=0, in_flight=0, total=100, batch=0, seed0=0, seeds=None):
    """Every form of the call with the same arguments: the default context, an explicit (null) context, a list of contexts."""
    L = runtime.lib()
    variants = variants if variants is not None else _variants(n)
    ctxs = (C.c_void_p * 1)(None)
    sp = seeds.ctypes.data_as(C.POINTER(C.c_uint64)) if seeds is not None else None
    tail = (variants if variants is not False else None, n, seed0, total, sp, batch, in_flight, flags, C.byref(s) if s is not None else None)
    return (L.madsim_hip_run_sweep_campaign(*tail), L.madsim_hip_ctx_run_sweep_campaign(None, *tail), L.madsim_hip_run_sweep_campaign_multi(ctxs, 1, *tail))


def _last_error():
    return runtime.lib().madsim_hip_last_error().decode()


def test_argument_errors_need_no_gpu():
    """Told before any context is looked at, so these hold with and without a device (the contexts here are null)."""
    for n in (0, 1, 9, 1 << 31):
        assert _call(_sweep(), _variants(min(n, 9)), n=n) == (E_ARG,) * 3, n                   # n_variants outside 2 .. 8
    assert _call(_sweep(), False) == (E_ARG,) * 3                                          # null variants
    assert _call(None) == (E_ARG,) * 3                                                     # null sweep
    for v in (0, 2):
        assert _call(_sweep(), _variants(3, null_w=v), n=3) == (E_ARG,) * 3
        assert _call(_sweep(), _variants(3, null_out=v), n=3) == (E_ARG,) * 3
    for bad in (128, 127 | 128, 1 << 31):
        assert _call(_sweep(fields=bad)) == (E_ARG,) * 3, bad                              # a bit above ALL
    assert _call(_sweep(rule=3)) == (E_ARG,) * 3
    assert _call(_sweep(fields=0, rule=A.SWEEP_LIST_DIFFERING)) == (E_ARG,) * 3            # nothing compared, yet listing what differs
    assert _call(_sweep(cap=4, with_array=False)) == (E_ARG,) * 3                          # cap > 0 without records
    assert _call(_sweep(cap=0), flags=A.CAMPAIGN_STOP_AT_SWEEP) == (E_ARG,) * 3            # STOP_AT_SWEEP with cap == 0
    assert _call(_sweep(), seed0=5, total=3, seeds=np.array([1, 2, 3], dtype=np.uint64)) == (E_ARG,) * 3      # a list with seed0 != 0
    assert _call(_sweep(), total=4, seeds=np.array([1, 2, 2, 9], dtype=np.uint64)) == (E_ARG,) * 3            # a list that does not ascend
    assert "seeds[1] = 2 is not below seeds[2] = 2" in _last_error()
    assert _call(_sweep(), seed0=U64_MAX, total=2) == (E_ARG,) * 3                         # seed0 + total wraps
    assert _call(_sweep(), in_flight=9) == (E_ARG,) * 3
    assert _call(_sweep(), flags=A.CAMPAIGN_RESOLVE | 9 << A.CAMPAIGN_RESOLVE_ROUNDS_SHIFT) == (E_ARG,) * 3
    # a validate() error of a variant, with the variant named
    bad = workload.pingpong(4, 8)
    bad.struct.n_progs = 0
    rcs = _call(_sweep(), _variants(4, workloads=[workload.pingpong(4, 8)] * 3 + [bad]), n=4)
    assert all(rc < 0 and rc != E_NOINIT for rc in rcs), rcs
    assert _last_error().startswith("variant 3: "), _last_error()
    # the mirror raises for the same things
    w = workload.pingpong(4, 8)
    for kw in (dict(fields=128), dict(list_rule="none"), dict(list_rule="differing", fields=0), dict(max_listed=-1), dict(stop_at_listed=True),
               dict(in_flight=9), dict(seeds=[3, 2, 1])):
        with pytest.raises(runtime.MadsimHipError):
            runtime.run_campaign_sweep_multi([], [(w,), (w,)], total=0 if "seeds" in kw else 100, **kw)
    for variants in ([(w,)], [(w,)] * 9, [(None,), (w,)]):
        with pytest.raises(runtime.MadsimHipError):
            runtime.run_campaign_sweep(variants, total=100)


def test_an_empty_range_and_an_empty_list_need_no_device():
    """total == 0, with the range and with the list: 0, and every report as a campaign that ran nothing leaves it."""
    L = runtime.lib()
    for seeds in (None, np.zeros(1, dtype=np.uint64)):
        for form in (0, 1):
            s, variants = _sweep(fields=R.ALL, rule=2), _variants(3)
            s.n_listed = s.n_selected = s.n_settled = s.n_incomparable = 99
            for k in range(256):
                s.n_by_mask[k] = 7
            for _, _, _, rep in variants._keep:
                rep.seeds_run = rep.n_failed = 5
            sp = seeds.ctypes.data_as(C.POINTER(C.c_uint64)) if seeds is not None else None
            tail = (variants, 3, 0, 0, sp, 0, 0, 0, C.byref(s))
            assert (L.madsim_hip_ctx_run_sweep_campaign(None, *tail) if form else L.madsim_hip_run_sweep_campaign(*tail)) == 0 or not _no_gpu()
            assert R.of_struct(s, np.zeros(0, dtype=A.SWEEP_RECORD_DTYPE)) == R.sweep_truth([np.zeros(0, dtype=A.RESULT_DTYPE)] * 3, 0, R.ALL, 2, 0)
            for _, _, _, rep in variants._keep:
                assert (rep.seeds_run, rep.batches_run, rep.n_failed, rep.n_runner, rep.first_failing_seed) == (0, 0, 0, 0, U64_MAX)
    if _no_gpu():
        w = workload.pingpong(4, 8)
        for kw in (dict(total=0), dict(seeds=[])):
            reps, sw = runtime.run_campaign_sweep([(w,), (w, A.Config.default(packet_loss_rate=0.01))], max_listed=4, **kw)
            assert len(reps) == 2 and len(sw) == 0 and sw.n_settled == 0 and sw.n_by_mask.tolist() == [0] * 4


def test_a_valid_call_without_a_context_fails_loudly():
    """Null contexts: never a report of nothing that looks like "every seed passes everywhere"."""
    for kw in (dict(s=_sweep()), dict(s=_sweep(0, 1, 0)), dict(s=_sweep(), flags=A.CAMPAIGN_STOP_AT_SWEEP), dict(s=_sweep(), n=8),
               dict(s=_sweep(), flags=A.CAMPAIGN_STOP_AT_FAILURE | A.CAMPAIGN_STOP_AT_DIFFS),
               dict(s=_sweep(), total=3, seeds=np.array([1, 5, 9], dtype=np.uint64))):
        rcs = _call(**kw)
        assert rcs[1] == E_NOINIT and rcs[2] == E_NOINIT
        assert rcs[0] in (E_NOINIT, E_HIP) or not _no_gpu()
    if _no_gpu():
        w = workload.pingpong(4, 8)
        with pytest.raises(runtime.MadsimHipError, match="HIP|context|initiali"):
            runtime.run_campaign_sweep([(w,), (w, A.Config.default(packet_loss_rate=0.01))], 0, 1000)


# ---- CampaignSweep's helpers -------------------------------------------------------------------------------------------------------
def _report(masks, V):
    s = A.Sweep()
    for m in masks:
        s.n_by_mask[m] += 1
    s.n_settled = len(masks)
    return runtime.CampaignSweep(s, np.zeros(0, dtype=A.SWEEP_RECORD_DTYPE), V)


@pytest.mark.parametrize("V", [2, 3, 5, 8])
def test_the_helpers_against_brute_force(V):
    rng = np.random.default_rng([SEED, 11, V])
    suffixes = [((1 << V) - 1) & ~((1 << k) - 1) for k in range(V)]
    for case in range(6):
        masks = [int(m) for m in (rng.integers(0, 1 << V, 400) if case < 3 else rng.choice([0, 0] + suffixes[case - 3:], 400))]
        rep = _report(masks, V)
        assert len(rep.n_by_mask) == 1 << V and int(rep.n_by_mask.sum()) == len(masks)
        for v in range(V):
            assert rep.fails(v) == sum(m >> v & 1 for m in masks)
            assert rep.only(v) == sum(m == 1 << v for m in masks)
            for j in range(V):
                assert rep.fails_not(v, j) == sum(bool(m >> v & 1 and not m >> j & 1) for m in masks)
        is_suffix = lambda m: all(m >> k & 1 for k in range(min(k for k in range(V) if m >> k & 1), V))
        assert rep.nested() == all(is_suffix(m) for m in masks if m)
        assert rep.nested() == (case >= 3)
        assert rep.first_failing().tolist() == [sum(m != 0 and min(k for k in range(V) if m >> k & 1) == v for m in masks) for v in range(V)]
    assert _report([0] * 5, V).nested() and _report([], V).nested() and not _report([1], V).nested()


# ---- the end-to-end range, on the CPU ------------------------------------------------------------------------------------------------
def test_the_four_loss_rates_nest():
    """What tests/test_campaign_sweep_gpu.py relies on: the failures per loss rate, all deadlocks, no runner verdict, and failing sets that
    grow with the loss rate."""
    _, cfgs, res = R.four_configs()
    assert [c.packet_loss_rate for c in cfgs] == list(R.LOSSES)
    assert [int((r["verdict"] != A.PASS).sum()) for r in res] == list(R.FAILURES) == [int((r["verdict"] == A.DEADLOCK).sum()) for r in res]
    t = R.sweep_truth(res, R.SEED0, R.ALL, R.MIXED, 4)
    assert {m: c for m, c in enumerate(t["n_by_mask"]) if c} == R.MASKS and t["n_incomparable"] == 0 and t["n_settled"] == R.TOTAL
    assert t["n_differ_from_first"] == list(R.FAILURES) + [0] * 4 and t["n_selected"] == R.TOTAL - R.MASKS[0]
    mixed = R.selected(*R.classify(res, 1), R.MIXED, 4)
    per_thousand = [int(mixed[k:k + 1000].sum()) for k in range(0, R.TOTAL, 1000)]
    assert min(per_thousand) == 431 and max(per_thousand) == 482 and per_thousand[:2] == [469, 470]
