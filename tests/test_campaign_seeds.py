"""List campaigns (madsim_hip_run_seeds_campaign, madsim_hip_run_seeds_campaign_diff) without a GPU: the list truth of tests/seedlist_ref.py —
the range truths at seed0 = 0 with every seed-valued field s replaced by seeds[s] — against plain Python ints; the six prototypes in the
header, the ctypes mirror and the Rust sys file, the exports (the six _list launchers among them) and the ABI version; and the argument
errors, which are told before any context is looked at.  What a list campaign reports is tests/test_campaign_seeds_gpu.py's business, the
list kernels are tests/test_seedlist_kernels.py's."""
import ctypes as C
import inspect
import os
import re
import struct

import numpy as np
import pytest

from madsim_amd import _abi as A
from madsim_amd import runtime, workload
from tests import cheader as H
from tests import diff_ref as D
from tests import groups_ref as G
from tests import seedlist_ref as S
from tests import stats_ref as R

E_ARG, E_HIP, E_NOINIT = -1, -2, -3
U64 = (1 << 64) - 1
SEED = 20261019
COUNTS = (1, 63, 64, 65, 1023, 1025, 4097)


# ---- the lists and the truth ---------------------------------------------------------------------------------------------------
def test_the_three_lists_are_what_they_promise():
    for count in COUNTS + (262_209,):
        for name, make in S.LISTS:
            s = make(count)
            assert s.dtype == np.uint64 and len(s) == count and (count < 2 or (s[:-1] < s[1:]).all()), (name, count)
        assert int(S.dense(count)[0]) == (1 << 40) + 7 and int(S.dense(count)[-1]) == (1 << 40) + 7 + count - 1
        assert int(S.top(count)[-1]) == U64 and int(S.top(count)[0]) == U64 - (count - 1) and int(S.top(count)[0]) >> 63 == 1
    g = [int(x) for x in S.gapped(9)]
    assert g == [0, 1, 3, 6, 6 + (1 << 33), 7 + (1 << 33), 9 + (1 << 33), 12 + (1 << 33), 12 + (2 << 33)]
    assert all(int(s) - i >= 1 << 33 for i, s in enumerate(S.gapped(65)) if i >= 4)          # position and seed differ above bit 32


def synthetic(rng, n):
    """Every verdict value (runner verdicts, 7, 2^32 - 1), key fields from a small pool (so groups have members), the metrics with ties."""
    r = np.zeros(n, dtype=A.RESULT_DTYPE)
    r["verdict"] = rng.choice(np.array([0, 0, 0, 1, 2, 3, 4, 5, 6, 7, 0xffffffff], dtype=np.uint32), n)
    r["steps"] = rng.integers(0, 4, n)
    for name in ("clock_ns", "msg_count", "rng_calls"):
        r[name] = rng.choice(np.array([0, 5, 1 << 40, U64], dtype=np.uint64), n)
    r["trace_hash"], r["obs_hash"] = rng.integers(0, 1 << 64, n, dtype=np.uint64), rng.choice(np.array([0, U64, 77], dtype=np.uint64), n)
    return r


def py_rows(results, seeds):
    return [(int(s),) + tuple(int(x) for x in r) for s, r in zip(seeds, results.tolist())]      # (seed, verdict, steps, clock, msgs, rng, trace, obs)


@pytest.mark.parametrize("count", (1, 63, 65, 1025))
def test_the_list_truth_is_plain_pythons(count):
    """Every seed-valued field of every list truth against a restatement in Python ints over (seed, result) rows."""
    for j, (name, make) in enumerate(S.LISTS):
        rng = np.random.default_rng([SEED, count, j])
        res, seeds = synthetic(rng, count), make(count)
        rows = py_rows(res, seeds)
        what = (SEED, count, name)
        failing = [r for r in rows if r[1] != A.PASS]
        genuine = [r for r in failing if r[1] < A.OVERFLOW]
        six = [min([r[0] for r in failing] + [U64]), len(failing), sum(r[2] for r in rows) % (1 << 64), sum(r[3] for r in rows) % (1 << 64),
               min([r[0] for r in genuine] + [U64]), len(failing) - len(genuine)]
        assert S.summary6_truth(res, seeds) == six, what
        assert S.campaign_truth(res, seeds) == {"seeds_run": count, "first_failing_seed": six[4], "n_failed": len(genuine), "n_runner": six[5],
                                                "total_steps": six[2], "total_clock_ns": six[3]}, what
        for list_runner in (0, 1):
            listed = failing if list_runner else genuine
            for cap in sorted({0, 1, len(listed), count}):
                words, recs = S.collect_truth(res, seeds, cap, list_runner)
                by = [sum(1 for r in rows if min(r[1], 7) == v) for v in range(8)]
                assert [int(x) for x in words] == six + by + [len(listed)], (what, list_runner, cap)
                assert recs == b"".join(struct.pack("<QIIQQQQQ", *r) for r in listed[:cap]), (what, list_runner, cap)
        for include, top_k in ((0b1111, 16), (0b0001, 2), (0b0100, 1)):
            t = S.stats_truth(res, seeds, include, top_k)
            counted = [r for r in rows if r[1] < 4 and include >> r[1] & 1]
            for m, col in zip(R.METRICS, (3, 2, 4, 5)):
                assert t[m]["top"] == [(r[col], r[0]) for r in sorted(counted, key=lambda r: (-r[col], r[0]))[:top_k]], (what, include, top_k, m)
            assert t["n"] == len(counted)
        for include, key_field in ((0b1110, A.GROUP_KEY_OBS), (0b1111, A.GROUP_KEY_STEPS)):
            col = 7 if key_field == A.GROUP_KEY_OBS else 2
            modes = {}
            for r in rows:
                if r[1] < 4 and include >> r[1] & 1:
                    m = modes.setdefault((r[1], r[col]), [0, r[0]])
                    m[0] += 1
            want = sorted(((v, k, c, f) for (v, k), (c, f) in modes.items()), key=lambda g: g[3])
            assert S.all_groups(res, seeds, include, key_field) == want, (what, include, key_field)
            t = S.groups_truth(res, seeds, include, key_field, 2)
            assert t == {"groups": want[:2], "n_grouped": sum(g[2] for g in want[:2]), "n_ungrouped": sum(g[2] for g in want[2:])}
        a, b = D.synthetic(rng, count, p_differ=0.3)
        for fields, cap in ((A.DIFF_ALL, count), (A.DIFF_VERDICT | A.DIFF_OBS, 3), (A.DIFF_ALL, 0)):
            t = S.diff_truth(a, b, seeds, fields, cap)
            differing = [i for i in range(count) if a["verdict"][i] < 4 and b["verdict"][i] < 4
                         and any(fields >> k & 1 and a[f][i] != b[f][i] for k, f in enumerate(D.FIELDS))]
            recs = np.frombuffer(t["records"], dtype=A.DIFF_RECORD_DTYPE)
            assert t["n_differ"] == len(differing) and [int(x) for x in recs["seed"]] == [int(seeds[i]) for i in differing[:cap]], (what, fields, cap)
            assert recs["a"].tobytes() == a[differing[:cap]].tobytes() and recs["b"].tobytes() == b[differing[:cap]].tobytes()
            plain = D.diff_truth(a, b, 0, fields, cap)
            assert {k: v for k, v in t.items() if k != "records"} == {k: v for k, v in plain.items() if k != "records"}
        for steps_maxed in (0, 1):
            got_seeds, got_idx = S.resolve_truth(res, seeds, steps_maxed)
            want = [(r[0], i) for i, r in enumerate(rows) if r[1] == A.OVERFLOW or (r[1] == A.STEP_LIMIT and not steps_maxed)]
            assert [(int(s), int(i)) for s, i in zip(got_seeds, got_idx)] == want, (what, steps_maxed)


def test_the_sentinel_stays_and_the_sentinel_value_can_be_a_member():
    res = np.zeros(3, dtype=A.RESULT_DTYPE)
    seeds = S.top(3)
    assert S.summary6_truth(res, seeds)[0] == S.summary6_truth(res, seeds)[4] == U64          # nothing fails: "no such seed"
    res["verdict"][2] = A.DEADLOCK
    six = S.summary6_truth(res, seeds)
    assert six[0] == six[4] == U64 and six[1] == 1                                            # seed 2^64 - 1 fails: test n_failed, not the sentinel
    assert S.campaign_truth(res, seeds)["n_failed"] == 1
    assert S.seed_at(seeds, U64) == U64 and S.seed_at(seeds, 0) == U64 - 2
    # a dense list is the range: the mapping is the range truth's own seeds
    rng = np.random.default_rng([SEED, 9])
    res, seed0 = synthetic(rng, 1025), (1 << 40) + 7
    from tests import report_ref as T
    assert S.summary6_truth(res, S.dense(1025)) == T.summary_truth(res, seed0)[1]
    assert S.collect_truth(res, S.dense(1025), 100, 1)[1] == T.collect_truth(res, seed0, 100, 1)[1]
    assert S.all_groups(res, S.dense(1025), 15, 0) == G.all_groups(res, seed0, 15, 0)
    assert R.same(S.stats_truth(res, S.dense(1025), 15, 16), R.stats_truth(res, np.uint64(seed0), 15, 16))
    a, b = D.synthetic(rng, 1025, 0.3)
    assert S.diff_truth(a, b, S.dense(1025), 127, 50) == D.diff_truth(a, b, seed0, 127, 50)


# ---- the ABI -------------------------------------------------------------------------------------------------------------------
PLAIN = ["const madsim_workload_t*", "const madsim_config_t*", "const uint64_t*", "uint64_t", "uint64_t", "uint32_t", "uint32_t", "const madsim_limits_t*",
         "madsim_campaign_t*", "madsim_collect_t*", "madsim_stats_t*", "madsim_groups_t*"]
SIDE = ["const madsim_workload_t*", "const madsim_config_t*", "const madsim_limits_t*"]
DIFF = SIDE + SIDE + ["const uint64_t*", "uint64_t", "uint64_t", "uint32_t", "uint32_t", "madsim_campaign_t*", "madsim_campaign_t*", "madsim_diff_t*"]
LAUNCHERS = ("madsim_k_launch_summary6_list", "madsim_k_launch_collect_list", "madsim_k_launch_stats_list", "madsim_k_launch_groups_list",
             "madsim_k_launch_diff_list", "madsim_k_launch_resolve_list_list")


def test_the_six_prototypes_in_the_header_the_mirror_and_the_library():
    L, fns = runtime.lib(), H.functions()
    for base, tail in (("run_seeds_campaign", PLAIN), ("run_seeds_campaign_diff", DIFF)):
        forms = {f"madsim_hip_{base}": tail, f"madsim_hip_ctx_{base}": ["madsim_hip_ctx_t*"] + tail,
                 f"madsim_hip_{base}_multi": ["madsim_hip_ctx_t* const*", "int"] + tail}
        assert all("run_campaign" not in name for name in forms)      # (tests/test_resolve.py counts the header's run_campaign functions: fifteen, the range forms)
        for name, params in forms.items():
            assert fns[name] == ("int", params), name
            assert hasattr(L, name), name
            assert len(getattr(L, name).argtypes) == len(params), name
    u64p = C.POINTER(C.c_uint64)
    assert L.madsim_hip_run_seeds_campaign.argtypes[2:5] == [u64p, C.c_uint64, C.c_uint64]
    assert L.madsim_hip_run_seeds_campaign.argtypes[8:] == [C.POINTER(A.Campaign), C.POINTER(A.Collect), C.POINTER(A.Stats), C.POINTER(A.Groups)]
    assert L.madsim_hip_run_seeds_campaign_diff.argtypes[6:9] == [u64p, C.c_uint64, C.c_uint64] and L.madsim_hip_run_seeds_campaign_diff.argtypes[-1] == C.POINTER(A.Diff)
    for name in LAUNCHERS:
        assert hasattr(L, name), name
    k_h = open(os.path.join(H.ROOT, "madsim_amd", "csrc", "sim_kernel.h")).read()
    for name in LAUNCHERS:
        assert re.search(r"\b%s\(const madsim_result_t\* \w+, (const madsim_result_t\* \w+, )?uint64_t count, const uint64_t\* d_seeds," % name, k_h), name
    assert L.madsim_hip_version() == A.ABI_VERSION == 7 == int(re.search(r"MADSIM_HIP_ABI_VERSION (\d+)u", H.header_text()).group(1))
    text = open(H.HEADER_PATH).read()
    assert "MUST ASCEND STRICTLY" in text and "so that nothing about ordering changes" in text      # the rule, and why


def test_the_rust_sys_file_declares_them():
    sys_rs = open(os.path.join(H.ROOT, "bindings", "rust", "madsim-hip-sys", "src", "lib.rs")).read()
    for fn in ("madsim_hip_run_seeds_campaign", "madsim_hip_ctx_run_seeds_campaign", "madsim_hip_run_seeds_campaign_multi"):
        assert re.search(r"pub fn %s\([^;]*seeds: \*const u64, n: u64, batch: u64, in_flight: u32, flags: u32, lim: \*const madsim_limits_t, "
                         r"out: \*mut madsim_campaign_t, col: \*mut madsim_collect_t, st: \*mut madsim_stats_t, grp: \*mut madsim_groups_t\) -> c_int;" % fn, sys_rs), fn
    for fn in ("madsim_hip_run_seeds_campaign_diff", "madsim_hip_ctx_run_seeds_campaign_diff", "madsim_hip_run_seeds_campaign_diff_multi"):
        assert re.search(r"pub fn %s\([^;]*seeds: \*const u64, n: u64, batch: u64, in_flight: u32, flags: u32, outA: \*mut madsim_campaign_t, "
                         r"outB: \*mut madsim_campaign_t, diff: \*mut madsim_diff_t\) -> c_int;" % fn, sys_rs), fn


def test_the_mirror_has_the_forms_and_keeps_the_old_parameter_lists():
    want = ["workload", "seeds", "batch", "in_flight", "stop_at_failure", "config", "limits", "collect", "list_runner", "stop_at_cap", "stats", "groups",
            "stop_at_groups", "resolve", "observe"]
    assert list(inspect.signature(runtime.run_campaign_seeds).parameters) == want
    assert list(inspect.signature(runtime.Context.run_campaign_seeds).parameters) == ["self"] + want
    assert list(inspect.signature(runtime.run_campaign_seeds_multi).parameters)[:3] == ["contexts", "workload", "seeds"]
    for fn in (runtime.run_campaign_diff_seeds, runtime.Context.run_campaign_diff_seeds, runtime.run_campaign_diff_seeds_multi):
        p = list(inspect.signature(fn).parameters)
        assert "seeds" in p and "other" in p and "resolve" in p and "seed0" not in p and "total" not in p, fn
    assert list(inspect.signature(runtime.run_campaign_diff_seeds).parameters)[:3] == ["workload", "seeds", "other"]
    assert list(inspect.signature(runtime.run_campaign_diff).parameters) == [
        "workload", "seed0", "total", "other", "config", "other_config", "limits", "other_limits", "fields", "max_listed", "stop_at_diffs", "batch", "in_flight"]
    assert list(inspect.signature(runtime.run_campaign).parameters)[:3] == ["workload", "seed0", "total"]


# ---- argument errors -----------------------------------------------------------------------------------------------------------
def _parts(collect=None, stats=None, groups=None):
    col = st = grp = None
    if collect is not None:
        col = A.Collect()
        col._keep = (A.Failure * max(collect, 1))()
        col.failures, col.cap = C.cast(col._keep, C.POINTER(A.Failure)), collect
    if stats is not None:
        st = A.Stats()
        st.include, st.top_k = stats
        st._keep = (A.Extreme * (A.STAT_METRICS * A.STAT_MAX_TOP))()
        st.top = C.cast(st._keep, C.POINTER(A.Extreme))
    if groups is not None:
        grp = A.Groups()
        grp.include, grp.key_field, grp.cap = groups
        grp._keep = (A.Group * max(grp.cap, 1))()
        grp.groups = C.cast(grp._keep, C.POINTER(A.Group))
    return col, st, grp


def _ptr(seeds):
    if seeds is None:
        return None, None
    arr = np.ascontiguousarray(seeds, dtype=np.uint64)
    return arr, arr.ctypes.data_as(C.POINTER(C.c_uint64))


def _call(seeds, n=None, batch=0, in_flight=0, flags=0, parts=(None, None, None), report=True):
    """Every form of the call with the same arguments and null contexts: ((rc, rc, rc), the three reports, the last error text)."""
    L = runtime.lib()
    w, cfg, lim = workload.pingpong(4, 8), A.Config.default(), A.Limits()
    keep, p = _ptr(seeds)
    n = (0 if keep is None else len(keep)) if n is None else n
    arr = (C.c_void_p * 1)(None)
    reps = [A.Campaign() for _ in range(3)]
    col, st, grp = parts
    tail = lambda rep: (w.ref(), C.byref(cfg), p, n, batch, in_flight, flags, C.byref(lim), C.byref(rep) if report else None,      # noqa: E731
                        C.byref(col) if col else None, C.byref(st) if st else None, C.byref(grp) if grp else None)
    rcs = (L.madsim_hip_run_seeds_campaign(*tail(reps[0])), L.madsim_hip_ctx_run_seeds_campaign(None, *tail(reps[1])),
           L.madsim_hip_run_seeds_campaign_multi(arr, 1, *tail(reps[2])))
    return rcs, reps, L.madsim_hip_last_error().decode()


def _call_diff(seeds, n=None, batch=0, in_flight=0, flags=0, d=None):
    L = runtime.lib()
    w, cfg, lim = workload.pingpong(4, 8), A.Config.default(), A.Limits()
    keep, p = _ptr(seeds)
    n = (0 if keep is None else len(keep)) if n is None else n
    arr = (C.c_void_p * 1)(None)
    if d is None:
        d = A.Diff()
        d.fields = A.DIFF_ALL
    reps = [(A.Campaign(), A.Campaign()) for _ in range(3)]
    tail = lambda r: (w.ref(), C.byref(cfg), C.byref(lim), w.ref(), C.byref(cfg), C.byref(lim), p, n, batch, in_flight, flags, C.byref(r[0]),      # noqa: E731
                      C.byref(r[1]), C.byref(d))
    rcs = (L.madsim_hip_run_seeds_campaign_diff(*tail(reps[0])), L.madsim_hip_ctx_run_seeds_campaign_diff(None, *tail(reps[1])),
           L.madsim_hip_run_seeds_campaign_diff_multi(arr, 1, *tail(reps[2])))
    return rcs, reps, d, L.madsim_hip_last_error().decode()


BAD_LISTS = [
    ("equal neighbours", [1, 5, 5, 9], 1),
    ("a descending pair at position 0", [7, 3, 10, 11, 12], 0),
    ("a descending pair at the last position", list(range(100, 164)) + [20], 63),
    ("a descending pair exactly at a batch boundary", list(range(0, 64)) + [10] + list(range(200, 263)), 63),      # batch = 64: positions 63, 64
    ("the first of two bad pairs is named", [0, 4, 2, 9, 8], 1),
    ("2^64 - 1 twice", [5, U64, U64], 1),
]


@pytest.mark.parametrize("what,seeds,position", BAD_LISTS, ids=[b[0] for b in BAD_LISTS])
def test_a_list_that_does_not_ascend_is_refused_with_its_position(what, seeds, position):
    rcs, _, msg = _call(seeds, batch=64)
    assert rcs == (E_ARG,) * 3, (what, rcs)
    assert f"seeds[{position}]" in msg and f"seeds[{position + 1}]" in msg and "ascend" in msg, (what, msg)
    rcs, _, _, msg = _call_diff(seeds, batch=64)
    assert rcs == (E_ARG,) * 3 and f"seeds[{position}]" in msg, (what, rcs, msg)
    for parts in (_parts(collect=4), _parts(stats=(1, 2)), _parts(groups=(14, 0, 8)), _parts(4, (1, 2), (14, 0, 8))):
        assert _call(seeds, batch=64, parts=parts)[0] == (E_ARG,) * 3, what


def test_argument_errors_need_no_gpu():
    """Told before any context is looked at, so these hold with and without a device (the contexts here are null)."""
    rcs, _, msg = _call(None, n=5)
    assert rcs == (E_ARG,) * 3 and "null seed list" in msg                                    # NULL list with n > 0
    assert _call_diff(None, n=5)[0] == (E_ARG,) * 3
    good = [3, 4, 9, 1 << 40, U64]
    assert _call(good, report=False)[0] == (E_ARG,) * 3                                       # null report
    assert _call(good, in_flight=9)[0] == (E_ARG,) * 3
    assert _call(good, flags=A.CAMPAIGN_RESOLVE | 9 << A.CAMPAIGN_RESOLVE_ROUNDS_SHIFT)[0] == (E_ARG,) * 3
    # each present part's own checks
    assert _call(good, flags=A.CAMPAIGN_STOP_AT_CAP, parts=_parts(collect=0))[0] == (E_ARG,) * 3
    assert _call(good, parts=_parts(stats=(0, 2)))[0] == (E_ARG,) * 3
    assert _call(good, parts=_parts(stats=(1, 17)))[0] == (E_ARG,) * 3
    assert _call(good, parts=_parts(groups=(14, 6, 8)))[0] == (E_ARG,) * 3
    assert _call(good, flags=A.CAMPAIGN_STOP_AT_GROUPS, parts=_parts(groups=(14, 0, 0)))[0] == (E_ARG,) * 3
    d = A.Diff()
    assert _call_diff(good, d=d)[0] == (E_ARG,) * 3                                           # fields == 0
    # the grouping form's batch limit applies to min(batch, n): a short list under a huge batch is no argument error ...
    rcs, _, _ = _call(good, batch=1 << 40, parts=_parts(groups=(14, 0, 8)))
    assert rcs[1] == E_NOINIT and rcs[2] == E_NOINIT and rcs[0] != E_ARG
    # ... and flags that belong to an absent part are ignored: no E_ARG for STOP_AT_CAP / STOP_AT_GROUPS without their parts
    rcs, _, _ = _call(good, flags=A.CAMPAIGN_STOP_AT_CAP | A.CAMPAIGN_STOP_AT_GROUPS | A.CAMPAIGN_LIST_RUNNER)
    assert rcs[1] == E_NOINIT and rcs[2] == E_NOINIT and rcs[0] != E_ARG
    # a valid call without a context fails loudly, never with a report of nothing
    for parts in ((None, None, None), _parts(collect=4), _parts(4, (1, 2), (14, 0, 8))):
        rcs, _, _ = _call(good, parts=parts)
        assert rcs[1] == E_NOINIT and rcs[2] == E_NOINIT
    assert _call_diff(good)[0][1:] == (E_NOINIT, E_NOINIT)


def test_an_empty_list_returns_zero_and_initialised_reports():
    """n == 0: 0 from the default and the context form, with or without a device, a NULL list included; the reports as for total == 0."""
    for seeds in (None, []):
        for parts in ((None, None, None), _parts(4, (1, 2), (14, 0, 8))):
            for f in (parts[0], parts[1], parts[2]):
                if f is not None:                                                             # stale values going in
                    for name in ("n_listed", "n", "n_top", "n_groups", "n_grouped", "n_ungrouped"):
                        if hasattr(f, name):
                            setattr(f, name, 99)
            rcs, reps, _ = _call(seeds, n=0, parts=parts)
            assert rcs[0] == 0 and rcs[1] == 0, rcs
            for rep in reps[:2]:
                assert (rep.seeds_run, rep.batches_run, rep.batches_launched, rep.n_failed, rep.n_runner, rep.first_failing_seed) == (0, 0, 0, 0, 0, U64)
            col, st, grp = parts
            if col is not None:
                assert col.n_listed == 0 and not any(col.n_by_verdict)
                assert (st.n, st.n_top) == (0, 0) and all(st.metric[m].min == U64 and st.metric[m].max == 0 for m in range(A.STAT_METRICS))
                assert (grp.n_groups, grp.n_grouped, grp.n_ungrouped) == (0, 0, 0)
        d = A.Diff()
        d.fields, d.n_differ, d.n_compared = A.DIFF_ALL, 99, 99
        rcs, reps, d, _ = _call_diff(seeds, n=0, d=d)
        assert rcs[0] == 0 and rcs[1] == 0 and (d.n_differ, d.n_compared, d.n_listed) == (0, 0, 0)
        assert all(r.seeds_run == 0 and r.first_failing_seed == U64 for pair in reps[:2] for r in pair)


def test_the_python_wrapper_refuses_and_never_reorders():
    w = workload.pingpong(4, 8)
    for bad in ([5, 3, 9], [1, 2, 2, 3], np.array([9, 1], dtype=np.uint64), (4, 4)):
        for call in (lambda s: runtime.run_campaign_seeds(w, s), lambda s: runtime.run_campaign_diff_seeds(w, s),
                     lambda s: runtime.run_campaign_seeds_multi([], w, s), lambda s: runtime.run_campaign_diff_seeds_multi([], w, s)):
            with pytest.raises(runtime.MadsimHipError, match=r"numpy\.unique"):
                call(bad)
    with pytest.raises(runtime.MadsimHipError, match=r"seeds\[2\] = 7 is not below seeds\[3\] = 7"):
        runtime.seed_list([1, 5, 7, 7, 2])
    for bad in ([-1, 2], [0.5, 2], [1 << 64], np.array([-3, 4]), np.zeros((2, 2), dtype=np.uint64), np.array([1.0, 2.0])):
        with pytest.raises(runtime.MadsimHipError):
            runtime.seed_list(bad)
    # what it hands the library is the caller's list, in the caller's order, as contiguous uint64
    for good in ([0, 1, 1 << 32, 1 << 63, U64], range(10, 20), np.arange(50, dtype=np.int64)[::5], np.array([3, 9], dtype=np.uint32), []):
        arr = runtime.seed_list(good)
        assert arr.dtype == np.uint64 and arr.flags["C_CONTIGUOUS"] and [int(x) for x in arr] == [int(x) for x in good]
    unsorted = [9, 1, 5]
    with pytest.raises(runtime.MadsimHipError):
        runtime.seed_list(unsorted)
    assert unsorted == [9, 1, 5]
    # observe= explains a list or groups: without either it is refused before anything runs
    with pytest.raises(runtime.MadsimHipError, match="observe"):
        runtime._campaign_seeds(None, None, w, None, None, None, collect=None, stats=None, groups=None, resolve=None, observe=8)
