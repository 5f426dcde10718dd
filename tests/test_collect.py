"""Collecting campaigns (madsim_hip_run_campaign_collect and its _ctx_ / _multi forms) at the C-ABI boundary, without a GPU:
the two new structs against the header, the exported symbols, the argument errors that need no device, and the loud failure of a valid
call on a host without one.  What the list holds is tests/test_collect_gpu.py's business."""
import ctypes as C
import re

import numpy as np
import pytest

from madsim_amd import _abi as A
from madsim_amd import runtime, workload
from tests import cheader as H

E_ARG, E_HIP, E_NOINIT = -1, -2, -3


def _no_gpu():
    import torch
    return not torch.cuda.is_available()


def test_failure_and_collect_structs_match_the_header():
    # madsim_failure_t holds a madsim_result_t by value and is declared in two statements: joined here, laid out with the inner size given
    joined = re.sub(r"\bstruct\s+(madsim_failure)\s*\{([^{}]*)\}\s*;\s*typedef\s+struct\s+\1\s+(\w+)\s*;", r"typedef struct \1 {\2} \3;", H.header_text())
    S = H.structs(joined)
    inner = {"madsim_result_t": (H.layout(S["madsim_result_t"])[1], 8)}
    assert inner["madsim_result_t"][0] == 48
    assert [f[:2] for f in S["madsim_failure_t"]] == [("seed", "uint64_t"), ("result", "madsim_result_t")]
    assert [f[0] for f in S["madsim_collect_t"]] == ["failures", "cap", "n_listed", "n_by_verdict"]
    for name, cls, want_size in (("madsim_failure_t", A.Failure, 56), ("madsim_collect_t", A.Collect, 88)):
        offs, size = H.layout(S[name], inner)
        assert size == want_size == C.sizeof(cls), (name, size, C.sizeof(cls))
        assert [f[0] for f in cls._fields_] == [f[0] for f in S[name]], name
        for fname, _, _, _ in S[name]:
            assert getattr(cls, fname).offset == offs[fname], (name, fname)
    assert A.Failure.result.offset == 8 and A.Collect.n_by_verdict.offset == 24 and A.Collect.n_by_verdict.size == 64
    # the numpy view is the same 56 bytes: the seed, then the result's fields where madsim_result_t has them
    dt = np.dtype(A.FAILURE_DTYPE)
    assert dt.itemsize == 56 and dt.names == ("seed",) + np.dtype(A.RESULT_DTYPE).names
    for fname in np.dtype(A.RESULT_DTYPE).names:
        assert dt.fields[fname][1] == 8 + getattr(A.Result, fname).offset, fname
    D = H.defines()
    assert (int(D["MADSIM_CAMPAIGN_STOP_AT_FAILURE"].rstrip("u")), int(D["MADSIM_CAMPAIGN_LIST_RUNNER"].rstrip("u")),
            int(D["MADSIM_CAMPAIGN_STOP_AT_CAP"].rstrip("u"))) == (A.CAMPAIGN_STOP_AT_FAILURE, A.CAMPAIGN_LIST_RUNNER, A.CAMPAIGN_STOP_AT_CAP) == (1, 2, 4)
    assert int(D["MADSIM_HIP_ABI_VERSION"].rstrip("u")) == A.ABI_VERSION == 7          # additive: the version stays


def test_library_exports_the_three_entry_points():
    L = runtime.lib()
    fns = H.functions()
    for name in ("madsim_hip_run_campaign_collect", "madsim_hip_ctx_run_campaign_collect", "madsim_hip_run_campaign_collect_multi"):
        assert name in fns and hasattr(L, name), name
    plain = fns["madsim_hip_run_campaign"][1]
    assert fns["madsim_hip_run_campaign_collect"] == ("int", plain + ["madsim_collect_t*"])
    assert fns["madsim_hip_ctx_run_campaign_collect"] == ("int", ["madsim_hip_ctx_t*"] + plain + ["madsim_collect_t*"])
    assert fns["madsim_hip_run_campaign_collect_multi"] == ("int", ["madsim_hip_ctx_t* const*", "int"] + plain + ["madsim_collect_t*"])


def _call(col, flags=0, in_flight=0):
    """Every form of the call with the same arguments: the default context, an explicit (null) context, a list of contexts."""
    L = runtime.lib()
    w, cfg, lim, rep = workload.pingpong(4, 8), A.Config.default(), A.Limits(), A.Campaign()
    colp = C.byref(col) if col is not None else None
    arr = (C.c_void_p * 1)(None)
    return (L.madsim_hip_run_campaign_collect(w.ref(), C.byref(cfg), 0, 100, 0, in_flight, flags, C.byref(lim), C.byref(rep), colp),
            L.madsim_hip_ctx_run_campaign_collect(None, w.ref(), C.byref(cfg), 0, 100, 0, in_flight, flags, C.byref(lim), C.byref(rep), colp),
            L.madsim_hip_run_campaign_collect_multi(arr, 1, w.ref(), C.byref(cfg), 0, 100, 0, in_flight, flags, C.byref(lim), C.byref(rep), colp))


def _collect(cap, with_array=True):
    col = A.Collect()
    col.cap = cap
    col._keep = (A.Failure * max(cap, 1))()
    if with_array:
        col.failures = C.cast(col._keep, C.POINTER(A.Failure))
    return col


def test_argument_errors_need_no_gpu():
    """Told before any context is looked at, so these hold with and without a device (the contexts here are null)."""
    assert _call(None) == (E_ARG,) * 3                                                     # null col
    assert _call(_collect(4, with_array=False)) == (E_ARG,) * 3                            # cap > 0 without failures
    assert _call(_collect(0), flags=A.CAMPAIGN_STOP_AT_CAP) == (E_ARG,) * 3                # STOP_AT_CAP with cap == 0
    assert _call(_collect(4), in_flight=9) == (E_ARG,) * 3                                 # more than 8 batches in flight
    assert b"in flight" in runtime.lib().madsim_hip_last_error()
    L = runtime.lib()
    w, cfg, lim, col = workload.pingpong(4, 8), A.Config.default(), A.Limits(), _collect(4)
    assert L.madsim_hip_run_campaign_collect(w.ref(), C.byref(cfg), 0, 100, 0, 0, 0, C.byref(lim), None, C.byref(col)) == E_ARG       # null report
    # the mirror raises for the same things
    with pytest.raises(runtime.MadsimHipError):
        runtime.run_campaign_multi([], workload.pingpong(4, 8), 0, 100, collect=0, stop_at_cap=True)


def test_a_valid_call_without_a_context_fails_loudly():
    """Null contexts: never an empty list that looks like "no seed fails"."""
    col = _collect(4)
    col.n_listed = 77
    rcs = _call(col)
    assert rcs[1] == E_NOINIT and rcs[2] == E_NOINIT
    assert rcs[0] in (E_NOINIT, E_HIP) or not _no_gpu()


def test_no_gpu_means_loud_failure_not_an_empty_list():
    if not _no_gpu():
        pytest.skip("a GPU is present")
    w = workload.pingpong(4, 8)
    for kw in (dict(collect=16), dict(collect=0), dict(collect=16, list_runner=True, stop_at_cap=True)):
        with pytest.raises(runtime.MadsimHipError, match="HIP|context|initiali"):
            runtime.run_campaign(w, 0, 1000, **kw)
    with pytest.raises(runtime.MadsimHipError):
        runtime.Context(0)


def test_run_campaign_without_collect_is_the_call_it_was():
    """collect=None: the same entry point, the same arguments, the Campaign report alone as the return value — compared on the error
    path where no device is present (the same exception, the same message), and by signature everywhere."""
    import inspect
    for fn in (runtime.run_campaign, runtime.run_campaign_multi, runtime.Context.run_campaign):
        p = inspect.signature(fn).parameters
        assert (p["collect"].default, p["list_runner"].default, p["stop_at_cap"].default) == (None, False, False)
    names = list(inspect.signature(runtime.run_campaign).parameters)
    assert names[:8] == ["workload", "seed0", "total", "batch", "in_flight", "stop_at_failure", "config", "limits"]    # positional callers keep working
    rep = A.Campaign()
    assert [f[0] for f in rep._fields_] == ["seeds_run", "batches_run", "batches_launched", "first_failing_seed", "n_failed", "n_runner",
                                            "total_steps", "total_clock_ns", "kernel_ms", "wall_s"]
    if _no_gpu():
        w = workload.pingpong(4, 8)
        errs = []
        for kw in ({}, dict(collect=None)):
            with pytest.raises(runtime.MadsimHipError) as ei:
                runtime.run_campaign(w, 0, 1000, **kw)
            errs.append((type(ei.value), str(ei.value)))
        assert errs[0] == errs[1]
    # the plain entry points take no notice of the collecting form's flags: without a context they answer as they always did
    L = runtime.lib()
    w, cfg, lim = workload.pingpong(4, 8), A.Config.default(), A.Limits()
    assert L.madsim_hip_ctx_run_campaign(None, w.ref(), C.byref(cfg), 0, 100, 0, 0, A.CAMPAIGN_STOP_AT_CAP, C.byref(lim), C.byref(rep)) == E_NOINIT
