"""A direct driver for span_fold_kernel / span_witness_kernel: the launcher libmadsim_hip.so exports (madsim_k_launch_probe_spans_form;
csrc/sim_kernel.h) over arrays of the caller's making, with the buffers as madsim_hip_probe_spans_range hands them over.  Test-only:
tests/test_spans_kernels.py feeds it synthetic rows, in both forms of the fold kernel (the workgroup accumulator in LDS and every update
straight to the global records), and holds the decoded records and the count words against tests/spans_ref.py.

Every buffer is checked on the host against the size the launcher demands before anything is launched; every buffer a launch writes is
followed by a guard region filled with PATTERN that must come back intact, and every input must come back as it went in.  The records need
not be zero before a launch (the launcher zeroes them) — which is why `launches` > 1 can run the same input again over the same buffers."""
import ctypes as C
import os
import re

import numpy as np
import torch

from madsim_amd import _abi as A
from madsim_amd import runtime

SPANS_WORDS, REC_WORDS, UNCOUNTED = 8, 280, 4
PATTERN, GUARD_BYTES = 0xA5, 512
RESULT_BYTES = np.dtype(A.RESULT_DTYPE).itemsize


def header_constants():
    path = os.path.join(os.path.dirname(os.path.abspath(runtime.__file__)), "csrc", "sim_kernel.h")
    with open(path) as f:
        return {k: int(v) for k, v in re.findall(r"^#define\s+MADSIM_K_(PROBE_SPANS_WORDS|SPAN_REC_WORDS|SPAN_UNCOUNTED)\s+(\d+)u\b", f.read(), re.M)}


assert header_constants() == {"PROBE_SPANS_WORDS": SPANS_WORDS, "SPAN_REC_WORDS": REC_WORDS, "SPAN_UNCOUNTED": UNCOUNTED}, header_constants()
assert RESULT_BYTES == 48 and REC_WORDS == A.SPAN_REC_WORDS and 8 * REC_WORDS == np.dtype(A.SPAN_DTYPE).itemsize

_bound = None


def _lib():
    global _bound
    if _bound is None:
        L = runtime.lib()
        p, u64, u32 = C.c_void_p, C.c_uint64, C.c_uint32
        L.madsim_k_launch_probe_spans_form.argtypes = [p, p, u64, p, p, p, u64, u32, p, u64, p, p, p, p, p, C.c_int]
        L.madsim_k_launch_probe_spans_form.restype = C.c_int
        _bound = L
    return _bound


def _upload(a, n_bytes):
    a = np.ascontiguousarray(a)
    assert a.nbytes == n_bytes, (a.nbytes, n_bytes)
    return torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).cuda()


def _guarded(n_bytes, fill):
    t = torch.full((n_bytes + GUARD_BYTES,), PATTERN, dtype=torch.uint8, device="cuda")
    if fill is not None:
        t[:n_bytes] = fill
    return t


def _need(t, n_bytes, what):
    assert t.is_cuda and t.is_contiguous() and t.dtype == torch.uint8 and t.data_ptr() % 16 == 0, what
    assert t.numel() >= n_bytes, (what, t.numel(), n_bytes)


def decode(defs, recs, words, include, obs_cap):
    """The report a chunk's device records and words fold to — through the library's own host fold (madsim_k_fold_probe_spans) into empty
    records — as (spans ndarray[A.SPAN_DTYPE], n_counted, n_truncated, n_runner)."""
    m = len(defs)
    spans = runtime.empty_spans(m)
    ps = A.ProbeSpans(include=include, obs_cap=obs_cap, n_spans=m)
    ps.defs, ps.spans = defs.ctypes.data_as(C.POINTER(A.SpanDef)), spans.ctypes.data_as(C.POINTER(A.Span))
    recs, words = np.ascontiguousarray(recs, dtype=np.uint64), np.ascontiguousarray(words, dtype=np.uint64)
    assert runtime.lib().madsim_k_fold_probe_spans(C.byref(ps), words.ctypes.data_as(C.c_void_p), recs.ctypes.data_as(C.c_void_p), m) == 0
    return spans, tuple(ps.n_counted), int(ps.n_truncated), int(ps.n_runner)


def probe_spans(rows, times, lens, results, seeds, include, defs, launches=1, direct=False):
    """`launches` results, each (records uint64[m, REC_WORDS] as the device wrote them, words uint64[SPANS_WORDS], st uint32[n, m], dur
    uint64[n, m]), of madsim_k_launch_probe_spans_form over host arrays: rows / times uint64[n, obs_cap], lens uint64[n], results
    ndarray[A.RESULT_DTYPE], seeds uint64[n], defs ndarray[A.SPAN_DEF_DTYPE] — every launch over the SAME record, state and duration
    buffers, never cleared by the caller.  `direct`: every update straight to the global records in place of the accumulator in LDS."""
    n, obs_cap = rows.shape
    m = len(defs)
    defs = np.ascontiguousarray(defs)
    assert rows.dtype == np.uint64 and times.dtype == np.uint64 and times.shape == rows.shape
    assert 1 <= n <= 1 << 31 and 1 <= obs_cap <= A.CENSUS_MAX_OBS_CAP and n * obs_cap < (1 << 32) - 1
    assert 1 <= m <= A.PROBE_SPANS_MAX and include and not include & ~0xf
    ins = [(rows, 8 * n * obs_cap), (times, 8 * n * obs_cap), (np.asarray(lens, dtype=np.uint64), 8 * n), (results, n * RESULT_BYTES),
           (np.asarray(seeds, dtype=np.uint64), 8 * n)]
    dev = [_upload(a, nb) for a, nb in ins]
    for t, (a, nb) in zip(dev, ins):
        _need(t, nb, "input")
    sizes = (("records", 8 * REC_WORDS * m), ("states", 4 * n * m), ("durations", 8 * n * m))
    recs, st, dur = (_guarded(nb, None) for _, nb in sizes)             # (PATTERN all over: nothing here needs to be zero)
    for t, (what, nb) in zip((recs, st, dur), sizes):
        _need(t, nb, what)
    out = []
    for _ in range(launches):
        words = _guarded(8 * SPANS_WORDS, 0)
        _need(words, 8 * SPANS_WORDS, "words")
        rc = _lib().madsim_k_launch_probe_spans_form(dev[0].data_ptr(), dev[1].data_ptr(), obs_cap, dev[2].data_ptr(), dev[3].data_ptr(), dev[4].data_ptr(), n,
                                                     include, defs.ctypes.data, m, st.data_ptr(), dur.data_ptr(), recs.data_ptr(), words.data_ptr(),
                                                     torch.cuda.current_stream().cuda_stream, 1 if direct else 0)
        assert rc == 0, rc
        torch.cuda.synchronize()
        for t, (what, nb) in zip((recs, st, dur, words), sizes + (("words", 8 * SPANS_WORDS),)):
            assert bool((t[nb:] == PATTERN).all()), f"{what}: bytes behind the buffer were written"
        for t, (a, nb) in zip(dev, ins):                                            # the inputs are read, never written
            assert t.cpu().numpy().tobytes() == np.ascontiguousarray(a).tobytes(), "an input array was modified"
        w = words[:8 * SPANS_WORDS].cpu().numpy().view(np.uint64).copy()
        assert int(w[0]) == m and int(w[1]) == 0
        out.append((recs[:8 * REC_WORDS * m].cpu().numpy().view(np.uint64).reshape(m, REC_WORDS).copy(), w,
                    st[:4 * n * m].cpu().numpy().view(np.uint32).reshape(n, m).copy(), dur[:8 * n * m].cpu().numpy().view(np.uint64).reshape(n, m).copy()))
    return out


def refused(**kw):
    """The launcher's return code for sizes and arrays it is not written for, over tiny real buffers: nothing may be launched."""
    a = dict(n=1, obs_cap=1, include=0xf, m=1, flags=0, missing=None)
    a.update(kw)
    bufs = {k: torch.zeros(4096, dtype=torch.uint8, device="cuda") for k in ("obs", "times", "len", "res", "seeds", "st", "dur", "recs", "words")}
    ptr = {k: (None if a["missing"] == k else t.data_ptr()) for k, t in bufs.items()}
    defs = np.zeros(max(a["m"], 1), dtype=A.SPAN_DEF_DTYPE)
    defs["flags"] = a["flags"]
    rc = _lib().madsim_k_launch_probe_spans_form(ptr["obs"], ptr["times"], a["obs_cap"], ptr["len"], ptr["res"], ptr["seeds"], a["n"], a["include"],
                                                 None if a["missing"] == "defs" else defs.ctypes.data, a["m"], ptr["st"], ptr["dur"], ptr["recs"],
                                                 ptr["words"], torch.cuda.current_stream().cuda_stream, 0)
    torch.cuda.synchronize()
    assert rc == 0 or all(not bool(t.any()) for t in bufs.values())
    return rc
