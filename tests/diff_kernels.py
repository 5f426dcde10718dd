"""A direct driver for the differential campaign's report kernels: the launcher libmadsim_hip.so exports (madsim_k_launch_diff;
csrc/sim_kernel.h) over two madsim_result_t arrays of the caller's making, with the buffers prepared as run_variants_impl prepares them.
Test-only: tests/test_diff_kernels.py feeds it synthetic arrays and holds every word, record and wave count against tests/diff_ref.py.

Every buffer is checked on the host against the size the launcher demands before anything is launched; every buffer a launch writes is
followed by a guard region filled with PATTERN that must come back intact, and so must the record bytes behind the batch's list."""
import ctypes as C
import os
import re

import numpy as np
import torch

from madsim_amd import _abi as A
from madsim_amd import runtime

DIFF_WORDS, WAVES = 74, 1024
PATTERN, GUARD_BYTES = 0xA5, 512
RESULT_BYTES, RECORD_BYTES = np.dtype(A.RESULT_DTYPE).itemsize, np.dtype(A.DIFF_RECORD_DTYPE).itemsize


def header_constants():
    """MADSIM_K_DIFF_WORDS and MADSIM_K_COLLECT_WAVES as csrc/sim_kernel.h states them."""
    path = os.path.join(os.path.dirname(os.path.abspath(runtime.__file__)), "csrc", "sim_kernel.h")
    with open(path) as f:
        return {k: int(v) for k, v in re.findall(r"^#define\s+MADSIM_K_(DIFF_WORDS|COLLECT_WAVES)\s+(\d+)u\b", f.read(), re.M)}


assert header_constants() == {"DIFF_WORDS": DIFF_WORDS, "COLLECT_WAVES": WAVES}, header_constants()
assert (RESULT_BYTES, RECORD_BYTES) == (48, 104)

_bound = None


def _lib():
    global _bound
    if _bound is None:
        L = runtime.lib()
        p, u64, u32 = C.c_void_p, C.c_uint64, C.c_uint32
        L.madsim_k_launch_diff.argtypes, L.madsim_k_launch_diff.restype = [p, p, u64, u64, u32, p, p, p, u64, p], C.c_int
        _bound = L
    return _bound


def upload(results):
    """A numpy array of A.RESULT_DTYPE as a uint8 tensor on the device."""
    results = np.ascontiguousarray(results)
    assert results.dtype == np.dtype(A.RESULT_DTYPE) and results.ndim == 1
    return torch.from_numpy(results.view(np.uint8).copy()).cuda()


def _guarded(n_bytes, fill=None):
    t = torch.full((n_bytes + GUARD_BYTES,), PATTERN, dtype=torch.uint8, device="cuda")
    if fill is not None:
        t[:n_bytes] = fill
    return t


def _need(t, n_bytes, what):
    assert t.is_cuda and t.is_contiguous() and t.dtype == torch.uint8 and t.data_ptr() % 16 == 0, what
    assert t.numel() >= n_bytes, (what, t.numel(), n_bytes)


def diff(d_a, d_b, count, seed0, fields, cap):
    """(words: uint64[DIFF_WORDS], wave counts: uint32[waves of the grid], records: ndarray[DIFF_RECORD_DTYPE] of min(cap, n_differ)) of
    diff_count_kernel + diff_write_kernel on freshly prepared buffers.  Asserts the guards intact, the wave counts behind the grid's waves
    untouched and the record bytes behind the batch's list untouched."""
    assert 1 <= count < 1 << 32 and 0 <= seed0 and seed0 + count <= 1 << 64, (count, seed0)
    assert 0 < fields <= A.DIFF_ALL and 0 <= cap
    room = min(cap, count)                                     # what the campaign gives a batch: no batch lists more
    _need(d_a, count * RESULT_BYTES, "side A")
    _need(d_b, count * RESULT_BYTES, "side B")
    words = _guarded(8 * DIFF_WORDS, 0)
    wcnt = _guarded(4 * WAVES)                                 # scratch the campaign does not prepare
    recs = _guarded(RECORD_BYTES * room)
    _need(words, 8 * DIFF_WORDS, "words"); _need(wcnt, 4 * WAVES, "wave counts"); _need(recs, RECORD_BYTES * room, "records")
    rc = _lib().madsim_k_launch_diff(d_a.data_ptr(), d_b.data_ptr(), count, seed0, fields, words.data_ptr(), wcnt.data_ptr(),
                                     recs.data_ptr() if room else None, room, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, rc
    torch.cuda.synchronize()
    for t, n, what in ((words, 8 * DIFF_WORDS, "words"), (wcnt, 4 * WAVES, "wave counts"), (recs, RECORD_BYTES * room, "records")):
        assert bool((t[n:] == PATTERN).all()), f"{what}: the guard behind the buffer was written"
    w = words[:8 * DIFF_WORDS].cpu().numpy().view(np.uint64).copy()
    n_waves = 4 * max(1, min(256, (count + 1023) // 1024))
    assert bool((wcnt[4 * n_waves:] == PATTERN).all()), "wave counts behind the grid's waves were written"
    waves = wcnt[:4 * n_waves].cpu().numpy().view(np.uint32).copy()
    n = min(room, int(w[0]))
    assert int(w[0]) <= count
    assert bool((recs[RECORD_BYTES * n:] == PATTERN).all()), "record bytes behind the batch's list were written"
    got = recs[:RECORD_BYTES * n].cpu().numpy().view(A.DIFF_RECORD_DTYPE).copy()
    return w, waves, got
