"""A direct driver for order_fold_kernel / order_extract_kernel: the launcher libmadsim_hip.so exports (madsim_k_launch_probe_order_form;
csrc/sim_kernel.h) over arrays of the caller's making, with the buffers as madsim_hip_probe_order_range hands them over.  Test-only:
tests/test_probe_order_kernels.py feeds it synthetic rows, in both forms of the fold kernel (the workgroup accumulator in LDS and every
update straight to the global matrix), and holds the entries and the count words against tests/order_ref.py.

Every buffer is checked on the host against the size the launcher demands before anything is launched; every buffer a launch writes is
followed by a guard region filled with PATTERN that must come back intact, every input must come back as it went in, and the matrix must be
all zero again after every launch — which is why `launches` > 1 can run the same input again on the same matrix."""
import ctypes as C
import os
import re

import numpy as np
import torch

from madsim_amd import _abi as A
from madsim_amd import runtime

ORDER_WORDS, MATRIX_WORDS, ORDER_WAVES, ERR_TAG = 12, 8192, 1024, 2
PATTERN, GUARD_BYTES = 0xA5, 512
RESULT_BYTES = np.dtype(A.RESULT_DTYPE).itemsize
ENTRY_BYTES = np.dtype(A.PROBE_ORDER_PAIR_DTYPE).itemsize


def header_constants():
    path = os.path.join(os.path.dirname(os.path.abspath(runtime.__file__)), "csrc", "sim_kernel.h")
    with open(path) as f:
        return {k: int(v) for k, v in re.findall(r"^#define\s+MADSIM_K_PROBE_ORDER_(\w+)\s+(\d+)u\b", f.read(), re.M)}


assert header_constants() == {"WORDS": ORDER_WORDS, "MATRIX_WORDS": MATRIX_WORDS, "WAVES": ORDER_WAVES, "ERR_TAG": ERR_TAG}, header_constants()
assert RESULT_BYTES == 48 and ENTRY_BYTES == 72 and MATRIX_WORDS == 2 * 4 * A.PROBE_ORDER_MAX_VOCAB ** 2

_bound = None


def _lib():
    global _bound
    if _bound is None:
        L = runtime.lib()
        p, u64, u32 = C.c_void_p, C.c_uint64, C.c_uint32
        L.madsim_k_launch_probe_order_form.argtypes = [p, u64, p, p, p, u64, u32, p, u64, p, p, p, p, C.c_int]
        L.madsim_k_launch_probe_order_form.restype = C.c_int
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


def probe_order(rows, lens, results, seeds, include, vocab, launches=1, direct=False):
    """`launches` results, each (entries ndarray[A.PROBE_ORDER_PAIR_DTYPE] as the device wrote them, words uint64[ORDER_WORDS]), of
    madsim_k_launch_probe_order_form over host arrays: rows uint64[n, obs_cap], lens uint64[n], results ndarray[A.RESULT_DTYPE], seeds
    uint64[n], vocab: the vocabulary — every launch on the SAME matrix, zeroed once before the first.  With a non-zero error word the
    entries are empty.  `direct`: every update straight to the global matrix in place of the accumulator in LDS."""
    n, obs_cap = rows.shape
    vocab = np.ascontiguousarray(np.array([int(v) for v in vocab], dtype=np.uint64))
    m = len(vocab)
    assert rows.dtype == np.uint64 and 1 <= n <= 1 << 31 and 1 <= obs_cap <= A.CENSUS_MAX_OBS_CAP and n * obs_cap < (1 << 32) - 1
    assert 1 <= m <= A.PROBE_ORDER_MAX_VOCAB and include and not include & ~0xf
    ins = [(rows, 8 * n * obs_cap), (np.asarray(lens, dtype=np.uint64), 8 * n), (results, n * RESULT_BYTES), (np.asarray(seeds, dtype=np.uint64), 8 * n)]
    dev = [_upload(a, nb) for a, nb in ins]
    for t, (a, nb) in zip(dev, ins):
        _need(t, nb, "input")
    matrix = _guarded(4 * MATRIX_WORDS, 0)
    _need(matrix, 4 * MATRIX_WORDS, "matrix")
    out = []
    for _ in range(launches):
        words, ent = _guarded(8 * ORDER_WORDS, 0), _guarded(m * m * ENTRY_BYTES, None)
        _need(words, 8 * ORDER_WORDS, "words"); _need(ent, m * m * ENTRY_BYTES, "entries")
        rc = _lib().madsim_k_launch_probe_order_form(dev[0].data_ptr(), obs_cap, dev[1].data_ptr(), dev[2].data_ptr(), dev[3].data_ptr(), n, include,
                                                     vocab.ctypes.data, m, matrix.data_ptr(), words.data_ptr(), ent.data_ptr(),
                                                     torch.cuda.current_stream().cuda_stream, 1 if direct else 0)
        assert rc == 0, rc
        torch.cuda.synchronize()
        for t, nb, what in ((matrix, 4 * MATRIX_WORDS, "matrix"), (words, 8 * ORDER_WORDS, "words"), (ent, m * m * ENTRY_BYTES, "entries")):
            assert bool((t[nb:] == PATTERN).all()), f"{what}: bytes behind the buffer were written"
        assert not bool(matrix[:4 * MATRIX_WORDS].any()), "the matrix is not all zero after the extract pass"
        for t, (a, nb) in zip(dev, ins):                                            # the inputs are read, never written
            assert t.cpu().numpy().tobytes() == np.ascontiguousarray(a).tobytes(), "an input array was modified"
        w = words[:8 * ORDER_WORDS].cpu().numpy().view(np.uint64).copy()
        ne = 0 if w[1] else int(w[0])
        assert ne <= m * m
        e = ent[:ne * ENTRY_BYTES].cpu().numpy().view(A.PROBE_ORDER_PAIR_DTYPE).copy()
        assert bool((ent[ne * ENTRY_BYTES:m * m * ENTRY_BYTES] == PATTERN).all()), "entries behind the chunk's cells were written"
        out.append((e, w))
    return out
