"""A direct driver for the paired campaign's report kernels: the launchers libmadsim_hip.so exports (madsim_k_launch_paired and its _list
form; csrc/sim_kernel.h) over two madsim_result_t arrays of the caller's making, with the buffers prepared as the campaign prepares them.
Test-only: tests/test_paired_kernels.py feeds it synthetic arrays and holds every word and every top record against tests/paired_ref.py.

Every buffer is checked on the host against the size the launcher demands before anything is launched; every buffer a launch writes is
followed by a guard region filled with PATTERN that must come back intact, and so must the candidate words of workgroups the grid does not
have and the top records behind a row's entries (both start as PATTERN: the kernels only ever store there, they never accumulate)."""
import ctypes as C
import os
import re

import numpy as np
import torch

from madsim_amd import _abi as A
from madsim_amd import runtime
from tests import paired_ref as R

WORDS, HEAD_WORDS, CAND_WORDS = 1466, 58, 65536
HIST_WORDS, TOP, WGS = 8 * 256 // 2, 16, 256
PATTERN, GUARD_BYTES = 0xA5, 512
RESULT_BYTES = np.dtype(A.RESULT_DTYPE).itemsize


def header_constants():
    """MADSIM_K_PAIRED_* as csrc/sim_kernel.h states them."""
    path = os.path.join(os.path.dirname(os.path.abspath(runtime.__file__)), "csrc", "sim_kernel.h")
    with open(path) as f:
        return {k: int(v) for k, v in re.findall(r"^#define\s+MADSIM_K_PAIRED_(\w+)\s+(\d+)u\b", f.read(), re.M)}


assert header_constants() == {"HEAD_WORDS": HEAD_WORDS, "WORDS": WORDS, "CAND_WORDS": CAND_WORDS}, header_constants()
assert (WORDS, HEAD_WORDS, RESULT_BYTES) == (R.WORDS, R.HEAD_WORDS, 48) and WORDS == HEAD_WORDS + HIST_WORDS + 8 * TOP * 3

_bound = None


def _lib():
    global _bound
    if _bound is None:
        L = runtime.lib()
        p, u64, u32 = C.c_void_p, C.c_uint64, C.c_uint32
        L.madsim_k_launch_paired.argtypes, L.madsim_k_launch_paired.restype = [p, p, u64, u64, u32, u32, u32, p, p, p], C.c_int
        L.madsim_k_launch_paired_list.argtypes, L.madsim_k_launch_paired_list.restype = [p, p, u64, p, u32, u32, u32, p, p, p], C.c_int
        _bound = L
    return _bound


def upload(results):
    """A numpy array of A.RESULT_DTYPE as a uint8 tensor on the device."""
    results = np.ascontiguousarray(results)
    assert results.dtype == np.dtype(A.RESULT_DTYPE) and results.ndim == 1
    return torch.from_numpy(results.view(np.uint8).copy()).cuda()


def upload_seeds(seeds):
    seeds = np.ascontiguousarray(seeds, dtype=np.uint64)
    return torch.from_numpy(seeds.view(np.uint8).copy()).cuda()


def _guarded(n_bytes):
    return torch.full((n_bytes + GUARD_BYTES,), PATTERN, dtype=torch.uint8, device="cuda")


def _need(t, n_bytes, what):
    assert t.is_cuda and t.is_contiguous() and t.dtype == torch.uint8 and t.data_ptr() % 16 == 0, what
    assert t.numel() >= n_bytes, (what, t.numel(), n_bytes)


def refused(d_a, d_b, count, include_a, include_b, top_k, with_cand=True):
    """The launcher's return value for arguments it must refuse (nothing is launched, so plain buffers do)."""
    words, cand = torch.zeros(8 * WORDS, dtype=torch.uint8, device="cuda"), torch.zeros(8 * CAND_WORDS, dtype=torch.uint8, device="cuda")
    rc = _lib().madsim_k_launch_paired(d_a.data_ptr(), d_b.data_ptr(), count, 0, include_a, include_b, top_k, words.data_ptr(),
                                       cand.data_ptr() if with_cand else None, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert not bool(words.any()) and not bool(cand.any())
    return rc


def paired(d_a, d_b, count, seeds, include_a, include_b, top_k):
    """words: uint64[WORDS] of paired_fold_kernel + paired_top_kernel on freshly prepared buffers — the head and the histograms zero, the top
    records and the candidate words PATTERN.  `seeds`: seed0 (the range form) or a device tensor from upload_seeds (the list form).  Asserts the
    guards intact, the candidate words of workgroups beyond the grid (all of them when top_k == 0) untouched, and the top records behind a
    row's min(top_k, n) entries untouched; those come back as zeros, as the campaign's prepared words would hold them."""
    assert 1 <= count < 1 << 32 and 0 < include_a < 16 and 0 < include_b < 16 and 0 <= top_k <= TOP, (count, include_a, include_b, top_k)
    _need(d_a, count * RESULT_BYTES, "side A")
    _need(d_b, count * RESULT_BYTES, "side B")
    words = _guarded(8 * WORDS)
    words[:8 * (HEAD_WORDS + HIST_WORDS)] = 0
    cand = _guarded(8 * CAND_WORDS)
    _need(words, 8 * WORDS, "words"); _need(cand, 8 * CAND_WORDS, "candidates")
    stream = torch.cuda.current_stream().cuda_stream
    if isinstance(seeds, torch.Tensor):
        _need(seeds, 8 * count, "seed list")
        rc = _lib().madsim_k_launch_paired_list(d_a.data_ptr(), d_b.data_ptr(), count, seeds.data_ptr(), include_a, include_b, top_k, words.data_ptr(),
                                                cand.data_ptr(), stream)
    else:
        assert 0 <= seeds and seeds + count <= 1 << 64, (seeds, count)
        rc = _lib().madsim_k_launch_paired(d_a.data_ptr(), d_b.data_ptr(), count, seeds, include_a, include_b, top_k, words.data_ptr(),
                                           cand.data_ptr(), stream)
    assert rc == 0, rc
    torch.cuda.synchronize()
    for t, n, what in ((words, 8 * WORDS, "words"), (cand, 8 * CAND_WORDS, "candidates")):
        assert bool((t[n:] == PATTERN).all()), f"{what}: the guard behind the buffer was written"
    grid = max(1, min(WGS, (count + 1023) // 1024))
    c = cand[:8 * CAND_WORDS].view(8, WGS, TOP * 16)
    assert bool((c[:, grid if top_k else 0:] == PATTERN).all()), "candidate words no workgroup of the grid owns were written"
    w = words[:8 * WORDS].cpu().numpy().view(np.uint64).copy()
    top = w[HEAD_WORDS + HIST_WORDS:].reshape(8, TOP, 3)
    untouched = np.uint64(int.from_bytes(bytes([PATTERN]) * 8, "little"))
    for j in range(8):
        n = min(top_k, int(w[2 + j]))
        assert (top[j, n:] == untouched).all(), f"top records behind the {n} entries of row {j} were written"
        top[j, n:] = 0
    return w
