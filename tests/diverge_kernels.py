"""A direct driver for diverge_kernel: the launcher libmadsim_hip.so exports (madsim_k_launch_diverge; csrc/sim_kernel.h) over arrays of the
caller's making, with the buffers as madsim_hip_diverge_seeds hands them over.  Test-only: tests/test_diverge_kernels.py feeds it synthetic
rows and holds every record and context word against tests/diverge_ref.py.

Every buffer is checked on the host against the size the launcher demands before anything is launched; the two buffers a launch writes
are followed by a guard region filled with PATTERN that must come back intact, and every input must come back as it went in."""
import ctypes as C
import os
import re

import numpy as np
import torch

from madsim_amd import _abi as A
from madsim_amd import runtime

DIVERGE_WAVES = 1024
PATTERN, GUARD_BYTES = 0xA5, 512
RESULT_BYTES = np.dtype(A.RESULT_DTYPE).itemsize
RECORD_BYTES = np.dtype(A.DIVERGENCE_DTYPE).itemsize


def header_constants():
    path = os.path.join(os.path.dirname(os.path.abspath(runtime.__file__)), "csrc", "sim_kernel.h")
    with open(path) as f:
        return {k: int(v) for k, v in re.findall(r"^#define\s+MADSIM_K_DIVERGE_(\w+)\s+(\d+)u\b", f.read(), re.M)}


assert header_constants() == {"WAVES": DIVERGE_WAVES}, header_constants()
assert RESULT_BYTES == 48 and RECORD_BYTES == 184 == 23 * 8

_bound = None


def _lib():
    global _bound
    if _bound is None:
        L = runtime.lib()
        p, u64, u32 = C.c_void_p, C.c_uint64, C.c_uint32
        L.madsim_k_launch_diverge.argtypes = [p, p, u64, p, p, u64, p, p, p, p, p, p, p, u64, u32, p, p, p]
        L.madsim_k_launch_diverge.restype = C.c_int
        _bound = L
    return _bound


def _upload(a, n_bytes):
    """Host array `a` as a uint8 device tensor of exactly its bytes (16 zero bytes for an empty one: a pointer the launcher may see)."""
    a = np.ascontiguousarray(a)
    assert a.nbytes == n_bytes, (a.nbytes, n_bytes)
    if a.nbytes == 0:
        return torch.zeros(16, dtype=torch.uint8, device="cuda")
    return torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).cuda()


def _guarded(n_bytes):
    return torch.full((n_bytes + GUARD_BYTES,), PATTERN, dtype=torch.uint8, device="cuda")


def _need(t, n_bytes, what):
    assert t.is_cuda and t.is_contiguous() and t.dtype == torch.uint8 and t.data_ptr() % 16 == 0, what
    assert t.numel() >= n_bytes, (what, t.numel(), n_bytes)


def diverge(logs_a, logs_b, log_len_a, log_len_b, obs_a, obs_b, obs_len_a, obs_len_b, res_a, res_b, seeds, win):
    """(records ndarray[A.DIVERGENCE_DTYPE], context rows uint64[n, 3 * win]) of one diverge_kernel launch over host arrays: logs uint8[n, log_cap],
    obs uint64[n, obs_cap], four uint64[n] length arrays, two result arrays, uint64[n] seeds."""
    n, log_cap = logs_a.shape
    obs_cap = obs_a.shape[1]
    assert 1 <= n < 1 << 32 and 0 <= win <= A.DIVERGE_MAX_WIN
    assert logs_b.shape == (n, log_cap) and obs_a.shape == obs_b.shape == (n, obs_cap) and logs_a.dtype == np.uint8 and obs_a.dtype == np.uint64
    ins = [(logs_a, n * log_cap), (logs_b, n * log_cap), (obs_a, 8 * n * obs_cap), (obs_b, 8 * n * obs_cap)]
    ins += [(np.asarray(x, dtype=np.uint64), 8 * n) for x in (log_len_a, log_len_b, obs_len_a, obs_len_b)]
    ins += [(res_a, n * RESULT_BYTES), (res_b, n * RESULT_BYTES), (np.asarray(seeds, dtype=np.uint64), 8 * n)]
    dev = [_upload(a, nb) for a, nb in ins]
    for t, (a, nb) in zip(dev, ins):
        _need(t, nb, "input")
    recs, ctx = _guarded(n * RECORD_BYTES), _guarded(24 * win * n)
    _need(recs, n * RECORD_BYTES, "recs"); _need(ctx, 24 * win * n, "ctx")
    ptr = [t.data_ptr() for t in dev]
    rc = _lib().madsim_k_launch_diverge(ptr[0] if log_cap else None, ptr[1] if log_cap else None, log_cap, ptr[2] if obs_cap else None,
                                        ptr[3] if obs_cap else None, obs_cap, ptr[4], ptr[5], ptr[6], ptr[7], ptr[8], ptr[9], ptr[10], n, win,
                                        recs.data_ptr(), ctx.data_ptr() if win else None, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert bool((recs[n * RECORD_BYTES:] == PATTERN).all()), "recs: bytes behind the records were written"
    assert bool((ctx[24 * win * n:] == PATTERN).all()), "ctx: bytes behind the context rows were written"
    for t, (a, nb) in zip(dev, ins):                                            # the inputs are read, never written
        assert nb == 0 or t.cpu().numpy().tobytes() == np.ascontiguousarray(a).tobytes(), "an input array was modified"
    return (recs[:n * RECORD_BYTES].cpu().numpy().view(A.DIVERGENCE_DTYPE).copy(),
            ctx[:24 * win * n].cpu().numpy().view(np.uint64).reshape(n, 3 * win).copy())
