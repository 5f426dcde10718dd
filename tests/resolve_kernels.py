"""A direct driver for the resolving campaign's kernels: the launchers libmadsim_hip.so exports (madsim_k_launch_resolve_list,
madsim_k_launch_resolve_scatter; csrc/sim_kernel.h) over arrays of the caller's making, with the buffers as resolve_results of madsim_hip.cpp
hands them over.  Test-only: tests/test_resolve_kernels.py feeds it synthetic result arrays and holds the lists against numpy.

Every buffer is checked on the host against the size the launcher demands before anything is launched — the scatter's indices too: distinct
and inside the result array —, and every buffer a launch writes is followed by a guard region filled with PATTERN that must come back
intact; so must the list entries behind the count the kernels report."""
import ctypes as C
import os
import re

import numpy as np
import torch

from madsim_amd import _abi as A
from madsim_amd import runtime

RESOLVE_WAVES, RESOLVE_CHUNKS = 1024, 3
PATTERN, GUARD_BYTES = 0xA5, 512
RESULT_BYTES = np.dtype(A.RESULT_DTYPE).itemsize


def header_constants():
    """The MADSIM_K_RESOLVE_* sizes as csrc/sim_kernel.h states them."""
    path = os.path.join(os.path.dirname(os.path.abspath(runtime.__file__)), "csrc", "sim_kernel.h")
    with open(path) as f:
        return {k: int(v) for k, v in re.findall(r"^#define\s+MADSIM_K_RESOLVE_(\w+)\s+(\d+)u\b", f.read(), re.M)}


assert header_constants() == {"WAVES": RESOLVE_WAVES, "CHUNKS": RESOLVE_CHUNKS}, header_constants()
assert RESULT_BYTES == 48 == 16 * RESOLVE_CHUNKS

_bound = None


def _lib():
    global _bound
    if _bound is None:
        L = runtime.lib()
        p, u64, u32 = C.c_void_p, C.c_uint64, C.c_uint32
        L.madsim_k_launch_resolve_list.argtypes, L.madsim_k_launch_resolve_list.restype = [p, u64, u64, u32, p, p, p, p, p], C.c_int
        L.madsim_k_launch_resolve_scatter.argtypes, L.madsim_k_launch_resolve_scatter.restype = [p, p, p, u64, p], C.c_int
        _bound = L
    return _bound


def rerunnable(verdicts, steps_maxed):
    """The rule, on the host: MADSIM_OVERFLOW always, MADSIM_STEP_LIMIT while the step cap can still grow."""
    v = np.asarray(verdicts)
    return (v == A.OVERFLOW) | ((v == A.STEP_LIMIT) & (not steps_maxed))


def upload(results):
    """A numpy array of A.RESULT_DTYPE as a uint8 tensor on the device."""
    results = np.ascontiguousarray(results)
    assert results.dtype == np.dtype(A.RESULT_DTYPE) and results.ndim == 1
    return torch.from_numpy(results.view(np.uint8).copy()).cuda()


def _guarded(n_bytes, data=None):
    """A uint8 device tensor of n_bytes + GUARD_BYTES, all PATTERN but the leading bytes that `data` (host bytes) fills."""
    t = torch.full((n_bytes + GUARD_BYTES,), PATTERN, dtype=torch.uint8, device="cuda")
    if data is not None:
        assert data.nbytes <= n_bytes
        t[:data.nbytes] = torch.from_numpy(data.view(np.uint8).copy()).cuda()
    return t


def _need(t, n_bytes, what):
    assert t.is_cuda and t.is_contiguous() and t.dtype == torch.uint8 and t.data_ptr() % 16 == 0, what
    assert t.numel() >= n_bytes, (what, t.numel(), n_bytes)


def _intact(t, n_bytes, what):
    assert bool((t[n_bytes:] == PATTERN).all()), f"{what}: bytes behind what the launch may write were written"


def _stream():
    return torch.cuda.current_stream().cuda_stream


def resolve_list(d_results, count, seed0, steps_maxed):
    """(m, seeds: uint64[m], idx: uint32[m]) of resolve_count_kernel + resolve_write_kernel on buffers nobody prepared (all PATTERN).  Asserts
    the guards intact and the list entries from m on untouched."""
    assert 1 <= count < 1 << 32 and 0 <= seed0 and seed0 + count <= 1 << 64 and steps_maxed in (0, 1), (count, seed0, steps_maxed)
    _need(d_results, count * RESULT_BYTES, "results")
    wave_cnt, total, seeds, idx = _guarded(4 * RESOLVE_WAVES), _guarded(4), _guarded(8 * count), _guarded(4 * count)
    _need(wave_cnt, 4 * RESOLVE_WAVES, "wave_cnt"); _need(total, 4, "total"); _need(seeds, 8 * count, "seeds"); _need(idx, 4 * count, "idx")
    rc = _lib().madsim_k_launch_resolve_list(d_results.data_ptr(), count, seed0, steps_maxed, wave_cnt.data_ptr(), total.data_ptr(), seeds.data_ptr(),
                                             idx.data_ptr(), _stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    _intact(wave_cnt, 4 * RESOLVE_WAVES, "wave_cnt"); _intact(total, 4, "total")
    m = int(total[:4].cpu().numpy().view(np.uint32)[0])
    assert 0 <= m <= count, m
    _intact(seeds, 8 * m, "seeds"); _intact(idx, 4 * m, "idx")            # (the guard and the entries from m on)
    waves = 4 * min((count + 1023) // 1024, 256)
    cnt = wave_cnt[:4 * RESOLVE_WAVES].cpu().numpy().view(np.uint32)
    assert int(cnt[:waves].sum()) == m and (cnt[waves:] == 0xA5A5A5A5).all()
    return m, seeds[:8 * m].cpu().numpy().view(np.uint64).copy(), idx[:4 * m].cpu().numpy().view(np.uint32).copy()


def scatter(out, rerun, idx):
    """out[idx[j]] = rerun[j] on the device: returns the result array afterwards.  `out`, `rerun`: numpy arrays of A.RESULT_DTYPE; idx: uint32."""
    out, rerun, idx = np.ascontiguousarray(out), np.ascontiguousarray(rerun), np.ascontiguousarray(idx, dtype=np.uint32)
    m = len(idx)
    assert out.dtype == rerun.dtype == np.dtype(A.RESULT_DTYPE) and len(rerun) == m and 3 * m < 1 << 32
    assert len(set(idx.tolist())) == m and (m == 0 or int(idx.max()) < len(out)), "indices: distinct, inside the result array"
    d_out = _guarded(out.nbytes, out)
    d_rerun = _guarded(max(rerun.nbytes, 16), rerun if m else None)
    d_idx = _guarded(max(idx.nbytes, 16), idx if m else None)
    _need(d_out, out.nbytes, "out"); _need(d_rerun, rerun.nbytes, "rerun"); _need(d_idx, idx.nbytes, "idx")
    rc = _lib().madsim_k_launch_resolve_scatter(d_out.data_ptr(), d_rerun.data_ptr(), d_idx.data_ptr(), m, _stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    _intact(d_out, out.nbytes, "out")
    if m:                                                                     # the inputs are read, never written
        assert d_rerun[:rerun.nbytes].cpu().numpy().tobytes() == rerun.tobytes() and d_idx[:idx.nbytes].cpu().numpy().tobytes() == idx.tobytes()
    return d_out[:out.nbytes].cpu().numpy().view(A.RESULT_DTYPE).copy()
