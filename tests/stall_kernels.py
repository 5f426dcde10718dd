"""A direct driver for stall_sites_kernel: the launcher libmadsim_hip.so exports (madsim_k_launch_stall_sites; csrc/sim_kernel.h) over arrays
of the caller's making, with the buffers as madsim_hip_stall_census_range hands them over — and, behind it, the observation census's own
launcher (tests/census_kernels.py) over what the kernel wrote: the site pass and the shape pass of a chunk.  Test-only:
tests/test_stall_kernels.py feeds it synthetic rows and holds everything against tests/stall_ref.py.

Every buffer is checked on the host against the size the launcher demands before anything is launched; every buffer the launch writes is
followed by a guard region filled with PATTERN that must come back intact, and every input must come back as it went in.  (The census
driver checks the same of its launches, and its table all zero afterwards.)"""
import ctypes as C

import numpy as np
import torch

from madsim_amd import _abi as A
from madsim_amd import runtime
from tests import census_kernels as CK

PATTERN, GUARD_BYTES = CK.PATTERN, CK.GUARD_BYTES
RESULT_BYTES = CK.RESULT_BYTES

_bound = None


def _lib():
    global _bound
    if _bound is None:
        L = runtime.lib()
        p, u64 = C.c_void_p, C.c_uint64
        L.madsim_k_launch_stall_sites.argtypes = [p, u64, p, p, u64, p, p, p, p]
        L.madsim_k_launch_stall_sites.restype = C.c_int
        _bound = L
    return _bound


def refused(task_cap, n):
    """The launcher's answer for sizes it is not written for, with null arrays: nothing is launched either way."""
    return _lib().madsim_k_launch_stall_sites(None, task_cap, None, None, n, None, None, None, None)


def sites(rows, lens, results):
    """(site rows uint64[n, task_cap], shape words uint64[n], ones uint64[n]) of madsim_k_launch_stall_sites over host arrays: rows
    uint64[n, task_cap], lens uint64[n] (the true counts), results ndarray[A.RESULT_DTYPE]."""
    n, task_cap = rows.shape
    assert rows.dtype == np.uint64 and 1 <= n and 1 <= task_cap <= A.MAX_LIVE_TASKS and n * task_cap < (1 << 32) - 1
    ins = [(rows, 8 * n * task_cap), (np.asarray(lens, dtype=np.uint64), 8 * n), (results, n * RESULT_BYTES)]
    dev = [CK._upload(a, nb) for a, nb in ins]
    for t, (a, nb) in zip(dev, ins):
        CK._need(t, nb, "input")
    outs = [(CK._guarded(8 * n * task_cap, None), 8 * n * task_cap, "site rows"), (CK._guarded(8 * n, None), 8 * n, "shape words"),
            (CK._guarded(8 * n, None), 8 * n, "ones")]
    for t, nb, what in outs:
        CK._need(t, nb, what)
    rc = _lib().madsim_k_launch_stall_sites(dev[0].data_ptr(), task_cap, dev[1].data_ptr(), dev[2].data_ptr(), n, outs[0][0].data_ptr(),
                                            outs[1][0].data_ptr(), outs[2][0].data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert rc == 0, rc
    torch.cuda.synchronize()
    for t, nb, what in outs:
        assert bool((t[nb:] == PATTERN).all()), f"{what}: bytes behind the buffer were written"
    for t, (a, nb) in zip(dev, ins):                                                # the inputs are read, never written
        assert t.cpu().numpy().tobytes() == np.ascontiguousarray(a).tobytes(), "an input array was modified"
    got = [t[:nb].cpu().numpy().view(np.uint64).copy() for t, nb, _ in outs]
    return got[0].reshape(n, task_cap), got[1], got[2]


def census(rows, lens, results, seeds, include, site_cap, shape_cap, launches=1):
    """A chunk of the stall census as the host queues it: stall_sites_kernel, then the census launcher over the site rows (under the true
    counts) and over the shape words (rows of cap 1 under the ones).  Returns (`launches` site-pass results, `launches` shape-pass
    results), each as tests/census_kernels.census gives them: (entries sorted by value, words)."""
    srows, shp, ones = sites(rows, lens, results)
    a = CK.census(srows, lens, results, seeds, include, site_cap, launches=launches)
    b = CK.census(shp.reshape(-1, 1).copy(), ones, results, seeds, include, shape_cap, launches=launches)
    return a, b
