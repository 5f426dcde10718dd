"""A direct driver for the sweep campaign's report kernels: the launchers libmadsim_hip.so exports (madsim_k_launch_sweep and its _list
form; csrc/sim_kernel.h) over V madsim_result_t arrays of the caller's making, with the buffers prepared as run_variants_impl prepares
them.  Test-only: tests/test_sweep_kernels.py feeds it synthetic arrays and holds every word, record and wave count against tests/sweep_ref.py.

Every buffer is checked on the host against the size the launcher demands before anything is launched; every buffer a launch writes is
followed by a guard region filled with PATTERN that must come back intact, and so must the record bytes behind the batch's list."""
import ctypes as C
import os
import re

import numpy as np
import torch

from madsim_amd import _abi as A
from madsim_amd import runtime
from tests.diff_kernels import GUARD_BYTES, PATTERN, _guarded, _need, upload  # noqa: F401  (upload: re-exported)

SWEEP_WORDS, WAVES = 274, 1024
RESULT_BYTES, RECORD_BYTES = np.dtype(A.RESULT_DTYPE).itemsize, np.dtype(A.SWEEP_RECORD_DTYPE).itemsize


def header_constants():
    """MADSIM_K_SWEEP_WORDS and MADSIM_K_COLLECT_WAVES as csrc/sim_kernel.h states them."""
    path = os.path.join(os.path.dirname(os.path.abspath(runtime.__file__)), "csrc", "sim_kernel.h")
    with open(path) as f:
        return {k: int(v) for k, v in re.findall(r"^#define\s+MADSIM_K_(SWEEP_WORDS|COLLECT_WAVES)\s+(\d+)u\b", f.read(), re.M)}


assert header_constants() == {"SWEEP_WORDS": SWEEP_WORDS, "COLLECT_WAVES": WAVES}, header_constants()
assert (RESULT_BYTES, RECORD_BYTES) == (48, 24)

_bound = None


def _lib():
    global _bound
    if _bound is None:
        L = runtime.lib()
        p, u64, u32 = C.c_void_p, C.c_uint64, C.c_uint32
        L.madsim_k_launch_sweep.argtypes, L.madsim_k_launch_sweep.restype = [p, u32, u64, u64, u32, u32, p, p, p, u64, p], C.c_int
        L.madsim_k_launch_sweep_list.argtypes, L.madsim_k_launch_sweep_list.restype = [p, u32, u64, p, u32, u32, p, p, p, u64, p], C.c_int
        _bound = L
    return _bound


def upload_seeds(seeds):
    """A strictly ascending uint64 array as a uint8 tensor on the device (the batch's slice of a seed list)."""
    seeds = np.ascontiguousarray(seeds, dtype=np.uint64)
    return torch.from_numpy(seeds.view(np.uint8).copy()).cuda()


def side_table(d_sides):
    """The host array of device pointers the launchers take."""
    return (C.c_void_p * len(d_sides))(*[t.data_ptr() for t in d_sides])


def sweep(d_sides, count, seeds, fields, rule, cap):
    """(words: uint64[SWEEP_WORDS], wave counts: uint32[waves of the grid], records: ndarray[SWEEP_RECORD_DTYPE] of min(cap, n_selected)) of
    sweep_count_kernel + sweep_write_kernel on freshly prepared buffers.  `seeds`: an int (seed0 of a range) or a device tensor from
    upload_seeds (the list form).  Asserts the guards intact, the wave counts behind the grid's waves untouched and the record bytes behind
    the batch's list untouched."""
    V = len(d_sides)
    assert 2 <= V <= 8 and 1 <= count < 1 << 32 and 0 <= fields <= A.DIFF_ALL and rule in (0, 1, 2) and (rule != 2 or fields) and 0 <= cap
    room = min(cap, count)                                     # what the campaign gives a batch: no batch lists more
    for v, t in enumerate(d_sides):
        _need(t, count * RESULT_BYTES, f"variant {v}")
    words = _guarded(8 * SWEEP_WORDS, 0)
    wcnt = _guarded(4 * WAVES)                                 # scratch the campaign does not prepare
    recs = _guarded(RECORD_BYTES * room)
    _need(words, 8 * SWEEP_WORDS, "words"); _need(wcnt, 4 * WAVES, "wave counts"); _need(recs, RECORD_BYTES * room, "records")
    stream = torch.cuda.current_stream().cuda_stream
    if isinstance(seeds, int):
        assert 0 <= seeds and seeds + count <= 1 << 64, (count, seeds)
        rc = _lib().madsim_k_launch_sweep(side_table(d_sides), V, count, seeds, fields, rule, words.data_ptr(), wcnt.data_ptr(),
                                          recs.data_ptr() if room else None, room, stream)
    else:
        _need(seeds, 8 * count, "seed list")
        rc = _lib().madsim_k_launch_sweep_list(side_table(d_sides), V, count, seeds.data_ptr(), fields, rule, words.data_ptr(), wcnt.data_ptr(),
                                               recs.data_ptr() if room else None, room, stream)
    assert rc == 0, rc
    torch.cuda.synchronize()
    for t, n, what in ((words, 8 * SWEEP_WORDS, "words"), (wcnt, 4 * WAVES, "wave counts"), (recs, RECORD_BYTES * room, "records")):
        assert bool((t[n:] == PATTERN).all()), f"{what}: the guard behind the buffer was written"
    w = words[:8 * SWEEP_WORDS].cpu().numpy().view(np.uint64).copy()
    n_waves = 4 * max(1, min(256, (count + 1023) // 1024))
    assert bool((wcnt[4 * n_waves:] == PATTERN).all()), "wave counts behind the grid's waves were written"
    waves = wcnt[:4 * n_waves].cpu().numpy().view(np.uint32).copy()
    assert int(w[0]) <= count
    n = min(room, int(w[0]))
    assert bool((recs[RECORD_BYTES * n:] == PATTERN).all()), "record bytes behind the batch's list were written"
    got = recs[:RECORD_BYTES * n].cpu().numpy().view(A.SWEEP_RECORD_DTYPE).copy()
    return w, waves, got
