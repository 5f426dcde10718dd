"""A direct driver for census_fold_kernel / census_extract_kernel: the launcher libmadsim_hip.so exports (madsim_k_launch_census;
csrc/sim_kernel.h) over arrays of the caller's making, with the buffers as madsim_hip_census_range hands them over.  Test-only:
tests/test_census_kernels.py feeds it synthetic rows, in both forms of the fold kernel (the wave accumulator and the direct form), and
holds the entries and the count words against tests/census_ref.py.

Every buffer is checked on the host against the size the launcher demands before anything is launched; every buffer a launch writes is
followed by a guard region filled with PATTERN that must come back intact, every input must come back as it went in, and the table must
be all zero again after every launch — which is why `launches` > 1 can run the same input again on the same table."""
import ctypes as C
import os
import re

import numpy as np
import torch

from madsim_amd import _abi as A
from madsim_amd import runtime

CENSUS_WORDS, SLOT_BYTES, MIN_SLOTS, CENSUS_WAVES = 16, 32, 128, 1024
ERR_PROBE, ERR_TAG, ERR_CAP = 1, 2, 4
PATTERN, GUARD_BYTES = 0xA5, 512
RESULT_BYTES = np.dtype(A.RESULT_DTYPE).itemsize
ENTRY_BYTES = np.dtype(A.CENSUS_VALUE_DTYPE).itemsize


def header_constants():
    path = os.path.join(os.path.dirname(os.path.abspath(runtime.__file__)), "csrc", "sim_kernel.h")
    with open(path) as f:
        return {k: int(v) for k, v in re.findall(r"^#define\s+MADSIM_K_CENSUS_(\w+)\s+(\d+)u\b", f.read(), re.M)}


assert header_constants() == {"WORDS": CENSUS_WORDS, "SLOT_BYTES": SLOT_BYTES, "MIN_SLOTS": MIN_SLOTS, "WAVES": CENSUS_WAVES, "ERR_PROBE": ERR_PROBE,
                              "ERR_TAG": ERR_TAG, "ERR_CAP": ERR_CAP}, header_constants()
assert RESULT_BYTES == 48 and ENTRY_BYTES == 64

_bound = None


def _lib():
    global _bound
    if _bound is None:
        L = runtime.lib()
        p, u64, u32 = C.c_void_p, C.c_uint64, C.c_uint32
        L.madsim_k_launch_census.argtypes = [p, u64, p, p, p, u64, u32, p, u64, p, u64, p, p, p]
        L.madsim_k_launch_census.restype = C.c_int
        L.madsim_k_launch_census_form.argtypes = L.madsim_k_launch_census.argtypes + [C.c_int]
        L.madsim_k_launch_census_form.restype = C.c_int
        L.madsim_k_census_slots.argtypes, L.madsim_k_census_slots.restype = [u64], u64
        L.madsim_k_census_slot.argtypes, L.madsim_k_census_slot.restype = [u64, u64], u64
        _bound = L
    return _bound


def slots_for(cap):
    return int(_lib().madsim_k_census_slots(cap))


def slot_of(value, slots):
    return int(_lib().madsim_k_census_slot(int(value), slots))


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


def census(rows, lens, results, seeds, include, cap, launches=1, direct=False):
    """`launches` results, each (entries ndarray[A.CENSUS_VALUE_DTYPE] sorted by value, words uint64[CENSUS_WORDS]), of madsim_k_launch_census
    over host arrays: rows uint64[n, obs_cap], lens uint64[n], results ndarray[A.RESULT_DTYPE], seeds uint64[n] — every launch on the SAME
    table, zeroed once before the first.  With a non-zero error word the entries are empty.  `direct`: the fold kernel's direct form (one
    table update per row and distinct value) in place of the wave accumulator."""
    n, obs_cap = rows.shape
    assert rows.dtype == np.uint64 and 1 <= n and 1 <= obs_cap <= A.CENSUS_MAX_OBS_CAP and n * obs_cap < (1 << 32) - 1 and 1 <= cap <= A.CENSUS_MAX_VALUES
    slots = slots_for(cap)
    assert slots >= max(2 * cap, MIN_SLOTS) and slots & (slots - 1) == 0
    ins = [(rows, 8 * n * obs_cap), (np.asarray(lens, dtype=np.uint64), 8 * n), (results, n * RESULT_BYTES), (np.asarray(seeds, dtype=np.uint64), 8 * n)]
    dev = [_upload(a, nb) for a, nb in ins]
    for t, (a, nb) in zip(dev, ins):
        _need(t, nb, "input")
    table = _guarded(slots * SLOT_BYTES, 0)
    _need(table, slots * SLOT_BYTES, "table")
    out = []
    for _ in range(launches):
        lst, words, ent = _guarded(4 * cap, None), _guarded(8 * CENSUS_WORDS, 0), _guarded(cap * ENTRY_BYTES, None)
        _need(lst, 4 * cap, "list"); _need(words, 8 * CENSUS_WORDS, "words"); _need(ent, cap * ENTRY_BYTES, "entries")
        rc = _lib().madsim_k_launch_census_form(dev[0].data_ptr(), obs_cap, dev[1].data_ptr(), dev[2].data_ptr(), dev[3].data_ptr(), n, include,
                                                table.data_ptr(), slots, lst.data_ptr(), cap, words.data_ptr(), ent.data_ptr(),
                                                torch.cuda.current_stream().cuda_stream, 1 if direct else 0)
        assert rc == 0, rc
        torch.cuda.synchronize()
        for t, nb, what in ((table, slots * SLOT_BYTES, "table"), (lst, 4 * cap, "list"), (words, 8 * CENSUS_WORDS, "words"), (ent, cap * ENTRY_BYTES, "entries")):
            assert bool((t[nb:] == PATTERN).all()), f"{what}: bytes behind the buffer were written"
        assert not bool(table[:slots * SLOT_BYTES].any()), "the table is not all zero after the extract pass"
        for t, (a, nb) in zip(dev, ins):                                            # the inputs are read, never written
            assert t.cpu().numpy().tobytes() == np.ascontiguousarray(a).tobytes(), "an input array was modified"
        w = words[:8 * CENSUS_WORDS].cpu().numpy().view(np.uint64).copy()
        nv = 0 if w[1] else int(w[0])
        assert nv <= cap
        e = ent[:nv * ENTRY_BYTES].cpu().numpy().view(A.CENSUS_VALUE_DTYPE).copy()
        assert bool((ent[nv * ENTRY_BYTES:cap * ENTRY_BYTES] == PATTERN).all()), "entries behind the chunk's values were written"
        out.append((np.sort(e, order="value"), w))
    return out
