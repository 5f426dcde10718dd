"""A direct driver for the grouping campaign's report kernels: the launcher libmadsim_hip.so exports (madsim_k_launch_groups;
csrc/sim_kernel.h) over a madsim_result_t array of the caller's making, with the buffers prepared as run_campaign_impl prepares them.
Test-only: tests/test_group_kernels.py feeds it synthetic arrays and holds the entries against tests/groups_ref.py.

Every buffer is checked on the host against the size the launcher demands before anything is launched; every buffer a launch writes is
followed by a guard region filled with PATTERN that must come back intact, and so must the part of the entry buffer and of the slot list
behind the batch's groups.  The table — all zero going in — must be all zero again after the extraction pass."""
import ctypes as C
import os
import re

import numpy as np
import torch

from madsim_amd import _abi as A
from madsim_amd import runtime

GROUP_WORDS, SLOT_BYTES, MIN_SLOTS, MAX_COUNT = 2, 16, 128, 1 << 20
PATTERN, GUARD_BYTES = 0xA5, 512
RESULT_BYTES, GROUP_BYTES = np.dtype(A.RESULT_DTYPE).itemsize, np.dtype(A.GROUP_DTYPE).itemsize


def header_constants():
    """The MADSIM_K_GROUP_* sizes as csrc/sim_kernel.h states them."""
    path = os.path.join(os.path.dirname(os.path.abspath(runtime.__file__)), "csrc", "sim_kernel.h")
    with open(path) as f:
        return {k: int(v) for k, v in re.findall(r"^#define\s+MADSIM_K_GROUP_(\w+)\s+(\d+)u\b", f.read(), re.M)}


assert header_constants() == {"WORDS": GROUP_WORDS, "SLOT_BYTES": SLOT_BYTES, "MIN_SLOTS": MIN_SLOTS, "MAX_COUNT": MAX_COUNT}, header_constants()
assert (RESULT_BYTES, GROUP_BYTES) == (48, 32) and MAX_COUNT == A.GROUP_MAX_BATCH

_bound = None


def _lib():
    global _bound
    if _bound is None:
        L = runtime.lib()
        p, u64, u32 = C.c_void_p, C.c_uint64, C.c_uint32
        L.madsim_k_launch_groups.argtypes, L.madsim_k_launch_groups.restype = [p, u64, u64, u32, u32, p, u64, p, p, p, p], C.c_int
        L.madsim_k_group_slot.argtypes, L.madsim_k_group_slot.restype = [u64, u32, u64], u64
        L.madsim_k_group_slots.argtypes, L.madsim_k_group_slots.restype = [u64], u64
        _bound = L
    return _bound


def slots_for(count):
    """The table the campaign gives a batch of `count` seeds: a power of two, at least twice the batch."""
    s = int(_lib().madsim_k_group_slots(count))
    assert s >= max(2 * count, MIN_SLOTS) and s & (s - 1) == 0 and (s == MIN_SLOTS or s < 4 * count)
    return s


def slot_of(key, verdict, slots):
    """Where (key, verdict) starts probing."""
    return int(_lib().madsim_k_group_slot(key, verdict, slots))


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


def groups(d_results, count, seed0, include, key_field, slots=None):
    """(n_groups, entries: ndarray[GROUP_DTYPE] of n_groups in arrival order, slot list: uint32[n_groups]) of group_fold_kernel +
    group_extract_kernel on freshly prepared buffers.  Asserts the error word zero, the guards intact, whatever lies behind the batch's
    groups in the entry buffer and the list untouched, and the table all zero again."""
    slots = slots_for(count) if slots is None else slots
    assert 1 <= count <= MAX_COUNT and 0 <= seed0 and seed0 + count <= 1 << 64, (count, seed0)
    assert 0 < include < 16 and 0 <= key_field < A.GROUP_KEYS
    assert slots & (slots - 1) == 0 and slots >= max(2 * count, MIN_SLOTS) and slots <= 1 << 31
    _need(d_results, count * RESULT_BYTES, "results")
    table = _guarded(SLOT_BYTES * slots, 0)
    lst = _guarded(4 * count)                                  # scratch the campaign does not prepare
    grep = _guarded(8 * GROUP_WORDS, 0)
    entries = _guarded(GROUP_BYTES * count)
    _need(table, SLOT_BYTES * slots, "table"); _need(lst, 4 * count, "list"); _need(grep, 8 * GROUP_WORDS, "grep"); _need(entries, GROUP_BYTES * count, "entries")
    rc = _lib().madsim_k_launch_groups(d_results.data_ptr(), count, seed0, include, key_field, table.data_ptr(), slots, lst.data_ptr(), grep.data_ptr(),
                                       entries.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert rc == 0, rc
    torch.cuda.synchronize()
    for t, n, what in ((table, SLOT_BYTES * slots, "table"), (lst, 4 * count, "list"), (grep, 8 * GROUP_WORDS, "grep"), (entries, GROUP_BYTES * count, "entries")):
        assert bool((t[n:] == PATTERN).all()), f"{what}: the guard behind the buffer was written"
    words = grep[:8 * GROUP_WORDS].cpu().numpy().view(np.uint64)
    n, err = int(words[0]), int(words[1])
    assert err == 0, f"error word {err}"
    assert 0 <= n <= count
    assert not bool(table[:SLOT_BYTES * slots].any()), "the extraction pass left a slot of the table set"
    assert bool((entries[GROUP_BYTES * n:] == PATTERN).all()), "entries behind the batch's groups were written"
    assert bool((lst[4 * n:] == PATTERN).all()), "list words behind the batch's groups were written"
    got = entries[:GROUP_BYTES * n].cpu().numpy().view(A.GROUP_DTYPE).copy()
    claimed = lst[:4 * n].cpu().numpy().view(np.uint32).copy()
    assert len(set(claimed.tolist())) == n and (claimed < slots).all()
    return n, got, claimed


def by_first_seed(entries):
    """Entries as [(verdict, key, count, first_seed)], sorted by first_seed — arrival order is not part of the answer."""
    assert (entries["reserved"] == 0).all()
    out = sorted(((int(g["verdict"]), int(g["key"]), int(g["count"]), int(g["first_seed"])) for g in entries), key=lambda g: g[3])
    return out
