"""A direct driver for sets_mask_kernel / sets_fold_kernel / sets_extract_kernel: the launcher libmadsim_hip.so exports
(madsim_k_launch_probe_sets; csrc/sim_kernel.h) over arrays of the caller's making, with the buffers as madsim_hip_probe_sets_range hands
them over.  Test-only: tests/test_probe_sets_kernels.py feeds it synthetic rows, in both forms of the fold kernel (the in-wave combine and
one table update per seed), and holds the set words, the entries and the count words against tests/sets_ref.py.

Every buffer is checked on the host against the size the launcher demands before anything is launched; every buffer a launch writes —
sig[] included — is followed by a guard region filled with PATTERN that must come back intact, every input must come back as it went in,
and the table must be all zero again after every launch — which is why `launches` > 1 can run the same input again on the same table.
sig[] itself starts as PATTERN too: the words of rows that are not counted must still hold it afterwards."""
import ctypes as C
import os
import re

import numpy as np
import torch

from madsim_amd import _abi as A
from madsim_amd import runtime

SETS_WORDS, SLOT_BYTES, MIN_SLOTS, SETS_WAVES = 8, 48, 128, 1024
ERR_PROBE, ERR_TAG, ERR_CAP = 1, 2, 4
PATTERN, GUARD_BYTES = 0xA5, 512
PATTERN_WORD = int.from_bytes(bytes([PATTERN]) * 8, "little")
RESULT_BYTES = np.dtype(A.RESULT_DTYPE).itemsize
ENTRY_BYTES = np.dtype(A.PROBE_SET_DTYPE).itemsize


def header_constants():
    path = os.path.join(os.path.dirname(os.path.abspath(runtime.__file__)), "csrc", "sim_kernel.h")
    with open(path) as f:
        return {k: int(v) for k, v in re.findall(r"^#define\s+MADSIM_K_PROBE_SETS_(\w+)\s+(\d+)u\b", f.read(), re.M)}


assert header_constants() == {"WORDS": SETS_WORDS, "SLOT_BYTES": SLOT_BYTES, "MIN_SLOTS": MIN_SLOTS, "WAVES": SETS_WAVES, "ERR_PROBE": ERR_PROBE,
                              "ERR_TAG": ERR_TAG, "ERR_CAP": ERR_CAP}, header_constants()
assert RESULT_BYTES == 48 and ENTRY_BYTES == 72

_bound = None


def _lib():
    global _bound
    if _bound is None:
        L = runtime.lib()
        p, u64, u32 = C.c_void_p, C.c_uint64, C.c_uint32
        L.madsim_k_launch_probe_sets.argtypes = [p, u64, p, p, p, u64, u32, p, u64, p, p, u64, p, u64, p, p, p]
        L.madsim_k_launch_probe_sets.restype = C.c_int
        L.madsim_k_launch_probe_sets_form.argtypes = L.madsim_k_launch_probe_sets.argtypes + [C.c_int]
        L.madsim_k_launch_probe_sets_form.restype = C.c_int
        L.madsim_k_probe_sets_slots.argtypes, L.madsim_k_probe_sets_slots.restype = [u64], u64
        L.madsim_k_census_slot.argtypes, L.madsim_k_census_slot.restype = [u64, u64], u64
        _bound = L
    return _bound


def slots_for(cap):
    return int(_lib().madsim_k_probe_sets_slots(cap))


def slot_of(set_word, slots):
    """Where a set word starts probing: the census's hash (csrc/sim_kernel.h)."""
    return int(_lib().madsim_k_census_slot(int(set_word), slots))


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


def probe_sets(rows, lens, results, seeds, include, vocab, cap, launches=1, per_seed=False):
    """`launches` results, each (entries ndarray[A.PROBE_SET_DTYPE] sorted by set, words uint64[SETS_WORDS], sig uint64[n]), of
    madsim_k_launch_probe_sets over host arrays: rows uint64[n, obs_cap], lens uint64[n], results ndarray[A.RESULT_DTYPE], seeds uint64[n],
    vocab: the vocabulary — every launch on the SAME table, zeroed once before the first.  With a non-zero error word the entries are
    empty.  `per_seed`: one table update per counted seed in place of the in-wave combine."""
    n, obs_cap = rows.shape
    vocab = np.ascontiguousarray(np.array([int(v) for v in vocab], dtype=np.uint64))
    assert rows.dtype == np.uint64 and 1 <= n <= 1 << 31 and 1 <= obs_cap <= A.CENSUS_MAX_OBS_CAP and n * obs_cap < (1 << 32) - 1
    assert 1 <= cap <= A.PROBE_SETS_MAX and 1 <= len(vocab) <= A.PROBE_SETS_MAX_VOCAB and include and not include & ~0xf
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
        sig, lst, words, ent = _guarded(8 * n, None), _guarded(4 * cap, None), _guarded(8 * SETS_WORDS, 0), _guarded(cap * ENTRY_BYTES, None)
        _need(sig, 8 * n, "sig"); _need(lst, 4 * cap, "list"); _need(words, 8 * SETS_WORDS, "words"); _need(ent, cap * ENTRY_BYTES, "entries")
        rc = _lib().madsim_k_launch_probe_sets_form(dev[0].data_ptr(), obs_cap, dev[1].data_ptr(), dev[2].data_ptr(), dev[3].data_ptr(), n, include,
                                                    vocab.ctypes.data, len(vocab), sig.data_ptr(), table.data_ptr(), slots, lst.data_ptr(), cap,
                                                    words.data_ptr(), ent.data_ptr(), torch.cuda.current_stream().cuda_stream, 1 if per_seed else 0)
        assert rc == 0, rc
        torch.cuda.synchronize()
        for t, nb, what in ((sig, 8 * n, "sig"), (table, slots * SLOT_BYTES, "table"), (lst, 4 * cap, "list"), (words, 8 * SETS_WORDS, "words"),
                            (ent, cap * ENTRY_BYTES, "entries")):
            assert bool((t[nb:] == PATTERN).all()), f"{what}: bytes behind the buffer were written"
        assert not bool(table[:slots * SLOT_BYTES].any()), "the table is not all zero after the extract pass"
        for t, (a, nb) in zip(dev, ins):                                            # the inputs are read, never written
            assert t.cpu().numpy().tobytes() == np.ascontiguousarray(a).tobytes(), "an input array was modified"
        w = words[:8 * SETS_WORDS].cpu().numpy().view(np.uint64).copy()
        ne = 0 if w[1] else int(w[0])
        assert ne <= cap
        e = ent[:ne * ENTRY_BYTES].cpu().numpy().view(A.PROBE_SET_DTYPE).copy()
        assert bool((ent[ne * ENTRY_BYTES:cap * ENTRY_BYTES] == PATTERN).all()), "entries behind the chunk's sets were written"
        out.append((np.sort(e, order="set"), w, sig[:8 * n].cpu().numpy().view(np.uint64).copy()))
    return out
