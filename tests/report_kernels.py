"""A direct driver for the campaign report kernels: the launchers libmadsim_hip.so exports (madsim_k_launch_summary, _summary6, _collect,
_stats; csrc/sim_kernel.h) over a madsim_result_t array of the caller's making, with the buffers prepared as run_campaign_impl's `queue`
prepares them.  Test-only: tests/test_report_kernels.py feeds it synthetic arrays and holds the words against tests/report_ref.py.

Every buffer is checked on the host against the size the launcher demands before anything is launched, and every buffer a launch writes
is followed by a guard region filled with PATTERN that must come back intact (so are the parts inside a buffer that a launch must leave
alone: records from `cap` on, wave counts beyond the grid, candidate lists of workgroups that do not run, and — with top_k == 0, when the
campaign does not even clear them — the candidate array and the top words as a whole)."""
import ctypes as C
import os
import re

import numpy as np
import torch

from madsim_amd import _abi as A
from madsim_amd import runtime
from tests import stats_ref as R

COLLECT_WORDS, COLLECT_WAVES, STATS_WORDS, STATS_CAND_WORDS = 15, 1024, 657, 32768
TOP_OFF = 17 + A.STAT_METRICS * A.STAT_BUCKETS // 2
PATTERN, GUARD_BYTES = 0xA5, 512
PATTERN64, PATTERN32 = 0xA5A5A5A5A5A5A5A5, 0xA5A5A5A5
RESULT_BYTES, FAILURE_BYTES = np.dtype(A.RESULT_DTYPE).itemsize, np.dtype(A.FAILURE_DTYPE).itemsize


def header_constants():
    """The MADSIM_K_* sizes as csrc/sim_kernel.h states them."""
    path = os.path.join(os.path.dirname(os.path.abspath(runtime.__file__)), "csrc", "sim_kernel.h")
    with open(path) as f:
        return {k: int(v) for k, v in re.findall(r"^#define\s+MADSIM_K_(\w+)\s+(\d+)u\s*$", f.read(), re.M)}


assert header_constants() == {"COLLECT_WORDS": COLLECT_WORDS, "COLLECT_WAVES": COLLECT_WAVES, "STATS_WORDS": STATS_WORDS,
                              "STATS_CAND_WORDS": STATS_CAND_WORDS}, header_constants()
assert STATS_WORDS == TOP_OFF + 2 * A.STAT_METRICS * A.STAT_MAX_TOP and STATS_CAND_WORDS == A.STAT_METRICS * (COLLECT_WAVES // 4) * A.STAT_MAX_TOP * 2
assert (RESULT_BYTES, FAILURE_BYTES) == (48, 56)

_bound = None


def _lib():
    global _bound
    if _bound is None:
        L = runtime.lib()
        p, u64, u32 = C.c_void_p, C.c_uint64, C.c_uint32
        for name, args in (("madsim_k_launch_summary", [p, u64, u64, p, p]), ("madsim_k_launch_summary6", [p, u64, u64, p, p]),
                           ("madsim_k_launch_collect", [p, u64, u64, u32, p, p, p, u64, p]),
                           ("madsim_k_launch_stats", [p, u64, u64, u32, u32, p, p, p])):
            getattr(L, name).argtypes, getattr(L, name).restype = args, None
        _bound = L
    return _bound


def upload(results):
    """A numpy array of A.RESULT_DTYPE as a uint8 tensor on the device."""
    results = np.ascontiguousarray(results)
    assert results.dtype == np.dtype(A.RESULT_DTYPE) and results.ndim == 1
    return torch.from_numpy(results.view(np.uint8).copy()).cuda()


def _guarded(n_bytes, fill=None):
    """A uint8 device tensor of n_bytes + GUARD_BYTES, all PATTERN but the first n_bytes when `fill` (a byte value) is given."""
    t = torch.full((n_bytes + GUARD_BYTES,), PATTERN, dtype=torch.uint8, device="cuda")
    if fill is not None:
        t[:n_bytes] = fill
    return t


def _need(t, n_bytes, what):
    assert t.is_cuda and t.is_contiguous() and t.dtype == torch.uint8 and t.data_ptr() % 16 == 0, what
    assert t.numel() >= n_bytes, (what, t.numel(), n_bytes)


def _batch(d_results, count, seed0):
    assert 1 <= count < 0xffffffff and 0 <= seed0 and seed0 + count <= 1 << 64, (count, seed0)
    _need(d_results, count * RESULT_BYTES, "results")


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _intact(t, n_bytes, what):
    assert bool((t[n_bytes:] == PATTERN).all()), f"{what}: the guard behind the buffer was written"


def _words(t, n_words):
    return t[:8 * n_words].cpu().numpy().view(np.uint64).copy()


def _summary(fn, n_words, d_results, count, seed0):
    _batch(d_results, count, seed0)
    acc = _guarded(8 * n_words, 0)
    acc[0:8] = 0xff                                            # the first failing seed: a minimum
    if n_words == 6:
        acc[32:40] = 0xff
    _need(acc, 8 * n_words, "acc")
    fn(d_results.data_ptr(), count, seed0, acc.data_ptr(), _stream())
    torch.cuda.synchronize()
    _intact(acc, 8 * n_words, "acc")
    return [int(x) for x in _words(acc, n_words)]


def summary(d_results, count, seed0):
    """summary_kernel's four words."""
    return _summary(_lib().madsim_k_launch_summary, 4, d_results, count, seed0)


def summary6(d_results, count, seed0):
    """summary6_kernel's six words."""
    return _summary(_lib().madsim_k_launch_summary6, 6, d_results, count, seed0)


def collect(d_results, count, seed0, list_runner, cap):
    """(rep: uint64[15], wave_cnt: uint32[1024] — PATTERN32 where no wave wrote —, recs: FAILURE_DTYPE[cap] — PATTERN bytes where no
    record was written) of collect_count_kernel + collect_write_kernel on freshly prepared buffers."""
    _batch(d_results, count, seed0)
    assert 0 <= cap <= count and list_runner in (0, 1)
    rep = _guarded(8 * COLLECT_WORDS, 0)
    rep[0:8] = 0xff
    rep[32:40] = 0xff
    wave_cnt = _guarded(4 * COLLECT_WAVES)                     # scratch the campaign does not prepare
    recs = _guarded(FAILURE_BYTES * cap)                       # (so cap == 0 hands the kernels a guard and nothing else)
    _need(rep, 8 * COLLECT_WORDS, "rep"); _need(wave_cnt, 4 * COLLECT_WAVES, "wave_cnt"); _need(recs, FAILURE_BYTES * cap, "recs")
    _lib().madsim_k_launch_collect(d_results.data_ptr(), count, seed0, list_runner, rep.data_ptr(), wave_cnt.data_ptr(), recs.data_ptr(), cap, _stream())
    torch.cuda.synchronize()
    _intact(rep, 8 * COLLECT_WORDS, "rep"); _intact(wave_cnt, 4 * COLLECT_WAVES, "wave_cnt"); _intact(recs, FAILURE_BYTES * cap, "recs")
    return (_words(rep, COLLECT_WORDS), wave_cnt[:4 * COLLECT_WAVES].cpu().numpy().view(np.uint32).copy(),
            recs[:FAILURE_BYTES * cap].cpu().numpy().view(A.FAILURE_DTYPE).copy())


def stats(d_results, count, seed0, include, top_k):
    """(srep: uint64[657], cand: uint64[32768]) of stats_fold_kernel + stats_top_kernel on freshly prepared buffers: srep all zero — but
    its top words PATTERN64 when top_k == 0, which the campaign then neither clears nor reads —, cand PATTERN64 where no workgroup wrote."""
    _batch(d_results, count, seed0)
    assert 0 < include < 16 and 0 <= top_k <= A.STAT_MAX_TOP
    srep = _guarded(8 * STATS_WORDS, 0)
    if top_k == 0:
        srep[8 * TOP_OFF:8 * STATS_WORDS] = PATTERN
    cand = _guarded(8 * STATS_CAND_WORDS)
    _need(srep, 8 * STATS_WORDS, "srep"); _need(cand, 8 * STATS_CAND_WORDS, "cand")
    _lib().madsim_k_launch_stats(d_results.data_ptr(), count, seed0, include, top_k, srep.data_ptr(), cand.data_ptr(), _stream())
    torch.cuda.synchronize()
    _intact(srep, 8 * STATS_WORDS, "srep"); _intact(cand, 8 * STATS_CAND_WORDS, "cand")
    return _words(srep, STATS_WORDS), _words(cand, STATS_CAND_WORDS)


def fold(batches, top_k, include=1):
    """madsim_k_fold_stats (the host fold of madsim_hip.cpp: no device involved) over the batches' 657 words, in the order given, from the
    state run_campaign_impl starts with — every minimum all-ones, the rest zero; the answer in the shape of stats_ref.stats_truth's."""
    L = runtime.lib()
    L.madsim_k_fold_stats.argtypes, L.madsim_k_fold_stats.restype = [C.POINTER(A.Stats), C.c_void_p], None
    assert 0 <= top_k <= A.STAT_MAX_TOP
    st = A.Stats()
    st.include, st.top_k = include, top_k
    top = np.zeros((A.STAT_METRICS, top_k), dtype=A.EXTREME_DTYPE)
    st.top = top.ctypes.data_as(C.POINTER(A.Extreme)) if top_k else None
    for m in range(A.STAT_METRICS):
        st.metric[m].min = (1 << 64) - 1
    for w in batches:
        w = np.ascontiguousarray(w, dtype=np.uint64)
        assert w.shape == (STATS_WORDS,)
        L.madsim_k_fold_stats(C.byref(st), w.ctypes.data)
    return R.of_stats(runtime.CampaignStats(st, top))
