"""A direct driver for the LIST forms of the report launchers libmadsim_hip.so exports (madsim_k_launch_summary6_list, _collect_list,
_stats_list, _groups_list, _diff_list, _resolve_list_list; csrc/sim_kernel.h): result i belongs to seed d_seeds[i].  The twin of
tests/report_kernels.py, group_kernels.py, diff_kernels.py and resolve_kernels.py — the same buffers, prepared the same way, the same guard
regions behind every written buffer, the same return shapes — so that tests/test_seedlist_kernels.py can hold a list launch and a range
launch over one array against each other byte for byte.  Test-only.

The seed list itself sits in a buffer of exactly `count` words with a guard behind it: a read past the slice would report PATTERN64 as a
seed, and the slice must come back unwritten."""
import ctypes as C

import numpy as np
import torch

from madsim_amd import _abi as A
from tests import diff_kernels as KD
from tests import group_kernels as KG
from tests import report_kernels as K
from tests import resolve_kernels as KR

PATTERN, PATTERN32, PATTERN64 = K.PATTERN, K.PATTERN32, K.PATTERN64
_bound = None


def _lib():
    global _bound
    if _bound is None:
        L = K._lib()
        p, u64, u32 = C.c_void_p, C.c_uint64, C.c_uint32
        for name, args, res in (("madsim_k_launch_summary6_list", [p, u64, p, p, p], None),
                                ("madsim_k_launch_collect_list", [p, u64, p, u32, p, p, p, u64, p], None),
                                ("madsim_k_launch_stats_list", [p, u64, p, u32, u32, p, p, p], None),
                                ("madsim_k_launch_groups_list", [p, u64, p, u32, u32, p, u64, p, p, p, p], C.c_int),
                                ("madsim_k_launch_diff_list", [p, p, u64, p, u32, p, p, p, u64, p], C.c_int),
                                ("madsim_k_launch_resolve_list_list", [p, u64, p, u32, p, p, p, p, p], C.c_int)):
            getattr(L, name).argtypes, getattr(L, name).restype = args, res
        _bound = L
    return _bound


class SeedList:
    """A strictly ascending uint64 list on the device, a guard behind its last word."""

    def __init__(self, seeds):
        self.host = np.ascontiguousarray(seeds, dtype=np.uint64)
        assert self.host.ndim == 1 and len(self.host) >= 1 and (len(self.host) < 2 or bool((self.host[:-1] < self.host[1:]).all()))
        self.n_bytes = self.host.nbytes
        self.dev = K._guarded(self.n_bytes)
        self.dev[:self.n_bytes] = torch.from_numpy(self.host.view(np.uint8).copy()).cuda()

    def ptr(self, count):
        assert count == len(self.host), (count, len(self.host))                     # the slice is the batch: never shorter
        K._need(self.dev, self.n_bytes, "seed list")
        return self.dev.data_ptr()

    def unwritten(self):
        assert self.dev[:self.n_bytes].cpu().numpy().tobytes() == self.host.tobytes(), "the seed list was written"
        K._intact(self.dev, self.n_bytes, "seed list")


def _results(d_results, count):
    assert 1 <= count < 0xffffffff
    K._need(d_results, count * K.RESULT_BYTES, "results")


def summary6(d_results, count, sl):
    """summary6_kernel<ListSeeds>'s six words."""
    _results(d_results, count)
    acc = K._guarded(48, 0)
    acc[0:8] = 0xff
    acc[32:40] = 0xff
    _lib().madsim_k_launch_summary6_list(d_results.data_ptr(), count, sl.ptr(count), acc.data_ptr(), K._stream())
    torch.cuda.synchronize()
    K._intact(acc, 48, "acc")
    sl.unwritten()
    return [int(x) for x in K._words(acc, 6)]


def collect(d_results, count, sl, list_runner, cap):
    """report_kernels.collect's (rep, wave_cnt, recs) from the list launcher."""
    _results(d_results, count)
    assert 0 <= cap <= count and list_runner in (0, 1)
    rep = K._guarded(8 * K.COLLECT_WORDS, 0)
    rep[0:8] = 0xff
    rep[32:40] = 0xff
    wave_cnt = K._guarded(4 * K.COLLECT_WAVES)
    recs = K._guarded(K.FAILURE_BYTES * cap)
    _lib().madsim_k_launch_collect_list(d_results.data_ptr(), count, sl.ptr(count), list_runner, rep.data_ptr(), wave_cnt.data_ptr(), recs.data_ptr(), cap,
                                        K._stream())
    torch.cuda.synchronize()
    K._intact(rep, 8 * K.COLLECT_WORDS, "rep"); K._intact(wave_cnt, 4 * K.COLLECT_WAVES, "wave_cnt"); K._intact(recs, K.FAILURE_BYTES * cap, "recs")
    sl.unwritten()
    return (K._words(rep, K.COLLECT_WORDS), wave_cnt[:4 * K.COLLECT_WAVES].cpu().numpy().view(np.uint32).copy(),
            recs[:K.FAILURE_BYTES * cap].cpu().numpy().view(A.FAILURE_DTYPE).copy())


def stats(d_results, count, sl, include, top_k):
    """report_kernels.stats' (srep, cand) from the list launcher."""
    _results(d_results, count)
    assert 0 < include < 16 and 0 <= top_k <= A.STAT_MAX_TOP
    srep = K._guarded(8 * K.STATS_WORDS, 0)
    if top_k == 0:
        srep[8 * K.TOP_OFF:8 * K.STATS_WORDS] = PATTERN
    cand = K._guarded(8 * K.STATS_CAND_WORDS)
    _lib().madsim_k_launch_stats_list(d_results.data_ptr(), count, sl.ptr(count), include, top_k, srep.data_ptr(), cand.data_ptr(), K._stream())
    torch.cuda.synchronize()
    K._intact(srep, 8 * K.STATS_WORDS, "srep"); K._intact(cand, 8 * K.STATS_CAND_WORDS, "cand")
    sl.unwritten()
    return K._words(srep, K.STATS_WORDS), K._words(cand, K.STATS_CAND_WORDS)


def groups(d_results, count, sl, include, key_field):
    """group_kernels.groups' (n_groups, entries in arrival order, claimed slots) from the list launcher, with its checks: the error word
    zero, nothing behind the batch's groups written, the table all zero again."""
    slots = KG.slots_for(count)
    assert 1 <= count <= KG.MAX_COUNT and 0 < include < 16 and 0 <= key_field < A.GROUP_KEYS
    _results(d_results, count)
    table = K._guarded(KG.SLOT_BYTES * slots, 0)
    lst = K._guarded(4 * count)
    grep = K._guarded(8 * KG.GROUP_WORDS, 0)
    entries = K._guarded(KG.GROUP_BYTES * count)
    rc = _lib().madsim_k_launch_groups_list(d_results.data_ptr(), count, sl.ptr(count), include, key_field, table.data_ptr(), slots, lst.data_ptr(),
                                            grep.data_ptr(), entries.data_ptr(), K._stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    for t, n, what in ((table, KG.SLOT_BYTES * slots, "table"), (lst, 4 * count, "list"), (grep, 8 * KG.GROUP_WORDS, "grep"), (entries, KG.GROUP_BYTES * count, "entries")):
        K._intact(t, n, what)
    sl.unwritten()
    words = K._words(grep, KG.GROUP_WORDS)
    n, err = int(words[0]), int(words[1])
    assert err == 0 and 0 <= n <= count, (err, n)
    assert not bool(table[:KG.SLOT_BYTES * slots].any()), "the extraction pass left a slot of the table set"
    assert bool((entries[KG.GROUP_BYTES * n:] == PATTERN).all()) and bool((lst[4 * n:] == PATTERN).all()), "something behind the batch's groups was written"
    return n, entries[:KG.GROUP_BYTES * n].cpu().numpy().view(A.GROUP_DTYPE).copy(), lst[:4 * n].cpu().numpy().view(np.uint32).copy()


def diff(d_a, d_b, count, sl, fields, cap):
    """diff_kernels.diff's (words, wave counts of the grid, records) from the list launcher."""
    assert 1 <= count < 1 << 32 and 0 < fields <= A.DIFF_ALL and 0 <= cap
    room = min(cap, count)
    _results(d_a, count); _results(d_b, count)
    words = K._guarded(8 * KD.DIFF_WORDS, 0)
    wcnt = K._guarded(4 * KD.WAVES)
    recs = K._guarded(KD.RECORD_BYTES * room)
    rc = _lib().madsim_k_launch_diff_list(d_a.data_ptr(), d_b.data_ptr(), count, sl.ptr(count), fields, words.data_ptr(), wcnt.data_ptr(),
                                          recs.data_ptr() if room else None, room, K._stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    K._intact(words, 8 * KD.DIFF_WORDS, "words"); K._intact(wcnt, 4 * KD.WAVES, "wave counts"); K._intact(recs, KD.RECORD_BYTES * room, "records")
    sl.unwritten()
    w = K._words(words, KD.DIFF_WORDS)
    n_waves = 4 * max(1, min(256, (count + 1023) // 1024))
    assert bool((wcnt[4 * n_waves:] == PATTERN).all()), "wave counts behind the grid's waves were written"
    n = min(room, int(w[0]))
    assert int(w[0]) <= count and bool((recs[KD.RECORD_BYTES * n:] == PATTERN).all()), "record bytes behind the batch's list were written"
    return w, wcnt[:4 * n_waves].cpu().numpy().view(np.uint32).copy(), recs[:KD.RECORD_BYTES * n].cpu().numpy().view(A.DIFF_RECORD_DTYPE).copy()


def resolve_list(d_results, count, sl, steps_maxed):
    """resolve_kernels.resolve_list's (m, seeds, idx) from the list launcher: the seed list read, the compacted list written — two buffers."""
    assert 1 <= count < 1 << 32 and steps_maxed in (0, 1)
    _results(d_results, count)
    wave_cnt, total, seeds, idx = KR._guarded(4 * KR.RESOLVE_WAVES), KR._guarded(4), KR._guarded(8 * count), KR._guarded(4 * count)
    rc = _lib().madsim_k_launch_resolve_list_list(d_results.data_ptr(), count, sl.ptr(count), steps_maxed, wave_cnt.data_ptr(), total.data_ptr(),
                                                  seeds.data_ptr(), idx.data_ptr(), K._stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    KR._intact(wave_cnt, 4 * KR.RESOLVE_WAVES, "wave_cnt"); KR._intact(total, 4, "total")
    sl.unwritten()
    m = int(total[:4].cpu().numpy().view(np.uint32)[0])
    assert 0 <= m <= count, m
    KR._intact(seeds, 8 * m, "seeds"); KR._intact(idx, 4 * m, "idx")
    waves = 4 * min((count + 1023) // 1024, 256)
    cnt = wave_cnt[:4 * KR.RESOLVE_WAVES].cpu().numpy().view(np.uint32)
    assert int(cnt[:waves].sum()) == m and (cnt[waves:] == PATTERN32).all()
    return m, seeds[:8 * m].cpu().numpy().view(np.uint64).copy(), idx[:4 * m].cpu().numpy().view(np.uint32).copy()
