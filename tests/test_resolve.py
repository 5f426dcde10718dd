"""Self-resolving campaigns (MADSIM_CAMPAIGN_RESOLVE) at the C-ABI boundary, without a GPU: the new struct and defines against the header
and the ctypes mirror, the three new exports, the fifteen campaign signatures as they were, madsim_hip_grow_limits against a table written
out here, the argument errors that need no device, and the loud failure of a valid resolving call on a host without one.  What a
resolving campaign reports is tests/test_campaign_resolve_gpu.py's business."""
import ctypes as C
import inspect

import pytest

from madsim_amd import _abi as A
from madsim_amd import runtime, workload
from tests import cheader as H

E_ARG, E_HIP, E_NOINIT = -1, -2, -3
RESOLVE9 = A.CAMPAIGN_RESOLVE | 9 << A.CAMPAIGN_RESOLVE_ROUNDS_SHIFT


def _no_gpu():
    import torch
    return not torch.cuda.is_available()


def test_struct_and_defines_match_the_header():
    S = H.structs()
    fields = S["madsim_resolve_t"]
    assert [(f[0], f[1], f[2]) for f in fields] == [
        ("n_first_pass", "uint64_t", 0), ("n_resolved", "uint64_t", 0), ("n_unresolved", "uint64_t", 0), ("n_by_round", "uint64_t", 8),
        ("batches_resolved", "uint64_t", 0), ("rounds", "uint32_t", 0), ("reserved", "uint32_t", 0), ("rerun_kernel_ms", "double", 0)]
    offs, size = H.layout(fields)
    assert size == 112 == C.sizeof(A.Resolve) and A.HEADER_STRUCTS["madsim_resolve_t"] is A.Resolve
    assert [f[0] for f in A.Resolve._fields_] == [f[0] for f in fields]
    for fname, _, _, _ in fields:
        assert getattr(A.Resolve, fname).offset == offs[fname], fname
    D = {k: int(v.rstrip("u"), 0) for k, v in H.defines().items() if "RESOLVE" in k}
    assert D == {"MADSIM_CAMPAIGN_RESOLVE": 32, "MADSIM_CAMPAIGN_RESOLVE_ROUNDS_SHIFT": 8, "MADSIM_CAMPAIGN_RESOLVE_ROUNDS_MASK": 0xF00,
                 "MADSIM_RESOLVE_DEFAULT_ROUNDS": 4, "MADSIM_RESOLVE_MAX_ROUNDS": 8}
    assert (A.CAMPAIGN_RESOLVE, A.CAMPAIGN_RESOLVE_ROUNDS_SHIFT, A.CAMPAIGN_RESOLVE_ROUNDS_MASK, A.RESOLVE_DEFAULT_ROUNDS, A.RESOLVE_MAX_ROUNDS) \
        == (32, 8, 0xF00, 4, 8)
    assert D["MADSIM_RESOLVE_MAX_ROUNDS"] == len(A.Resolve().n_by_round)
    # a new flag bit, beside the five there were, and the rounds bits clear of all of them
    flags = [int(H.defines()["MADSIM_CAMPAIGN_" + k].rstrip("u")) for k in ("STOP_AT_FAILURE", "LIST_RUNNER", "STOP_AT_CAP", "STOP_AT_GROUPS", "STOP_AT_DIFFS")]
    assert flags == [1, 2, 4, 8, 16] and not (sum(flags) | 32) & 0xF00
    assert int(H.defines()["MADSIM_HIP_ABI_VERSION"].rstrip("u")) == A.ABI_VERSION == 7          # additive: the version stays


def test_the_three_new_functions_and_the_fifteen_old_signatures():
    L, fns = runtime.lib(), H.functions()
    assert fns["madsim_hip_campaign_resolved"] == ("int", ["madsim_resolve_t*"])
    assert fns["madsim_hip_ctx_campaign_resolved"] == ("int", ["madsim_hip_ctx_t*", "madsim_resolve_t*"])
    assert fns["madsim_hip_grow_limits"] == ("int", ["const madsim_workload_t*", "const madsim_limits_t*", "uint32_t", "madsim_limits_t*"])
    for name in ("madsim_hip_campaign_resolved", "madsim_hip_ctx_campaign_resolved", "madsim_hip_grow_limits"):
        assert hasattr(L, name), name
    plain = ["const madsim_workload_t*", "const madsim_config_t*", "uint64_t", "uint64_t", "uint64_t", "uint32_t", "uint32_t", "const madsim_limits_t*",
             "madsim_campaign_t*"]
    side = ["const madsim_workload_t*", "const madsim_config_t*", "const madsim_limits_t*"]
    tails = {"": [], "_collect": ["madsim_collect_t*"], "_stats": ["madsim_collect_t*", "madsim_stats_t*"],
             "_groups": ["madsim_collect_t*", "madsim_stats_t*", "madsim_groups_t*"]}
    n = 0
    for form, tail in tails.items():
        assert fns[f"madsim_hip_run_campaign{form}"] == ("int", plain + tail)
        assert fns[f"madsim_hip_ctx_run_campaign{form}"] == ("int", ["madsim_hip_ctx_t*"] + plain + tail)
        assert fns[f"madsim_hip_run_campaign{form}_multi"] == ("int", ["madsim_hip_ctx_t* const*", "int"] + plain + tail)
        n += 3
    diff = side + side + ["uint64_t", "uint64_t", "uint64_t", "uint32_t", "uint32_t", "madsim_campaign_t*", "madsim_campaign_t*", "madsim_diff_t*"]
    assert fns["madsim_hip_run_campaign_diff"] == ("int", diff)
    assert fns["madsim_hip_ctx_run_campaign_diff"] == ("int", ["madsim_hip_ctx_t*"] + diff)
    assert fns["madsim_hip_run_campaign_diff_multi"] == ("int", ["madsim_hip_ctx_t* const*", "int"] + diff)
    assert n + 3 == 15 == len([f for f in fns if "run_campaign" in f])
    assert [f[0] for f in A.Campaign._fields_] == ["seeds_run", "batches_run", "batches_launched", "first_failing_seed", "n_failed", "n_runner",
                                                   "total_steps", "total_clock_ns", "kernel_ms", "wall_s"]


CAPS = ("heap_lds_slots", "heap_spill_slots", "max_tasks", "mbox_regs", "mbox_msgs", "max_conns", "chan_queue", "max_steps", "lanes_per_wave")


def caps(lim):
    return tuple(int(getattr(lim, f)) for f in CAPS)


def test_grow_limits_against_the_table():
    w = workload.pingpong(4, 8)
    P = w.struct.n_progs
    assert P == 5
    zero = A.Limits()
    assert bytes(runtime.grown_limits(w, zero, 0)) == bytes(zero)                         # rounds = 0: the identity
    some = A.Limits()
    some.time_limit_ns, some.max_steps, some.heap_lds_slots, some.heap_spill_slots, some.sched, some.state_mem = 5, 77, 3, 9, 1, A.STATE_GLOBAL | A.STATE_DEDUP_TIMERS
    assert bytes(runtime.grown_limits(w, some, 0)) == bytes(some)
    # from all-zero limits, round by round: heap_lds, heap_spill, max_tasks, mbox_regs, mbox_msgs, max_conns, chan_queue, max_steps, lanes_per_wave
    table = {1: (8, 64, 2 * (P + 8), 4, 4, 8, 4, 1 << 28, 0),
             2: (8, 128, 52, 8, 8, 16, 8, 1 << 28, 0),
             3: (8, 256, 104, 16, 16, 32, 15, 1 << 28, 0),
             4: (8, 512, 208, 32, 32, 64, 15, 1 << 28, 0),
             5: (8, 1024, 254, 64, 64, 127, 15, 1 << 28, 0),
             8: (8, 8192, 254, 255, 127, 127, 15, 1 << 28, 0)}                            # (mbox_msgs: the ping-pong has no extended op, its builds take 127)
    for rounds, want in table.items():
        assert caps(runtime.grown_limits(w, zero, rounds)) == want, rounds
    assert caps(runtime.grown_limits(w, None, 1)) == table[1]                             # no limits = the defaults
    ext = workload.WorkloadBuilder()                                                      # one extended op: mbox_msgs goes on to 255
    n = ext.create_node(); a = ext.addr(n, 1)
    t = ext.task(n); t.bind(a); t.recv_from_timeout(a, 1, ms=1); t.done()
    m = ext.main(); m.spawn(t); m.join(t); m.done()
    assert [runtime.grown_limits(ext.build(), zero, r).mbox_msgs for r in (5, 6, 7, 8)] == [64, 128, 255, 255]
    assert [runtime.grown_limits(w, zero, r).mbox_msgs for r in (5, 6, 7)] == [64, 127, 127]
    # MADSIM_LIMIT_NONE counts as unset; an explicit LDS quota is kept, lanes_per_wave is dropped
    lim = A.Limits()
    lim.mbox_regs, lim.heap_lds_slots, lim.lanes_per_wave, lim.heap_spill_slots = A.LIMIT_NONE, 2, 16, 1
    g = runtime.grown_limits(w, lim, 1)
    assert (g.mbox_regs, g.heap_lds_slots, g.lanes_per_wave, g.heap_spill_slots) == (4, 2, 0, 2)
    assert runtime.grown_limits(w, lim, 3).heap_spill_slots == 8
    # the state layout: COMPACT becomes AUTO, NARROW_HEAP is cleared, DEDUP_TIMERS is kept
    lim = A.Limits()
    lim.state_mem = A.STATE_COMPACT | A.STATE_NARROW_HEAP | A.STATE_DEDUP_TIMERS
    assert runtime.grown_limits(w, lim, 1).state_mem == A.STATE_AUTO | A.STATE_DEDUP_TIMERS
    lim.state_mem = A.STATE_GLOBAL | A.STATE_NARROW_HEAP
    assert runtime.grown_limits(w, lim, 2).state_mem == A.STATE_GLOBAL
    # after 8 rounds every capacity sits at its ceiling (the spill quota from 4 096: 4 096 * 2^8 = 2^20)
    lim = A.Limits()
    lim.heap_spill_slots = 4096
    g = runtime.grown_limits(w, lim, 8)
    assert (g.max_tasks, g.mbox_regs, g.mbox_msgs, g.max_conns, g.chan_queue, g.heap_spill_slots) == (254, 255, 127, 127, 15, 1 << 20)      # (mbox_msgs: a base-op workload's ceiling)
    assert caps(runtime.grown_limits(w, lim, 9)) == caps(g)                               # ... and stays there
    # max_steps: 16-fold per round, never above max_steps_ceiling (0 = 2^28), which is never below the first pass's cap
    for first, ceiling, want in ((64, 1024, [1024, 1024]), (64, 128, [128, 128]), (64, 0, [1024, 16384]), (0, 0, [1 << 28, 1 << 28]),
                                 (1000, 500, [1000, 1000]), (3, 1 << 30, [48, 768])):
        lim = A.Limits()
        lim.max_steps, lim.max_steps_ceiling = first, ceiling
        got = [runtime.grown_limits(w, lim, r).max_steps for r in (1, 2)]
        assert got == want, (first, ceiling, got)
        assert all(s <= max(ceiling or 1 << 28, first or 1 << 24) for s in got)
    # what a round never touches
    lim = A.Limits()
    lim.time_limit_ns, lim.sched, lim.no_trace_hash, lim.max_steps_ceiling = 123456789, A.SCHED_QUEUE, 1, 4096
    g = runtime.grown_limits(w, lim, 8)
    assert (g.time_limit_ns, g.sched, g.no_trace_hash, g.max_steps_ceiling) == (123456789, A.SCHED_QUEUE, 1, 4096)
    # argument errors
    L = runtime.lib()
    out = A.Limits()
    assert L.madsim_hip_grow_limits(None, C.byref(lim), 1, C.byref(out)) == E_ARG
    assert L.madsim_hip_grow_limits(w.ref(), C.byref(lim), 1, None) == E_ARG
    assert L.madsim_hip_grow_limits(w.ref(), C.byref(lim), 65, C.byref(out)) == E_ARG


def _forms(flags):
    """Every campaign form x every call form with the same flags and null contexts: fifteen return codes, by entry point."""
    L = runtime.lib()
    w, cfg, lim = workload.pingpong(4, 8), A.Config.default(), A.Limits()
    rep, rep_b, col, st, grp, d = A.Campaign(), A.Campaign(), A.Collect(), A.Stats(), A.Groups(), A.Diff()
    st.include, grp.include, d.fields = 1, 2, A.DIFF_ALL
    arr = (C.c_void_p * 1)(None)
    head = (w.ref(), C.byref(cfg), 0, 100, 0, 0, flags, C.byref(lim), C.byref(rep))
    tails = {"": (), "_collect": (C.byref(col),), "_stats": (C.byref(col), C.byref(st)), "_groups": (C.byref(col), C.byref(st), C.byref(grp))}
    out = {}
    for form, tail in tails.items():
        out[f"madsim_hip_run_campaign{form}"] = getattr(L, f"madsim_hip_run_campaign{form}")(*head, *tail)
        out[f"madsim_hip_ctx_run_campaign{form}"] = getattr(L, f"madsim_hip_ctx_run_campaign{form}")(None, *head, *tail)
        out[f"madsim_hip_run_campaign{form}_multi"] = getattr(L, f"madsim_hip_run_campaign{form}_multi")(arr, 1, *head, *tail)
    side = (w.ref(), C.byref(cfg), C.byref(lim))
    dtail = (0, 100, 0, 0, flags, C.byref(rep), C.byref(rep_b), C.byref(d))
    out["madsim_hip_run_campaign_diff"] = L.madsim_hip_run_campaign_diff(*side, *side, *dtail)
    out["madsim_hip_ctx_run_campaign_diff"] = L.madsim_hip_ctx_run_campaign_diff(None, *side, *side, *dtail)
    out["madsim_hip_run_campaign_diff_multi"] = L.madsim_hip_run_campaign_diff_multi(arr, 1, *side, *side, *dtail)
    assert len(out) == 15
    return out


def test_argument_errors_need_no_gpu():
    """Told before any context is looked at, so they hold with and without a device (the contexts here are null)."""
    assert set(_forms(RESOLVE9).values()) == {E_ARG}                                     # nine rounds with the flag: every entry point
    assert b"rounds" in runtime.lib().madsim_hip_last_error()
    for rounds in (10, 15):
        assert set(_forms(A.CAMPAIGN_RESOLVE | rounds << 8).values()) == {E_ARG}
    # the rounds bits without the flag are ignored, as unknown bits are: the call gets as far as its (null) context
    for flags in (9 << 8, 15 << 8, 0):
        rcs = _forms(flags)
        for name, rc in rcs.items():
            if "_ctx_" in name or name.endswith("_multi"):
                assert rc == E_NOINIT, (name, flags, rc)
            else:
                assert rc in (E_NOINIT, E_HIP) or not _no_gpu(), (name, flags, rc)
    # a valid resolving call: every number of rounds the flag admits gets past the argument checks
    for rounds in (0, 1, 8):
        rcs = _forms(A.CAMPAIGN_RESOLVE | rounds << 8)
        assert all(rc == E_NOINIT for name, rc in rcs.items() if "_ctx_" in name or name.endswith("_multi")), (rounds, rcs)
    # the mirror: nine rounds reach the library and come back as its error; sixteen do not fit the bits
    if _no_gpu():
        with pytest.raises(runtime.MadsimHipError):
            runtime.run_campaign(workload.pingpong(4, 8), 0, 100, resolve=9)
    with pytest.raises(runtime.MadsimHipError, match="resolve"):
        runtime.run_campaign_multi([], workload.pingpong(4, 8), 0, 100, resolve=16)
    assert runtime._resolve_flags(None) == runtime._resolve_flags(False) == 0 and runtime._resolve_flags(True) == 32
    assert runtime._resolve_flags(1) == 32 | 1 << 8 and runtime._resolve_flags(8) == 32 | 8 << 8


def test_no_gpu_means_loud_failure_not_an_unresolved_report():
    if not _no_gpu():
        pytest.skip("a GPU is present")
    w = workload.pingpong(4, 8)
    for kw in (dict(resolve=True), dict(resolve=2, collect=16), dict(resolve=8, collect=0, list_runner=True)):
        with pytest.raises(runtime.MadsimHipError, match="HIP|context|initiali"):
            runtime.run_campaign(w, 0, 1000, **kw)
    with pytest.raises(runtime.MadsimHipError, match="HIP|context|initiali"):
        runtime.run_campaign_stats(w, 0, 1000, resolve=True)
    with pytest.raises(runtime.MadsimHipError, match="HIP|context|initiali"):
        runtime.run_campaign_groups(w, 0, 1000, resolve=True)
    with pytest.raises(runtime.MadsimHipError, match="HIP|context|initiali"):
        runtime.run_campaign_diff_resolved(w, 0, 1000)


def test_campaign_resolved_before_any_campaign_is_all_zero():
    L = runtime.lib()
    if _no_gpu():
        r = runtime.campaign_resolved()                                                    # no default context: nothing has run through it
    else:
        with runtime.Context(0) as c:                                                      # a fresh context: nothing has run through it
            r = c.campaign_resolved()
    assert bytes(r) == bytes(C.sizeof(A.Resolve))
    r.n_first_pass = 7
    assert L.madsim_hip_ctx_campaign_resolved(None, C.byref(r)) == E_NOINIT and r.n_first_pass == 0      # a null context: an error, and zeros
    assert L.madsim_hip_campaign_resolved(None) == E_ARG and L.madsim_hip_ctx_campaign_resolved(None, None) == E_ARG


def test_every_wrapper_takes_resolve():
    fns = [runtime.run_campaign, runtime.run_campaign_stats, runtime.run_campaign_groups, runtime.run_campaign_multi, runtime.run_campaign_stats_multi,
           runtime.run_campaign_groups_multi, runtime.run_campaign_diff_multi, runtime.Context.run_campaign, runtime.Context.run_campaign_stats,
           runtime.Context.run_campaign_groups, runtime.Context.run_campaign_diff]
    for fn in fns:
        assert inspect.signature(fn).parameters["resolve"].default is None, fn.__name__
    # the default-context differential wrapper's parameter list is pinned by its own test: its resolving form is a sibling
    assert "resolve" not in inspect.signature(runtime.run_campaign_diff).parameters
    assert inspect.signature(runtime.run_campaign_diff_resolved).parameters["resolve"].default is True
    assert callable(runtime.grown_limits) and callable(runtime.campaign_resolved) and callable(runtime.Context.campaign_resolved)
    assert callable(runtime.grow_limits)                                                  # the older helper stays
