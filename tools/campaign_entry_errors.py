#!/usr/bin/env python3
"""What the campaign entry points of libmadsim_hip.so answer to calls that need no device: (return code, madsim_hip_last_error()) per call.

The table covers the ten campaign operations in their three spellings — madsim_hip_X (the default context), madsim_hip_ctx_X and
madsim_hip_X_multi — with one argument fault per row, rows that combine two faults (the message then tells which check runs first), and
the context errors that are told without a device: a NULL context, no contexts, and the list forms' "an empty list needs no device".
A default-context spelling only gets the rows whose fault is told before any context is looked at (`pre`): what it answers to the others
depends on whether the process has initialised a device.

    python tools/campaign_entry_errors.py            print the table as JSON
    python tools/campaign_entry_errors.py --write    write tests/golden/campaign_entry_errors.json

tests/test_campaign_entry_errors.py holds the library against that file.  MADSIM_HIP_LIB names another build of the library to record from.
"""
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from madsim_amd import _abi as A            # noqa: E402
from madsim_amd import runtime, workload    # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "campaign_entry_errors.json")
RESOLVE_9_ROUNDS = A.CAMPAIGN_RESOLVE | 9 << A.CAMPAIGN_RESOLVE_ROUNDS_SHIFT

# operation -> (kind, takes a list, the trailing parts of its signature)
OPS = {
    "run_campaign": ("plain", False, ()),
    "run_campaign_collect": ("plain", False, ("col",)),
    "run_campaign_stats": ("plain", False, ("col", "st")),
    "run_campaign_groups": ("plain", False, ("col", "st", "grp")),
    "run_seeds_campaign": ("plain", True, ("col", "st", "grp")),
    "run_campaign_diff": ("pair", False, ("diff",)),
    "run_seeds_campaign_diff": ("pair", True, ("diff",)),
    "run_paired_campaign": ("pair", False, ("diff", "pr")),
    "run_seeds_campaign_paired": ("pair", True, ("diff", "pr")),
    "run_sweep_campaign": ("sweep", False, ()),
}


def put(**kv):
    return lambda v: v.update(kv)


def field(key, **kv):
    def apply(v):
        for name, x in kv.items():
            setattr(v[key], name, x)
    return apply


def flag(bits):
    def apply(v):
        v["flags"] |= bits
    return apply


def faults(op):
    """{name: (what it does to a valid call's values, told before any context is looked at)} for one operation."""
    kind, listed, parts = OPS[op]
    f = {
        "in_flight_9": (put(in_flight=9), op != "run_campaign"),      # (the plain form hears of it from the engine, behind the context)
        "resolve_rounds_9": (flag(RESOLVE_9_ROUNDS), True),
    }
    if listed:
        f["null_list"] = (put(seeds=None, n=3), True)
    if listed or kind == "sweep":                               # (a sweep over a NULL list is its range form)
        f["unsorted_list"] = (put(seeds=[1, 3, 2]), True)
        f["duplicate_in_list"] = (put(seeds=[1, 2, 2]), True)
    if not listed:
        f["range_wraps"] = (put(seed0=(1 << 64) - 8, total=16), kind == "sweep")
    if kind == "plain":
        f["null_report"] = (put(out=None), True)
        if op == "run_seeds_campaign":
            f["stop_at_cap_without_collect"] = (lambda v: (v.update(col=None), flag(A.CAMPAIGN_STOP_AT_CAP)(v)), False)      # (an absent part's flag is ignored)
        if "col" in parts:
            if op == "run_campaign_collect":
                f["null_collect"] = (put(col=None), True)
            f["collect_cap_without_array"] = (field("col", cap=4), True)
            f["stop_at_cap_cap_0"] = (flag(A.CAMPAIGN_STOP_AT_CAP), True)
        if "st" in parts:
            if op == "run_campaign_stats":
                f["null_stats"] = (put(st=None), True)
            f["stats_include_0"] = (field("st", include=0), True)
            f["stats_include_0x10"] = (field("st", include=0x10), True)
            f["stats_top_k_17"] = (field("st", top_k=17), True)
            f["stats_top_k_without_array"] = (field("st", top_k=4), True)
        if "grp" in parts:
            if op == "run_campaign_groups":
                f["null_groups"] = (put(grp=None), True)
            f["groups_include_0"] = (field("grp", include=0), True)
            f["groups_include_0x10"] = (field("grp", include=0x10), True)
            f["groups_key_field_6"] = (field("grp", key_field=6), True)
            f["groups_cap_without_array"] = (field("grp", cap=4), True)
            f["stop_at_groups_cap_0"] = (flag(A.CAMPAIGN_STOP_AT_GROUPS), True)
            big = A.GROUP_MAX_BATCH + 1
            f["group_batch_too_large"] = (lambda v: v.update(batch=big, total=2 * big, seeds=np.arange(2 * big, dtype=np.uint64) if listed else None), True)
    if kind == "pair":
        paired = "pr" in parts
        f["null_report_a"] = (put(outA=None), True)
        f["null_report_b"] = (put(outB=None), True)
        f["null_diff"] = (put(diff=None), not paired)           # (a paired campaign's diff report is optional)
        f["diff_fields_0"] = (field("diff", fields=0), True)
        f["diff_fields_0x80"] = (field("diff", fields=0x80), True)
        f["diff_reserved"] = (field("diff", reserved=1), True)
        f["diff_cap_without_array"] = (field("diff", cap=4), True)
        f["stop_at_diffs_cap_0"] = (flag(A.CAMPAIGN_STOP_AT_DIFFS), True)
        if paired:
            f["null_paired"] = (put(pr=None), True)
            f["paired_include_a_0"] = (field("pr", include_a=0), True)
            f["paired_include_b_0x10"] = (field("pr", include_b=0x10), True)
            f["paired_reserved"] = (field("pr", reserved=1), True)
            f["paired_top_k_17"] = (field("pr", top_k=17), True)
            f["paired_top_k_without_array"] = (field("pr", top_k=4), True)
            f["null_reports_without_diff"] = (put(diff=None, outA=None), True)
    if kind == "sweep":
        f["one_variant"] = (put(n_variants=1), True)
        f["nine_variants"] = (put(n_variants=9), True)
        f["null_variants"] = (put(null_variants=True), True)
        f["null_sweep"] = (put(sweep=None), True)
        f["variant_null_workload"] = (put(variant_null="w"), True)
        f["variant_null_report"] = (put(variant_null="out"), True)
        f["sweep_fields_0x80"] = (field("sweep", fields=0x80), True)
        f["sweep_list_rule_3"] = (field("sweep", list_rule=3), True)
        f["differing_without_fields"] = (field("sweep", list_rule=A.SWEEP_LIST_DIFFERING, fields=0), True)
        f["sweep_cap_without_array"] = (field("sweep", cap=4), True)
        f["stop_at_sweep_cap_0"] = (flag(A.CAMPAIGN_STOP_AT_SWEEP), True)
        f["list_with_seed0"] = (put(seeds=[1, 2, 3], seed0=5), True)
    return f


def combos(op):
    """The rows of two faults: the answer names the check that runs first."""
    kind, listed, parts = OPS[op]
    c = [("resolve_rounds_9", "in_flight_9")]
    if kind == "plain":
        c += [("null_report", "in_flight_9"), ("null_report", "resolve_rounds_9")]
        if "col" in parts:
            c += [("collect_cap_without_array", "resolve_rounds_9"), ("stop_at_cap_cap_0", "in_flight_9")]
        if "st" in parts:
            c += [("stats_include_0", "collect_cap_without_array"), ("stats_top_k_17", "resolve_rounds_9")]
        if "grp" in parts:
            c += [("groups_include_0", "stats_include_0"), ("group_batch_too_large", "stats_include_0"), ("resolve_rounds_9", "group_batch_too_large"),
                  ("group_batch_too_large", "in_flight_9")]
    if kind == "pair":
        c += [("diff_fields_0", "in_flight_9"), ("null_report_a", "null_diff"), ("stop_at_diffs_cap_0", "resolve_rounds_9")]
        if "pr" in parts:
            c += [("null_paired", "null_report_a"), ("paired_include_a_0", "diff_fields_0"), ("paired_top_k_17", "in_flight_9")]
    if kind == "sweep":
        c += [("one_variant", "null_sweep"), ("null_variants", "nine_variants"), ("sweep_cap_without_array", "resolve_rounds_9"),
              ("unsorted_list", "in_flight_9"), ("range_wraps", "resolve_rounds_9"), ("variant_null_report", "sweep_fields_0x80")]
    if listed:
        c += [("unsorted_list", "null_report" if kind == "plain" else "null_report_a"), ("null_list", "in_flight_9")]
    return c


_W = None


def valid(op):
    """The values of a call of `op` that has no fault: what a row's faults are applied to."""
    global _W
    if _W is None:
        _W = workload.pingpong(4, 8)
    kind, listed, parts = OPS[op]
    v = dict(w=_W, cfg=A.Config.default(), lim=A.Limits(), seed0=0, total=16, seeds=[1, 2, 3] if listed else None, n=None, batch=0, in_flight=0, flags=0)
    if kind == "plain":
        v.update(out=A.Campaign(), col=A.Collect() if "col" in parts else None, st=A.Stats(include=1) if "st" in parts else None,
                 grp=A.Groups(include=2) if "grp" in parts else None)
    elif kind == "pair":
        v.update(outA=A.Campaign(), outB=A.Campaign(), diff=A.Diff(fields=A.DIFF_ALL), pr=A.Paired(include_a=1, include_b=1) if "pr" in parts else None)
    else:
        v.update(n_variants=2, null_variants=False, variant_null=None, sweep=A.Sweep(fields=A.DIFF_VERDICT), outs=[A.Campaign() for _ in range(9)])
    return v


def ref(x):
    return None if x is None else C.byref(x)


def arguments(op, v):
    """(the C arguments of `op` behind its contexts, the campaign reports the call fills, what must stay alive)."""
    kind, listed, parts = OPS[op]
    seeds = None if v["seeds"] is None else np.ascontiguousarray(np.asarray(v["seeds"], dtype=np.uint64))
    ptr = None if seeds is None else seeds.ctypes.data_as(C.POINTER(C.c_uint64)) if seeds.size else C.cast(C.pointer(C.c_uint64(0)), C.POINTER(C.c_uint64))
    n = v["n"] if v["n"] is not None else 0 if seeds is None else len(seeds)
    where = [ptr, n] if listed else [v["seed0"], v["total"]]
    tail = [v["batch"], v["in_flight"], v["flags"]]
    if kind == "plain":
        reports = [v["out"]]
        args = [v["w"].ref(), C.byref(v["cfg"])] + where + tail + [C.byref(v["lim"]), ref(v["out"])] + [ref(v[p]) for p in parts]
    elif kind == "pair":
        reports = [v["outA"], v["outB"]]
        side = [v["w"].ref(), C.byref(v["cfg"]), C.byref(v["lim"])]
        args = side + side + where + tail + [ref(v["outA"]), ref(v["outB"])] + [ref(v[p]) for p in parts]
    else:
        reports = v["outs"][:2]
        var = (A.SweepVariant * 9)()
        for i in range(9):
            var[i].w, var[i].out = C.pointer(v["w"].struct), C.pointer(v["outs"][i])
        if v["variant_null"] == "w":
            var[1].w = None
        if v["variant_null"] == "out":
            var[1].out = None
        if seeds is not None or v["n"] is not None:             # the list form: (seed0, n, the list)
            where = [v["seed0"], n, ptr]
        else:
            where = [v["seed0"], v["total"], None]
        args = [None if v["null_variants"] else var, v["n_variants"]] + where + tail + [ref(v["sweep"])]
        seeds = (seeds, var)
    for r in reports:
        if r is not None:
            C.memset(C.byref(r), 0xAA, C.sizeof(r))             # (a call that succeeds must have reset them)
    return args, reports, (seeds, v)


def rows():
    """[(row id, C symbol, the operation, the context arguments in front, the faults by name)]: the whole table."""
    out = []
    null_handle = (C.c_void_p * 1)(None)
    for op, (kind, listed, _) in OPS.items():
        f = faults(op)
        named = [(name,) for name in f] + combos(op)
        spellings = (("madsim_hip_" + op, [], True), ("madsim_hip_ctx_" + op, [None], False), (f"madsim_hip_{op}_multi", [None, 0], False))
        for symbol, front, pre_only in spellings:
            for names in named:
                if pre_only and not any(f[x][1] for x in names):
                    continue
                out.append((f"{symbol}:{'+'.join(names)}", symbol, op, front, names))
        empty = ["empty_list"] if listed or kind == "sweep" else []
        if kind == "sweep":
            empty.append("nothing_to_run")
        ctx, multi = "madsim_hip_ctx_" + op, f"madsim_hip_{op}_multi"
        out.append((ctx + ":null_context", ctx, op, [None], ()))
        out += [(f"{ctx}:{e}+null_context", ctx, op, [None], (e,)) for e in empty]
        out.append((multi + ":null_contexts", multi, op, [None, 1], ()))
        out.append((multi + ":no_contexts", multi, op, [null_handle, 0], ()))
        out.append((multi + ":null_context_in_list", multi, op, [null_handle, 1], ()))
        out += [(f"{multi}:{e}+no_contexts", multi, op, [null_handle, 0], (e,)) for e in empty]
    return out


_NOTHING = {"empty_list": put(seeds=[]), "nothing_to_run": put(total=0)}


def observe(L=None):
    """{row id: {"rc", "error"}} from the library — for a call that returns 0, {"rc": 0, "reports": the integer fields of each campaign report}."""
    L = L or runtime.lib()
    got = {}
    for row, symbol, op, front, names in rows():
        v, f = valid(op), faults(op)
        for name in names:
            (_NOTHING[name] if name in _NOTHING else f[name][0])(v)
        args, reports, keep = arguments(op, v)
        rc = getattr(L, symbol)(*(front + args))
        if rc:
            got[row] = {"rc": rc, "error": L.madsim_hip_last_error().decode()}
        else:
            got[row] = {"rc": 0, "reports": [[r.seeds_run, r.batches_run, r.batches_launched, r.first_failing_seed, r.n_failed, r.n_runner, r.total_steps]
                                             for r in reports]}
        del keep
    return got


if __name__ == "__main__":
    text = json.dumps(observe(), indent=1, sort_keys=True) + "\n"
    if "--write" in sys.argv[1:]:
        with open(GOLDEN, "w") as fh:
            fh.write(text)
    else:
        sys.stdout.write(text)
