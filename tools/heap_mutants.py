#!/usr/bin/env python3
"""Do the heap-boundary cases (tests/heap_cases.py) see a wrong tie order in timer_pop?  CPU only, not a test.

Copies madsim_amd/csrc, include and tests/emu to a temporary directory, once unchanged and once per mutant — three one-character edits of
k_timer.h's timer_pop, each a tie rule of BinaryHeap::pop turned round, each asserted to match the source exactly once —, builds the host
emulation from every copy with the command tests/emu uses, loads it through MADSIM_EMU_LIB (one child process per copy) and prints, per
copy, layout, workload and quota, how many of the 130 seeds differ from the oracle.

Required: every mutant is seen in at least two cases, the unchanged copy in none (exit status 1 otherwise).

    python tools/heap_mutants.py [--layouts rq_spill,queue_spill,...] [--md]        (--md: the table of profiles/heap_boundaries.md)
"""
import argparse
import json
import os
import shutil
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K_TIMER = os.path.join("madsim_amd", "csrc", "kernel", "k_timer.h")

MUTANTS = {
    "A": ("the spilled loop's stop test `ev_deadline(cand) <= idl` -> `<`",
          "                go = ev_deadline(cand) <= idl;\n",
          "                go = ev_deadline(cand) < idl;\n"),
    "B": ("the LDS-first loop's `ev_deadline(l) >= ev_deadline(r)` -> `>`",
          "                    heap_lds_get2<K>(c, L, child, l, r);\n                    const bool right = ev_deadline(l) >= ev_deadline(r);\n",
          "                    heap_lds_get2<K>(c, L, child, l, r);\n                    const bool right = ev_deadline(l) > ev_deadline(r);\n"),
    "C": ("`idl < ev_deadline(m)` -> `<=` in front of the final heap_sift_up",
          "!moved_below && pos > 0 && idl < ev_deadline(m)) {",
          "!moved_below && pos > 0 && idl <= ev_deadline(m)) {"),
}
DEFAULT_LAYOUTS = "rq_spill,queue_spill,stride32,time_lds,all_lds64,g_time64,g_time64_nh,g_time64_nhdd,g_all,g_all_nh"


def make_copy(tmp, name):
    """The sources the emulation is built from, under tmp/name, edited for mutant `name` ("clean": unchanged); -> the library's path."""
    top = os.path.join(tmp, name)
    for d in (os.path.join("madsim_amd", "csrc"), "include", os.path.join("tests", "emu")):
        shutil.copytree(os.path.join(ROOT, d), os.path.join(top, d), ignore=shutil.ignore_patterns("*.o", "*.so", "*.lock", "*.tmp", "__pycache__"))
    if name != "clean":
        _, old, new = MUTANTS[name]
        path = os.path.join(top, K_TIMER)
        src = open(path).read()
        assert src.count(old) == 1, (name, "the text to edit occurs", src.count(old), "times in", K_TIMER)
        open(path, "w").write(src.replace(old, new))
    here = os.path.join(top, "tests", "emu")
    lib = os.path.join(here, "libmadsim_emu.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-DMADSIM_EMU", "-x", "c++", "-I" + here, "-o", lib,
                           os.path.join(here, "emu_driver.cpp")])
    return lib


def child(layouts):
    """(in a process with MADSIM_EMU_LIB set) -> JSON rows [layout, workload key, q, differing seeds]."""
    sys.path.insert(0, ROOT)
    from tests import emu
    from tests import heap_cases as H
    rows = []
    for layout in layouts:
        for key, q, n in H.count_differing(layout, emu.run_batch):
            rows.append([layout, list(key), q, n])
    json.dump(rows, sys.stdout)


def name_of(key):
    kind, n, rounds, flavour = key
    return f"{kind}({n}, {rounds}){'' if flavour == 'base' else ', timeouts only' if flavour == 'time' else ', every class'}"


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--layouts", default=DEFAULT_LAYOUTS)
    ap.add_argument("--md", action="store_true", help="print the table as markdown")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    layouts = args.layouts.split(",")
    if args.child:
        return child(layouts)
    names = ["clean"] + list(MUTANTS)
    seen = {}
    with tempfile.TemporaryDirectory(prefix="heap_mutants.") as tmp:
        with ThreadPoolExecutor(len(names)) as pool:
            libs = dict(zip(names, pool.map(lambda n: make_copy(tmp, n), names)))

        def run(name):
            env = dict(os.environ, MADSIM_EMU_LIB=libs[name])
            out = subprocess.check_output([sys.executable, os.path.abspath(__file__), "--child", "--layouts", args.layouts], env=env)
            return [(lay, tuple(key), q, n) for lay, key, q, n in json.loads(out)]
        with ThreadPoolExecutor(len(names)) as pool:
            rows = dict(zip(names, pool.map(run, names)))
    if args.md:
        print("| Copy | Layout | Workload | Quotas at which seeds differ (q: seeds of 130) | Cases seen / run |")
        print("|---|---|---|---|---|")
    for name in names:
        what = "unchanged" if name == "clean" else MUTANTS[name][0]
        seen[name] = sum(1 for r in rows[name] if r[3])
        if not args.md:
            print(f"== {name}: {what}: seen in {seen[name]} of {len(rows[name])} cases")
        if args.md and name == "clean":
            print(f"| clean | every layout | every workload | {'none' if not seen[name] else 'SOME'} | {seen[name]} / {len(rows[name])} |")
            continue
        groups = {}
        for lay, key, q, n in rows[name]:
            groups.setdefault((lay, key), []).append((q, n))
        for (lay, key), qs in groups.items():
            hit = ", ".join(f"{q}: {n}" for q, n in qs if n)
            if args.md:
                if hit:
                    print(f"| {name} | {lay} | {name_of(key)} | {hit or 'none'} | {sum(1 for _, n in qs if n)} / {len(qs)} |")
            else:
                print(f"   {lay:14s} {name_of(key):40s} {hit or '-'}")
    ok = seen["clean"] == 0 and all(seen[m] >= 2 for m in MUTANTS)
    print(("\n" if args.md else "") + "; ".join(f"{n}: {seen[n]} cases" for n in names) + (" -- every mutant caught, the unchanged copy clean" if ok else " -- NOT as required"))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
