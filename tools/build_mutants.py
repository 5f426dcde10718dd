#!/usr/bin/env python3
"""Do the build-matrix cases (tests/build_cases.py) see a handler that is wrong on ONE family of builds only?  CPU only, not a test.

Copies madsim_amd/csrc, include and tests/emu to a temporary directory, once unchanged and once per mutant — three one-line edits of the
kernel, each a fault behind a build property (so every other build compiles to what it was), each asserted to match the source exactly
once —, builds the host emulation from every copy with the command tests/emu uses and loads it through MADSIM_EMU_LIB.  Per copy it runs

  * the suite as it was before the matrix: every non-gpu test file that runs the host-compiled kernel through that hook (SUITE below), and
  * the matrix cases, counting per row and case how many of the 130 seeds differ from the oracle.

Required: the unchanged copy fails nowhere; with every mutant the earlier suite still passes and the matrix cases see it, on rows of the
mutant's family only (exit status 1 otherwise).

    python tools/build_mutants.py [--md] [--skip-suite]        (--md: the table of profiles/build_matrix.md)
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
K_POLL = os.path.join("madsim_amd", "csrc", "kernel", "k_poll.h")
K_CHANNEL = os.path.join("madsim_amd", "csrc", "kernel", "k_channel.h")

# name -> (what, file, old text, new text, the FEAT bits a row must have to be of the family, whether global-state rows only)
MUTANTS = {
    "A": ("MS_OP_CSEND queues `imm ^ 1` on the ticker and select builds (K::FK)", K_POLL,
          "                CONNW(id, e) = imm; CONNW(id, e + 1) = (uint32_t)arrive;",
          "                CONNW(id, e) = imm ^ (uint32_t)K::FK; CONNW(id, e + 1) = (uint32_t)arrive;", 512, False),
    "B": ("guard_release keeps the socket's last guard on the global-state signal builds (K::G && K::FSIG)", K_CHANNEL,
          "    if (!(h >> 25)) return;\n    h -= 1u << 25;",
          "    if (!(h >> 25) || (K::G && K::FSIG)) return;\n    h -= 1u << 25;", 2048, True),
    "C": ("MS_OP_ADVANCE moves the clock one nanosecond too far on the select builds (K::FSEL)", K_POLL,
          "                L.clock += (uint64_t)b * NS_PER_S + imm;\n                pc++;\n                u0.y = pc | (sub << 16) | (from << 24);\n                TU(c, slot, 0) = u0;\n                if (u1_dirty) { tu1_store<K>(c, slot, u1); u1_dirty = false; }\n                timer_expire<K>(c, L, L.clock);",
          "                L.clock += (uint64_t)b * NS_PER_S + imm + (K::FSEL ? 1u : 0u);\n                pc++;\n                u0.y = pc | (sub << 16) | (from << 24);\n                TU(c, slot, 0) = u0;\n                if (u1_dirty) { tu1_store<K>(c, slot, u1); u1_dirty = false; }\n                timer_expire<K>(c, L, L.clock);", 1024, False),
}
# the non-gpu test files that run the host-compiled kernel through MADSIM_EMU_LIB, as they were before the matrix
SUITE = ["test_builder", "test_emu_cold_params", "test_emu_heap_boundaries", "test_emu_parity", "test_emu_pass_invariants", "test_geometry_consistency",
         "test_interval", "test_model_edges", "test_select", "test_signal", "test_timeout_scope"]


def make_copy(tmp, name):
    """The sources the emulation is built from, under tmp/name, edited for mutant `name` ("clean": unchanged); -> the library's path."""
    top = os.path.join(tmp, name)
    for d in (os.path.join("madsim_amd", "csrc"), "include", os.path.join("tests", "emu")):
        shutil.copytree(os.path.join(ROOT, d), os.path.join(top, d), ignore=shutil.ignore_patterns("*.o", "*.so", "*.lock", "*.tmp", "__pycache__"))
    if name != "clean":
        _, rel, old, new, _, _ = MUTANTS[name]
        path = os.path.join(top, rel)
        src = open(path).read()
        assert src.count(old) == 1, (name, "the text to edit occurs", src.count(old), "times in", rel)
        open(path, "w").write(src.replace(old, new))
    here = os.path.join(top, "tests", "emu")
    lib = os.path.join(here, "libmadsim_emu.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-DMADSIM_EMU", "-x", "c++", "-I" + here, "-o", lib,
                           os.path.join(here, "emu_driver.cpp")])
    return lib


def child():
    """(in a process with MADSIM_EMU_LIB set) -> JSON rows [row, workload, carriers, differing seeds] over the matrix, trace rows included."""
    sys.path.insert(0, ROOT)
    from tests import emu
    from tests import build_cases as B
    rows = []
    for row in B.ROWS:
        for name, cs, n in B.count_differing(row, emu.run_batch):
            rows.append([row, name, list(cs), n])
    for row in B.TRACE_ROWS:
        for name, cs, w, cfg, lim, seeds in B.trace_truth(row):
            n = 0
            for seed, log, _, res in seeds:
                got_log, got = emu.trace_seed(w, seed, cfg, lim)
                n += tuple(int(x) for x in got) != res or got_log != log
            rows.append([row, name, list(cs), n])
    json.dump(rows, sys.stdout)


def run_suite(lib, workers):
    env = dict(os.environ, MADSIM_EMU_LIB=lib)
    cmd = [sys.executable, "-m", "pytest", "-q", "-p", "no:cacheprovider", "-n", str(workers)] + [os.path.join("tests", f + ".py") for f in SUITE]
    p = subprocess.run(cmd, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    tail = [ln for ln in p.stdout.splitlines() if ln.strip()]
    return p.returncode, tail[-1].strip("= ") if tail else ""


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--md", action="store_true", help="print the table as markdown")
    ap.add_argument("--skip-suite", action="store_true", help="the matrix cases only")
    ap.add_argument("-n", type=int, default=8, help="pytest-xdist workers per suite run")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child()
    sys.path.insert(0, ROOT)
    from tests import build_cases as B
    feats = B.row_feats()
    g_rows = {name for name, row in B.ROWS.items() if row.sel[5]}
    names = ["clean"] + list(MUTANTS)
    with tempfile.TemporaryDirectory(prefix="build_mutants.") as tmp:
        with ThreadPoolExecutor(len(names)) as pool:
            libs = dict(zip(names, pool.map(lambda n: make_copy(tmp, n), names)))

        def run(name):
            env = dict(os.environ, MADSIM_EMU_LIB=libs[name])
            out = subprocess.check_output([sys.executable, os.path.abspath(__file__), "--child"], env=env)
            return [(row, w, tuple(cs), n) for row, w, cs, n in json.loads(out)]
        with ThreadPoolExecutor(len(names)) as pool:
            rows = dict(zip(names, pool.map(run, names)))
        suite = {n: (0, "not run") for n in names} if args.skip_suite else {n: run_suite(libs[n], args.n) for n in names}
    ok = True
    if args.md:
        print("| Copy | The suite before the matrix | Matrix cases that differ / run | Rows that see it | Cases (seeds of 130; of 8 on a trace row) |")
        print("|---|---|---|---|---|")
    for name in names:
        what = "unchanged" if name == "clean" else MUTANTS[name][0]
        seen = [r for r in rows[name] if r[3]]
        by_row = {}
        for row, w, cs, n in seen:
            by_row.setdefault(row, []).append(f"{w}{'+' + '+'.join(cs) if cs else ''}: {n}")
        if name == "clean":
            good = not seen and suite[name][0] == 0
        else:
            _, _, _, _, bits, g_only = MUTANTS[name]
            family = {r for r, f in feats.items() if f & bits and (not g_only or r in g_rows)}
            good = bool(seen) and set(by_row) <= family and suite[name][0] == 0
            what += f" [family: {len(family)} rows]"
        ok &= good
        cases = "; ".join(f"{row}: {', '.join(v)}" for row, v in by_row.items()) or "none"
        if args.md:
            print(f"| {name}: {what} | {suite[name][1]} | {len(seen)} / {len(rows[name])} | {', '.join(by_row) or 'none'} | {cases} |")
        else:
            print(f"== {name}: {what}\n   suite: {suite[name][1]}\n   matrix: {len(seen)} of {len(rows[name])} cases differ{'' if good else '   <-- NOT as required'}")
            for row, v in by_row.items():
                print(f"   {row:16s} {', '.join(v)}")
    print(("\n" if args.md else "") + ("every mutant passes the earlier suite and is seen by the matrix on its own family's rows only; the unchanged copy is clean"
                                       if ok else "NOT as required"))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
