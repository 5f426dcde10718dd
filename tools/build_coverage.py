#!/usr/bin/env python3
"""Which opcodes, and which lines of the kernel, does a pytest selection run on which kernel build?  CPU only, not a test.

sim_kernel is one source compiled into the builds of MADSIM_FOR_EACH_VARIANT; merged over all of them a suite's line coverage of
kernel/k_*.h says nothing about any one build.  This tool

  1. compiles the host emulation (tests/emu/emu_driver.cpp) with `g++ -O0 --coverage -DMADSIM_EMU_OPS` into a scratch directory — plain gcov
     on host code; -DMADSIM_EMU_OPS turns the kernel's existing region markers into per-build opcode notes (tests/emu/emu_shim.h), the kernel
     sources themselves are compiled as they stand;
  2. runs the selection in a child pytest with MADSIM_EMU_LIB naming that library (every process of the run leaves its notes and its .gcda);
  3. reduces `gcov --json-format` per template instantiation, i.e. per Variant<...>;
  4. prints the matrix build x opcode — `#` dispatched on that build, `.` compiled into it and never dispatched, blank: not compiled — and per
     build the lines of kernel/k_*.h never executed, as a count and (--lines FILE) as ranges.

    python tools/build_coverage.py [--md] [--lines FILE] [--json FILE] [--keep DIR] [-n WORKERS] -- PYTEST ARGS...
    python tools/build_coverage.py --md -- tests -m "not gpu" --deselect tests/test_emu_build_matrix.py       (the suite without the matrix)

Exit status: pytest's."""
import argparse
import glob
import json
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
EMU = os.path.join(ROOT, "tests", "emu")


def compile_lib(work):
    lib = os.path.join(work, "libmadsim_emu_cov.so")
    subprocess.check_call(["g++", "-O0", "--coverage", "-std=c++17", "-fPIC", "-shared", "-DMADSIM_EMU", "-DMADSIM_EMU_OPS", "-x", "c++", "-I" + EMU,
                           "-o", lib, os.path.join(EMU, "emu_driver.cpp")], cwd=work)
    return lib


def variant_table(lib):
    import ctypes as C
    L = C.CDLL(lib)
    tab = (C.c_int32 * (6 * 128))()
    n = L.madsim_emu_variants(tab, 128)
    return [tuple(tab[6 * i:6 * i + 6]) for i in range(n)]


def run_pytest(lib, work, args, workers):
    env = dict(os.environ, MADSIM_EMU_LIB=lib, MADSIM_EMU_OPS_OUT=os.path.join(work, "ops"))
    cmd = [sys.executable, "-m", "pytest", "-q", "-p", "no:cacheprovider"] + (["-n", str(workers)] if workers else []) + args
    p = subprocess.run(cmd, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    tail = [ln for ln in p.stdout.splitlines() if ln.strip()]
    return p.returncode, tail[-1] if tail else ""


def op_counts(work, n_rows):
    from madsim_amd import _abi as A
    n_ops = max(A.OP.values()) + 1
    tot = [[0] * n_ops for _ in range(n_rows)]
    for path in glob.glob(os.path.join(work, "ops.*")):
        for i, ln in enumerate(open(path)):
            for k, v in enumerate(ln.split()):
                tot[i][k] += int(v)
    return tot


def variant_of(demangled):
    m = re.search(r"Variant<(true|false), (true|false), (-?\d+), (\d+), (true|false), (true|false)>", demangled or "")
    if not m:
        return None
    b = lambda x: int(x == "true")      # noqa: E731
    return (b(m.group(1)), b(m.group(2)), int(m.group(3)), int(m.group(4)), b(m.group(5)), b(m.group(6)))


def line_coverage(work):
    """{variant row: {(file, line): executed}} over kernel/k_*.h, from gcov's JSON (one record per line and function instance)."""
    gcda = glob.glob(os.path.join(work, "*.gcda"))
    assert len(gcda) == 1, gcda
    out = subprocess.check_output(["gcov", "--json-format", "--stdout", os.path.basename(gcda[0])], cwd=work)
    cov = {}
    for doc in out.decode().splitlines():
        if not doc.strip():
            continue
        for f in json.loads(doc)["files"]:
            name = os.path.basename(f["file"])
            if not (name.startswith("k_") and name.endswith(".h") and os.sep + "kernel" + os.sep in f["file"]):
                continue
            which = {fn["name"]: variant_of(fn.get("demangled_name")) for fn in f["functions"]}
            for ln in f["lines"]:
                v = which.get(ln.get("function_name"))
                if v is None:
                    continue
                key = (name, ln["line_number"])
                d = cov.setdefault(v, {})
                d[key] = d.get(key, False) or ln["count"] > 0
    return cov


def ranges(keys):
    """[(file, first, last)] of sorted (file, line) keys, consecutive lines joined."""
    out = []
    for f, n in sorted(keys):
        if out and out[-1][0] == f and out[-1][2] + 1 == n:
            out[-1][2] = n
        else:
            out.append([f, n, n])
    return out


def name_of(v):
    b = lambda x: "true" if x else "false"      # noqa: E731
    return f"Variant<{b(v[0])}, {b(v[1])}, {v[2]}, {v[3]}, {b(v[4])}, {b(v[5])}>"


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--md", action="store_true", help="print markdown (profiles/build_matrix.md)")
    ap.add_argument("--lines", help="write per build the ranges of kernel lines never executed to this file")
    ap.add_argument("--json", help="write the whole result to this file")
    ap.add_argument("--keep", help="use this directory for the build and the coverage data, and keep it")
    ap.add_argument("-n", type=int, default=8, help="pytest-xdist workers (0: none)")
    ap.add_argument("pytest_args", nargs=argparse.REMAINDER)
    args = ap.parse_args()
    sel = [a for a in args.pytest_args if a != "--"] or ["tests", "-m", "not gpu"]
    from madsim_amd import _abi as A
    from tests import build_cases as B
    op_name = {v: k for k, v in A.OP.items()}
    n_ops = max(op_name) + 1
    with tempfile.TemporaryDirectory(prefix="build_coverage.") as tmp:
        work = args.keep or tmp
        os.makedirs(work, exist_ok=True)
        for old in glob.glob(os.path.join(work, "*.gcda")) + glob.glob(os.path.join(work, "ops.*")):
            os.unlink(old)
        lib = compile_lib(work)
        table = variant_table(lib)
        rc, summary = run_pytest(lib, work, sel, args.n)
        ops = op_counts(work, len(table))
        cov = line_coverage(work)
    result = []
    for i, v in enumerate(table):
        compiled = {A.OP[o] for o in B.compiled_ops(v[3])}
        lines = cov.get(v, {})
        never = [k for k, hit in lines.items() if not hit]
        result.append(dict(build=name_of(v), row=list(v), reached=[k for k in range(n_ops) if ops[i][k]], compiled=sorted(compiled),
                           lines=len(lines), lines_never=len(never), never=ranges(never)))
    tick = "`" if args.md else ""
    print(f"selection: {tick}{' '.join(sel)}{tick} -- {summary}\n")
    print("```" if args.md else "", end="\n" if args.md else "")
    print(f"{'opcode':48s}" + "".join(str(k // 10) for k in range(n_ops)))
    print(f"{'':48s}" + "".join(str(k % 10) for k in range(n_ops)))
    for r in result:
        cells = "".join("#" if k in r["reached"] else "." if k in r["compiled"] else " " for k in range(n_ops))
        print(f"{r['build']:48s}{cells}")
    print("```" if args.md else "")
    print("| Build | Opcodes dispatched / compiled | Compiled, never dispatched | Kernel lines never executed / instrumented |" if args.md else "")
    print("|---|---|---|---|" if args.md else "", end="\n" if args.md else "")
    for r in result:
        missing = [op_name[k] for k in r["compiled"] if k not in r["reached"]]
        stray = [op_name.get(k, str(k)) for k in r["reached"] if k not in r["compiled"]]
        what = ", ".join(missing) if missing else "none"
        if stray:
            what += " (dispatched though not compiled: " + ", ".join(stray) + ")"
        if not r["reached"]:
            what = "NEVER RUN"
        if args.md:
            print(f"| `{r['build']}` | {len(set(r['reached']) & set(r['compiled']))} / {len(r['compiled'])} | {what} | {r['lines_never']} / {r['lines']} |")
        else:
            print(f"{r['build']:48s} {len(r['reached']):2d} / {len(r['compiled']):2d}  lines never {r['lines_never']:4d} / {r['lines']:4d}  {what}")
    run = sum(1 for r in result if r["reached"])
    pairs = sum(len(set(r["reached"]) & set(r["compiled"])) for r in result)
    total = sum(len(r["compiled"]) for r in result)
    print(f"\nbuilds run: {run} of {len(result)}; (build, opcode) pairs dispatched: {pairs} of {total} compiled")
    if args.lines:
        with open(args.lines, "w") as f:
            f.write(f"kernel lines never executed, per build -- selection: {' '.join(sel)} -- {summary}\n")
            for r in result:
                f.write(f"\n{r['build']}: {r['lines_never']} of {r['lines']}\n")
                by = {}
                for fn, a, b in r["never"]:
                    by.setdefault(fn, []).append(f"{a}" if a == b else f"{a}-{b}")
                for fn, rs in by.items():
                    f.write(f"  {fn}: {' '.join(rs)}\n")
    if args.json:
        json.dump(dict(selection=sel, summary=summary, builds=result), open(args.json, "w"))
    return rc


if __name__ == "__main__":
    sys.exit(main())
