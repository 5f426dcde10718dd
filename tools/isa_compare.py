#!/usr/bin/env python3
"""Compare the gfx950 code of two sim_kernel.o builds kernel by kernel (no GPU needed).

Each object's device code is unbundled and disassembled with llvm-objdump; per function symbol, the instruction text is kept with
addresses, encodings, branch-target labels and pc-relative displacements (the literal added to an s_getpc_b64 result: a call of an
out-of-line function, a long branch) stripped, so code that moved as a whole still compares equal — the callee is a symbol of its own
and is compared like every other.  (What that leaves unseen: a call retargeted to ANOTHER callee, everything else equal, reads `same`.  The
displacement is not resolved to its target's name here.)  Prints one line per
symbol: `same`, `DIFFERENT` (with the count of differing lines) or `only in old / new`.  Exit status 1 if a symbol of the old object
is missing or different in the new one.

    python tools/isa_compare.py OLD/sim_kernel.o madsim_amd/csrc/sim_kernel.o
"""
import os
import re
import subprocess
import sys
import tempfile

B = "/opt/rocm/lib/llvm/bin"


def functions(obj, tmp):
    fat, co = os.path.join(tmp, "k.fat"), os.path.join(tmp, "k.co")
    subprocess.check_call(["objcopy", "-O", "binary", "--only-section=.hip_fatbin", obj, fat])
    targets = subprocess.check_output([f"{B}/clang-offload-bundler", "--list", "--type=o", f"--input={fat}"], text=True).split()
    t = next(x for x in targets if "gfx950" in x)
    subprocess.check_call([f"{B}/clang-offload-bundler", "--unbundle", "--type=o", f"--input={fat}", f"--targets={t}", f"--output={co}"])
    dis = subprocess.check_output([f"{B}/llvm-objdump", "-d", "--no-show-raw-insn", "--no-leading-addr", co], text=True)
    out, cur, pc = {}, None, None                            # pc: the register that holds the low half of the last s_getpc_b64
    for ln in dis.splitlines():
        m = re.match(r"^(?:[0-9a-f]+ )?<(.+)>:$", ln)
        if m:
            cur = m.group(1); out[cur] = []; continue
        if cur is None or not ln.strip():
            continue
        s = re.sub(r"//.*$", "", ln).strip()
        s = re.sub(r"<[^>]*>", "<L>", s)                     # branch targets: symbolic
        s = re.sub(r"\b0x[0-9a-f]+\b(?=\s*<L>)", "", s)
        if s:
            m = re.match(r"s_getpc_b64 s\[(\d+):\d+\]$", s)
            if pc is not None and re.match(r"s_add_u32 s%s, s%s, 0x[0-9a-f]+$" % (pc, pc), s):
                s = "s_add_u32 s%s, s%s, <pcrel>" % (pc, pc)
            pc = m.group(1) if m else None
            out[cur].append(s)
    for f in out.values():                                   # alignment padding behind a function (s_nop, the `...` of a zero run)
        while f and f[-1] in ("s_nop 0", "..."):
            f.pop()
    return out


def short(sym):
    return re.sub(r"EEEEEvNS_7KParamsE$", "", sym.replace("_ZN8madsim_k10sim_kernelINS_7VariantIL", "L"))


def main():
    old_o, new_o = sys.argv[1], sys.argv[2]
    with tempfile.TemporaryDirectory() as d:
        os.makedirs(os.path.join(d, "a")); os.makedirs(os.path.join(d, "b"))
        old, new = functions(old_o, os.path.join(d, "a")), functions(new_o, os.path.join(d, "b"))
    bad = 0
    for sym in sorted(set(old) | set(new), key=short):
        if sym not in new:
            print(f"{short(sym):48s} only in old"); bad += 1
        elif sym not in old:
            print(f"{short(sym):48s} only in new ({len(new[sym])} instructions)")
        elif old[sym] == new[sym]:
            print(f"{short(sym):48s} same ({len(old[sym])} instructions)")
        else:
            n = sum(1 for x, y in zip(old[sym], new[sym]) if x != y) + abs(len(old[sym]) - len(new[sym]))
            print(f"{short(sym):48s} DIFFERENT ({n} lines of {len(old[sym])})"); bad += 1
    print(f"{len(old)} functions in old, {len(new)} in new; {bad} of the old missing or different")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
