#!/usr/bin/env python3
"""Write tests/golden/host_plan.json: what validate, make_geometry and build_tables (madsim_amd/csrc/geometry.h) answer over the corpus of
tests/host_plan_cases.py.  Run it on the commit whose answers are the truth — before a change that is meant to keep them — and commit the
file; tests/test_host_plan.py replays the corpus against it.  CPU only.

    python tools/host_plan_record.py                 # record, check that every reachable fail( message of the two functions occurs, write
    python tools/host_plan_record.py --check         # the same without writing: exit status 1 when the record would differ or a rule is left out
    python tools/host_plan_record.py --verbose FILE  # also one line per answer into FILE (diff two of them to find what a cell's digest hides)
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tests import host_plan_cases as HP  # noqa: E402


def dumps(rec):
    """One entry a line."""
    return json.dumps(rec, separators=(",", ":")).replace('},"', '},\n"').replace('],"', '],\n"').replace('","', '",\n"').replace(':{"', ':{\n"') + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--check", action="store_true")
    ap.add_argument("--verbose", metavar="FILE")
    args = ap.parse_args()
    log = open(args.verbose, "w") if args.verbose else None
    rec, msgs = HP.record(log)
    lits = HP.fail_literals()
    missing = HP.uncovered(msgs)
    n = sum(len(v) for v in lits.values())
    print(f"{sum(e[0] for e in rec['accepted'].values())} accepted workloads in {len(rec['accepted'])} entries, {sum(e[0] for e in rec['refused'].values())} mutants of "
          f"{len(rec['refused'])} bases, {len(rec['messages'])} distinct answers")
    print(f"fail( literals of validate / make_geometry: {n}, unreachable by rule {len(HP.UNREACHABLE)}, uncovered {len(missing)}")
    for fn, lit in missing:
        print(f"  NOT COVERED  {fn}: {lit!r}")
    for lit, why in HP.UNREACHABLE.items():
        print(f"  unreachable  {lit!r}: {why}")
    text = dumps(rec)
    if args.check:
        same = os.path.exists(HP.GOLDEN) and open(HP.GOLDEN).read() == text
        print("record", "unchanged" if same else "DIFFERS")
        return 1 if missing or not same else 0
    if missing:
        return 1
    with open(HP.GOLDEN, "w") as f:
        f.write(text)
    print(f"wrote {HP.GOLDEN}: {len(text)} bytes")
    return 0


if __name__ == "__main__":
    sys.exit(main())
