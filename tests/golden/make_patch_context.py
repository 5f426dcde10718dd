"""Records tests/golden/patch_context.json: which lines of the madsim sources bindings/rust/patches/0001-*.patch rests on.

For every file the patch touches, the fixture holds the sha256 of that file in the madsim checkout it was recorded from and
the sha256 of every context / removed line of the patch's hunks (stripped) that is a line of that file — digests only, no
source text.  tests/test_rust_binding.py checks the patch against it without a madsim checkout.

    python tests/golden/make_patch_context.py <madsim checkout>
"""
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
PATCH = os.path.join(ROOT, "bindings", "rust", "patches", "0001-builder-run_workload.patch")
OUT = os.path.join(HERE, "patch_context.json")


def digest(text):
    return hashlib.sha256(text.encode()).hexdigest()


def context_lines(patch_text):
    """(path, stripped line) for every non-blank context / removed line of every hunk, in patch order."""
    cur = None
    for line in patch_text.splitlines():
        if line.startswith("+++ b/"):
            cur = line[6:]
        elif cur is not None and (line.startswith(" ") or (line.startswith("-") and not line.startswith("---"))):
            if line[1:].strip():
                yield cur, line[1:].strip()
        elif line.startswith("diff --git"):
            cur = None


def main(checkout):
    files = {}
    for path, text in context_lines(open(PATCH).read()):
        if path not in files:
            src = open(os.path.join(checkout, path), "rb").read()
            files[path] = {"file_sha256": hashlib.sha256(src).hexdigest(),
                           "ref": {l.strip() for l in src.decode().splitlines()}, "lines": set()}
        if text in files[path]["ref"]:
            files[path]["lines"].add(digest(text))
        else:
            print(f"not a line of {path}: {text}", file=sys.stderr)
    out = {"patch": os.path.relpath(PATCH, ROOT),
           "files": {p: {"file_sha256": f["file_sha256"], "line_sha256": sorted(f["lines"])} for p, f in sorted(files.items())}}
    with open(OUT, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main(sys.argv[1])
