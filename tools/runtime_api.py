#!/usr/bin/env python3
"""The public surface of madsim_amd.runtime as text: str(inspect.signature(f)) of every public function the module defines and of every
public method of runtime.Context — names, parameter order and defaults.

    python tools/runtime_api.py            print it as JSON
    python tools/runtime_api.py --write    write tests/golden/runtime_api.json

tests/test_runtime_api.py holds the module against that file: a spelling that is derived from another one must keep its own signature.
"""
import inspect
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

GOLDEN = os.path.join(ROOT, "tests", "golden", "runtime_api.json")


def public_callables():
    """{"functions": {name: function}, "Context": {name: method}} of madsim_amd.runtime."""
    from madsim_amd import runtime
    own = lambda ns: {n: f for n, f in sorted(vars(ns).items()) if not n.startswith("_") and inspect.isfunction(f) and f.__module__ == runtime.__name__}      # noqa: E731
    return {"functions": own(runtime), "Context": own(runtime.Context)}


def surface():
    return {kind: {n: str(inspect.signature(f)) for n, f in fs.items()} for kind, fs in public_callables().items()}


if __name__ == "__main__":
    text = json.dumps(surface(), indent=1, sort_keys=True) + "\n"
    if "--write" in sys.argv[1:]:
        with open(GOLDEN, "w") as fh:
            fh.write(text)
    else:
        sys.stdout.write(text)
