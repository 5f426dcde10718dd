"""The public surface of madsim_amd.runtime held against tests/golden/runtime_api.json (tools/runtime_api.py --write): every public function
of the module and every public method of runtime.Context with str(inspect.signature(...)) — no name lost, none added, no parameter or
default moved — and a docstring on each.  The module-level, Context and _multi spellings of an operation are derived from one definition;
this is what says each of them still reads as it did when every one was written out."""
import importlib.util
import json
import os

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


def _tool():
    spec = importlib.util.spec_from_file_location("runtime_api", os.path.join(HERE, "..", "tools", "runtime_api.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


TOOL = _tool()
GOLDEN = json.load(open(os.path.join(HERE, "golden", "runtime_api.json")))


def test_golden_counts():
    assert (len(GOLDEN["functions"]), len(GOLDEN["Context"])) == (55, 22)


@pytest.mark.parametrize("kind", ["functions", "Context"])
def test_no_name_lost_or_added(kind):
    assert sorted(TOOL.surface()[kind]) == sorted(GOLDEN[kind])


@pytest.mark.parametrize("kind,name", [(k, n) for k in ("functions", "Context") for n in sorted(GOLDEN[k])])
def test_signature_and_docstring(kind, name):
    f = TOOL.public_callables()[kind][name]
    assert TOOL.surface()[kind][name] == GOLDEN[kind][name]
    assert f.__name__ == name
    assert (f.__doc__ or "").strip(), f"{kind}: {name} has no docstring"
