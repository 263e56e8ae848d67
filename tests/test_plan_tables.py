"""CPU: the host-side planner decides what it decided before.  tests/golden/plan_tables.json.gz records,
for a matrix of engine configurations, the arena layout, the planned launches of every flag set with
their FLOPs / bytes, the data-parallel buckets and the acting geometry (tests/golden/make_plan_tables.py
generated it; no GPU is needed: the engine is bound to an address that is never dereferenced).  This
regenerates the same structure from the current build and asserts equality.  Floats are compared by
repr: a last-bit difference means a flops / bytes expression was reassociated.  A configuration the
fixture records as refused must be refused with the same code; nothing is skipped."""
import gzip
import importlib.util
import json
import os

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("make_plan_tables", os.path.join(HERE, "golden", "make_plan_tables.py"))
M = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(M)


@pytest.fixture(scope="module")
def recorded():
    with gzip.open(M.FIXTURE, "rb") as f:
        return json.loads(f.read().decode())


def _first_difference(want, got, path=""):
    if type(want) is not type(got):
        return "%s: %r != %r" % (path, want, got)
    if isinstance(want, dict):
        if sorted(want) != sorted(got):
            return "%s: keys %s != %s" % (path, sorted(want), sorted(got))
        for k in sorted(want):
            d = _first_difference(want[k], got[k], path + "/" + k)
            if d:
                return d
        return None
    if isinstance(want, list) and len(want) == len(got):
        for i, (a, b) in enumerate(zip(want, got)):
            d = _first_difference(a, b, "%s[%d]" % (path, i))
            if d:
                return d
        return None
    return None if want == got else "%s: %r != %r" % (path, want, got)


def test_fixture_covers_the_matrix(recorded):
    assert sorted(recorded) == sorted(M.GROUPS)
    for group in M.GROUPS:
        names = {"%s/%s/clip%d" % (n["name"], a, c) for n in M.nets(group) for a in M.ALGOS for c in (0, 1)}
        assert set(recorded[group]) == names, group
    default = recorded["default"]
    assert len(default) >= 198
    # every flag set of every created engine is there, as a launch list or as the refusal's code
    for name, t in default.items():
        assert "create" in t or sorted(t["steps"]) == sorted(str(f) for f in M.FLAGS), name
    # the non-default builders are what the variables select: they differ from the default plan
    for group in M.GROUPS[1:]:
        for name, t in recorded[group].items():
            assert t["steps"] != default[name]["steps"], (group, name)


@pytest.mark.parametrize("group", M.GROUPS)
def test_plan_tables_match_the_recorded_plan(monkeypatch, recorded, group):
    for k in [k for k in os.environ if k.startswith("DQNX_") and k != "DQNX_LIB"]:
        monkeypatch.delenv(k)
    if group != "default":
        var, val = group.split("=")
        monkeypatch.setenv(var, val)
    got = json.loads(json.dumps(M.tables(group, setenv=False)))   # (tuples and int keys as JSON holds them)
    want = recorded[group]
    assert sorted(got) == sorted(want)
    diffs = [d for d in (_first_difference(want[n], got[n], n) for n in sorted(want)) if d]
    assert not diffs, "%d of %d configurations differ; first: %s" % (len(diffs), len(want), diffs[:5])
