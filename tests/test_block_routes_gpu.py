"""The module-path forwards of the four block classes held to the commit before they were consolidated:
``scripts/dump_block_routes.py`` asked that commit, on the MI355X, for four consecutive forwards of every case — the route, the plans
built, the replay state, a SHA-256 of every output and of every gradient, or the refusal in full
(``tests/golden/block_routes_parent.json``); the same cases on the working tree give the same records, string by string.  (The
compute kernels use no atomics; the script ran every case twice at that commit and found the two runs identical.)"""
import importlib.util
import json
import os

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def dump():
    spec = importlib.util.spec_from_file_location("dump_block_routes", os.path.join(HERE, os.pardir, "scripts", "dump_block_routes.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def parent():
    with open(os.path.join(HERE, "golden", "block_routes_parent.json")) as f:
        return json.load(f)


def test_the_table_reaches_every_route(dump, parent):
    """Not vacuous: the tile kernel for bond and atom messages, both row chains, a per-step route, a replayed forward, every case of
    the script, every block class in every mode, refusals — all in the parent's record."""
    assert dump.required_routes(parent) == []
    assert sorted(parent) == sorted(dump.case_name(c) for c in dump.cases())
    assert all(len(calls) == 4 for calls in parent.values())
    for b in dump.BLOCKS:
        for m in dump.MODES:
            assert f"{b}|{m}|base|own|14" in parent
    raised = {r["raises"] for calls in parent.values() for r in calls if "raises" in r}
    assert {"InvalidShapeError", "RuntimeError", "NotImplementedError"} <= raised
    assert any(len(r["plans"]) == 1 and r["plans"][0] == [True, True] for calls in parent.values() for r in calls)   # a tile plan
    assert any("grad" in r and r["grad"].get("V") for calls in parent.values() for r in calls)                         # an input gradient


@pytest.mark.gpu
def test_every_case_is_the_parents(gpu_device, dump, parent):
    different = []
    for c in dump.cases():
        name = dump.case_name(c)
        got = json.loads(json.dumps(dump.run_case(c, gpu_device)))
        for i, (g, w) in enumerate(zip(got, parent[name])):
            for k in sorted(set(g) | set(w)):
                if g.get(k) != w.get(k) or type(g.get(k)) is not type(w.get(k)):
                    different.append(f"{name} call {i} {k}: {g.get(k)!r} != {w.get(k)!r}")
    assert not different, "\n".join(different[:40])
