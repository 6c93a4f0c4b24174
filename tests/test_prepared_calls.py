"""What a prepared call is, held bit for bit: every row of ``tests/golden/prepared_calls.json`` (frozen by
``tests/golden/make_prepared_calls.py`` from the commit BEFORE the prepared forward and the step's block planner were restructured)
rebuilt by ``prepared_rows`` on CPU tensors — routes, refusals and their messages, workspace shapes, every field of the argument
blocks, the seeds drawn and how many.  Needs no GPU: nothing is launched."""
import json
import os

import pytest
import torch

import prepared_rows as pr
from chemprop_amd import engine

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "prepared_calls.json")


@pytest.fixture
def on_cpu(monkeypatch):
    monkeypatch.setattr(engine, "_require_device", lambda t, name: None)


def test_every_prepared_call_is_the_frozen_one(on_cpu):
    with open(GOLDEN) as f:
        frozen = json.load(f)
    rows = json.loads(pr.dumps(pr.build_rows()))   # (through JSON: tuples and lists, int and str keys compare as the file has them)
    assert sorted(rows) == sorted(frozen), "the rows of prepared_rows.py and of the frozen file differ: regenerate it from the parent commit"
    bad = [k for k in frozen if rows[k] != frozen[k]]
    for k in bad[:5]:   # (in full: a row of the file is what differs from its ``like`` row)
        got, want = pr.expand(rows, k), pr.expand(frozen, k)
        print(f"--- {k}\n  frozen: {json.dumps(want, sort_keys=True)}\n  now:    {json.dumps(got, sort_keys=True)}")
    assert not bad, f"{len(bad)} of {len(frozen)} prepared calls changed: {bad[:20]}"


def test_a_refused_step_row_that_names_the_row_kernels_drew_nothing(on_cpu):
    """The refusals the step raises itself (the rows-dropout gate of an undirected or an atom block) come before the seed draw."""
    specs = pr.step_specs()
    gate = [k for k in specs if "/p>0/refused/" in k and k.split("/")[0] in ("undirected", "atom")]
    assert len(gate) >= 6
    for k in gate:
        with torch.random.fork_rng(devices=[]):
            row = pr.step_row(specs[k])
        assert row["raises"] == "NotImplementedError" and "lives in the row kernels, which refuse it" in row["message"], k
        assert row["draws"] == 0, k


def test_pad_columns_of_the_workspaces_are_zero_at_d_h_30(on_cpu, monkeypatch):
    """``d_h = 30`` gives ``ldh = 32``: later kernels read the two pad columns of the edge and atom workspaces with vector loads, so
    they must be finite whatever the allocator hands back — here every ``torch.empty`` float tensor comes back full of NaN."""
    empty = torch.empty

    def nan_empty(*a, **kw):
        t = empty(*a, **kw)
        return t.fill_(float("nan")) if t.is_floating_point() else t

    for name, spec in (("inference", dict(h=30)), ("kept", dict(h=30, kw=dict(keep=True))), ("atom", dict(h=30, kw=dict(atom=True, route="general", keep=True)))):
        monkeypatch.setattr(torch, "empty", nan_empty)
        try:
            _, st, _ = pr.forward_call(spec)
        finally:
            monkeypatch.setattr(torch, "empty", empty)
        assert st.ldh == 32 and st.dims["d_h"] == 30
        edge_ws, atom_ws = st.refs[12], st.refs[13]
        assert edge_ws is not None and atom_ws is not None and edge_ws.numel() and atom_ws.numel(), name
        assert edge_ws.shape[-1] == 32 and atom_ws.shape[-1] == 32, name
        assert bool((edge_ws[..., 30:] == 0).all()) and bool((atom_ws[..., 30:] == 0).all()), name
