"""K0 from the batch vector, every planner kernel against ONE statement of its output (``oracle.collate_numpy.batch_tile_plan``),
bit for bit (integer work): header words 0 / 6 / 7 / 8 and every slot of ``mtile_row`` / ``mtile_atom``.

    k_prepare_tiles_batch_multi       dmpnn_prepare_tiles (default, small batch)           GraphPlan(light="tiles", batch=...)
      ... with the weight pre-split   dmpnn_forward_tiles                                  launch="defer" + engine.forward
    k_prepare_tiles_batch             dmpnn_prepare_tiles under DMPNN_K0_SINGLE=1, or where the multi-workgroup scratch does not fit
    k_prepare_tiles_batch_split       dmpnn_forward_tiles under DMPNN_K0_SINGLE=1
    k_large_bounds / _blocks / _finish  dmpnn_prepare_tiles beyond the single-workgroup plan
    (the same, inside)                dmpnn_prepare_with_batch: the full plan with molecule tiles

and the bounds table K0 writes for the head inside ``dmpnn_train_step`` through the losses and gradients of the one-call step.
Invalid batch vectors must set the statement's error bits and make the tile forward NaN, never a finite wrong number.
"""
from __future__ import annotations

import numpy as np
import pytest
import torch

from conftest import parity_err

pytestmark = pytest.mark.gpu

D_H, D_V, D_E = 64, 72, 14


def _qm9_sizes(n, seed):
    from chemprop_amd import synth

    return [(len(m.V), int(m.edge_index.shape[1])) for m in synth.random_molgraphs(n, "qm9", seed=seed)]


def _graph(sizes, seed):
    """A batch of molecules of the given (atoms, directed edges) sizes, edges in molecule order (collate.py:48-62), random bonds
    inside each molecule; a molecule of 0 atoms is an id without atoms.  -> CPU tensors (batch, edge_index, rev, V, E)."""
    rng = np.random.default_rng(seed)
    batch, src, dst = [], [], []
    a0 = 0
    for m, (na, ne) in enumerate(sizes):
        batch += [m] * na
        for _ in range(ne // 2):
            u = int(rng.integers(na))
            v = (u + 1 + int(rng.integers(na - 1))) % na
            src += [a0 + u, a0 + v]
            dst += [a0 + v, a0 + u]
        a0 += na
    nE = len(src)
    return dict(batch=torch.tensor(batch, dtype=torch.int64), edge_index=torch.tensor([src, dst], dtype=torch.int64).reshape(2, nE),
                rev=torch.from_numpy(np.arange(nE, dtype=np.int64) ^ 1),
                V=torch.from_numpy(rng.standard_normal((a0, D_V)).astype(np.float32)),
                E=torch.from_numpy(rng.standard_normal((nE, D_E)).astype(np.float32)), n_mols=len(sizes))


def _put(sizes, at):
    s = list(sizes)
    for i, v in at.items():
        s[i] = v
    return s


def _largest_small(extra_atoms=0):
    """512 molecules of 9 atoms / 20 directed edges (10240 edges: the single-workgroup plan's edge limit), then lone atoms up to
    the largest atom count small_plan_fits accepts at that edge count (+ extra_atoms)."""
    from chemprop_amd.engine import small_plan_fits

    nE = 10240
    nV = 512 * 9
    while small_plan_fits(nV + 1, nE):
        nV += 1
    return [(9, 20)] * 512 + [(1, 0)] * (nV - 512 * 9 + extra_atoms)


OVER, LIMIT = (33, 50), (32, 48)
SMALL_CASES = {
    "qm9_512": lambda: _qm9_sizes(512, 1),
    **{f"qm9_{n}": (lambda n=n: _qm9_sizes(n, n)) for n in (63, 64, 65, 127, 128, 129)},
    "tile_limits": lambda: _put(_qm9_sizes(130, 2), {0: OVER, 5: LIMIT, 62: LIMIT, 63: OVER, 64: OVER, 70: LIMIT, 100: OVER,
                                                     101: (40, 60), 129: OVER}),
    "single_atom_runs": lambda: _put(_qm9_sizes(200, 3), {**{i: (1, 0) for i in range(10)}, **{i: (1, 0) for i in range(58, 71)},
                                                          **{i: (1, 0) for i in range(188, 200)}}),
    "only_single_atoms": lambda: [(1, 0)] * 300,
    "one_molecule": lambda: [(20, 40)],
    "one_atom": lambda: [(1, 0)],
    "gap_ids": lambda: [(2, 2), (0, 0)] * 3 + _put(_qm9_sizes(150, 4), {1: (0, 0), 2: (0, 0), 64: (0, 0), 100: (0, 0)}) + [(0, 0)] * 3,
    "largest_small_plan": _largest_small,
}
LARGE_CASES = {
    "qm9_2000": lambda: _qm9_sizes(2000, 5),
    "first_refused": lambda: _largest_small(1),
    "irregular": lambda: _put(_qm9_sizes(2100, 6), {0: OVER, 63: OVER, 64: OVER, 65: OVER, 700: LIMIT, 2099: OVER,
                                                     **{i: (1, 0) for i in range(100, 140)}, **{i: (0, 0) for i in (300, 301, 1024)}})
                              + [(0, 0)] * 2,
}


def _invalid(kind, g):
    """One defect in a valid batch (CPU tensors, modified copies)."""
    b, ei, rev = g["batch"].clone(), g["edge_index"].clone(), g["rev"].clone()
    nV = b.numel()
    last = int(b[-1])
    if kind == "advisor":            # [..., 5, 5, 1, 1]: the last molecule's id below earlier ones (clamped ids would read as sorted)
        b[b == last] = 1
    elif kind == "decrease":         # [.., 3, 3, 2, 2, 5, ..]: every id in range
        b[b == 4] = 2
    elif kind == "negative":
        b[nV // 2] = -1
    elif kind == "beyond":
        b[nV // 2] = nV + 5
    elif kind == "dst_range":
        ei[1, ei.shape[1] // 2] = nV + 3
    elif kind == "edge_order":       # sorted atoms; the edges of molecules 4 and 5 swapped (reverse pairs stay consistent)
        m_of_e = b[ei[1]]
        e4, e5 = torch.nonzero(m_of_e == 4).flatten(), torch.nonzero(m_of_e == 5).flatten()
        assert len(e4) and len(e5)
        perm = torch.arange(ei.shape[1])
        lo = int(e4[0])
        perm[lo:lo + len(e5) + len(e4)] = torch.cat([e5, e4])
        inv = torch.empty_like(perm)
        inv[perm] = torch.arange(perm.numel())
        ei, rev = ei[:, perm], inv[rev[perm]]
    return dict(g, batch=b, edge_index=ei, rev=rev)


INVALID = ("advisor", "decrease", "negative", "beyond", "dst_range", "edge_order")


@pytest.fixture(params=["multi", "single"])
def k0(request, monkeypatch):
    monkeypatch.setenv("DMPNN_K0_SINGLE", "1" if request.param == "single" else "0")
    return request.param


def _dev(g, dev):
    return {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in g.items()}


def _weights(dev):
    torch.manual_seed(7)
    W_i = (torch.randn(D_H, D_V + D_E) * 0.1).to(dev)
    W_h = (torch.randn(D_H, D_H) * 0.1).to(dev)
    W_o = (torch.randn(D_H, D_V + D_H) * 0.1).to(dev)
    b_o = (torch.randn(D_H) * 0.1).to(dev)
    return W_i, W_h, W_o, b_o


def _forward(plan, g, dev):
    from chemprop_amd import engine

    with torch.no_grad():
        out, _ = engine.forward(plan, g["V"], g["E"], *_weights(dev), depth=3, act="relu", route="mega")
    torch.cuda.synchronize()
    return out


def _multi_fits(nV, nE):
    """launch_prepare_tiles_batch: the multi-workgroup K0's scratch (multi_scratch, dmpnn_prepare.hip) below the row-tile table."""
    from chemprop_amd import _lib
    import ctypes as C

    off = (C.c_int64 * 15)()
    assert _lib.load().dmpnn_plan_layout(nV, nE, off) == 0
    a4 = lambda x: (x + 3) & ~3
    n_bounds = (max(nV, nE) + 1 + 1023) // 1024
    o = (off[0] + 1) & ~1
    o += 2 * a4(2 * (nV + 2)) + a4(2 * n_bounds)
    return o <= off[9]


def _check_tables(arr, want, what, light=2):
    hdr = arr["hdr"].numpy()
    assert (int(hdr[0]) & want["flags_mask"]) == want["flags"], (what, int(hdr[0]), want["flags"])
    if light is not None:
        assert int(hdr[7]) == light, what
    if not want["valid"]:
        return
    assert int(hdr[6]) == want["n_tiles"] and int(hdr[8]) == want["n_spill"], (what, hdr[6], want["n_tiles"], hdr[8], want["n_spill"])
    mr, ma = arr["mtile_row"].numpy(), arr["mtile_atom"].numpy()
    assert np.array_equal(mr, want["mtile_row"]), (what, np.flatnonzero(mr != want["mtile_row"])[:8])
    assert np.array_equal(ma, want["mtile_atom"]), (what, np.flatnonzero(ma != want["mtile_atom"])[:8])


def _statement(g, plan, planner):
    from oracle import collate_numpy as oc

    return oc.batch_tile_plan(g["batch"].numpy(), g["edge_index"][1].numpy(), max_mtiles=int(plan._offsets()[14]), planner=planner)


def _small_plans(g, gd, dev, what):
    """Both small-batch entry points on one batch: the plan alone, and K0 inside the forward (with the weight pre-split)."""
    from chemprop_amd.engine import GraphPlan

    nV = gd["V"].shape[0]
    p1 = GraphPlan(gd["edge_index"], gd["rev"], nV, light="tiles", batch=gd["batch"])
    assert p1.tiles_only and not p1.any_size
    want = _statement(g, p1, "small")
    _check_tables(p1.arrays(), want, what + "/prepare_tiles")
    if gd["E"].shape[0] == 0:
        return want, None, None
    out1 = _forward(p1, gd, dev)
    p2 = GraphPlan(gd["edge_index"], gd["rev"], nV, light="tiles", batch=gd["batch"], launch="defer")
    assert p2.pending is not None
    out2 = _forward(p2, gd, dev)
    assert p2.pending is None
    _check_tables(p2.arrays(), want, what + "/forward_tiles")
    return want, out1, out2


@pytest.mark.parametrize("case", list(SMALL_CASES))
def test_small_planners_vs_statement(case, k0, gpu_device):
    from chemprop_amd.engine import small_plan_fits

    g = _graph(SMALL_CASES[case](), seed=11)
    nV, nE = g["V"].shape[0], g["E"].shape[0]
    assert small_plan_fits(nV, nE)
    if case == "only_single_atoms":
        assert not _multi_fits(nV, nE), "this batch is the one that reaches the single-workgroup kernel in the default setting"
    if case in ("qm9_512", "largest_small_plan"):
        assert _multi_fits(nV, nE)
    want, out1, out2 = _small_plans(g, _dev(g, gpu_device), gpu_device, f"{case}/{k0}")
    assert want["valid"]
    if out1 is not None:
        assert torch.isfinite(out1).all() and torch.equal(out1, out2), case


@pytest.mark.parametrize("case", list(LARGE_CASES))
def test_large_planners_vs_statement(case, gpu_device):
    from chemprop_amd import _lib
    from chemprop_amd.engine import GraphPlan, small_plan_fits

    g = _graph(LARGE_CASES[case](), seed=12)
    gd = _dev(g, gpu_device)
    nV, nE = g["V"].shape[0], g["E"].shape[0]
    assert not small_plan_fits(nV, nE)
    lean = GraphPlan(gd["edge_index"], gd["rev"], nV, light="tiles", batch=gd["batch"])
    assert lean.tiles_only and lean.any_size
    want = _statement(g, lean, "large")
    assert want["valid"]
    _check_tables(lean.arrays(), want, case + "/large")
    assert torch.isfinite(_forward(lean, gd, gpu_device)).all()
    assert _lib.load().dmpnn_full_plan_keeps_tiles(nV, nE)
    full = GraphPlan(gd["edge_index"], gd["rev"], nV, batch=gd["batch"])
    assert full.any_size and not full.tiles_only
    arr = full.arrays()
    assert not (int(arr["hdr"][0]) & 8)
    _check_tables(arr, dict(want, flags=0, flags_mask=8), case + "/with_batch", light=0)


@pytest.mark.parametrize("kind", INVALID)
def test_small_planners_on_invalid_batches(kind, k0, gpu_device):
    g = _invalid(kind, _graph(_qm9_sizes(100, 8), seed=13))
    gd = _dev(g, gpu_device)
    want, out1, out2 = _small_plans(g, gd, gpu_device, f"{kind}/{k0}")
    assert not want["valid"] and want["flags"] & (2 | 8)
    assert torch.isnan(out1).all() and torch.isnan(out2).all(), kind


@pytest.mark.parametrize("kind", INVALID)
def test_large_planners_on_invalid_batches(kind, gpu_device):
    from chemprop_amd.engine import GraphPlan

    g = _invalid(kind, _graph(_qm9_sizes(2000, 9), seed=14))
    gd = _dev(g, gpu_device)
    nV = g["V"].shape[0]
    lean = GraphPlan(gd["edge_index"], gd["rev"], nV, light="tiles", batch=gd["batch"])
    assert lean.any_size
    want = _statement(g, lean, "large")
    assert not want["valid"] and want["flags"] == 8 | 16
    _check_tables(lean.arrays(), want, kind + "/large")
    assert torch.isnan(_forward(lean, gd, gpu_device)).all(), kind
    full = GraphPlan(gd["edge_index"], gd["rev"], nV, batch=gd["batch"])
    assert full.any_size
    assert int(full.arrays()["hdr"][0]) & 8, kind   # (the full plan keeps only this bit of the tile planner's header)


# ---- the bounds table K0 writes for the head, through the one-call training step ----
STEP_CASES = {
    "gap_ids": lambda: [(2, 2), (0, 0)] * 3 + _put(_qm9_sizes(120, 21), {5: (0, 0), 64: (0, 0), 65: (0, 0)}),
    "trailing_empty": lambda: _qm9_sizes(100, 22) + [(0, 0)] * 5,
    "single_atom_runs": lambda: _put(_qm9_sizes(150, 23), {**{i: (1, 0) for i in range(6)}, **{i: (1, 0) for i in range(60, 70)},
                                                           **{i: (1, 0) for i in range(144, 150)}}),
}


def _step_run(cfg, g, dev, y):
    """Two validated regular batches, then the case batch on the tile plan.  -> (state before step 3, loss, gradients, trainer)"""
    from chemprop_amd import synth
    from chemprop_amd.data import BatchMolGraph
    from chemprop_amd.model import FusedTrainer
    from test_model import build_mirror

    torch.manual_seed(31)
    model = build_mirror(cfg).to(dev).train()
    tr = FusedTrainer(model, lr=1e-3, tile_plan=True)
    for i in range(2):
        wb = synth.random_batch(64, "qm9", seed=40 + i)
        wb.to(dev)
        tr.step(wb, torch.randn(64, 1, generator=torch.Generator().manual_seed(i)).to(dev))
    torch.cuda.synchronize()
    state = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    gd = _dev(g, dev)
    bmg = BatchMolGraph.from_tensors(gd["V"], gd["E"], gd["edge_index"], gd["rev"], gd["batch"], size=g["n_mols"])
    out = tr.step(bmg, y.to(dev))
    torch.cuda.synchronize()
    assert tr.last_route == "mega16" and tr._last_plan_tiles
    return state, out[0].detach().cpu().clone(), [v.detach().cpu().clone() for v in tr.sync.views], model


@pytest.mark.parametrize("case,agg", [("gap_ids", "sum"), ("gap_ids", "mean"), ("trailing_empty", "norm"), ("single_atom_runs", "mean")])
def test_train_step_bounds_table_vs_restatement(case, agg, k0, gpu_device, monkeypatch):
    """Molecules without atoms (ids in between, molecules behind batch[-1]) and runs of lone atoms: the aggregate of every molecule
    from K0's bounds table — loss and every gradient against the float restatement, and the aggregate riding with the forward tile
    kernel (DMPNN_HEAD_AGG=tile) bit for bit equal to the head's own (=fused)."""
    from oracle import agg_torch, model_torch as om

    cfg = dict(mp=dict(d_h=D_H, activation="elu"), agg=agg, bn=True, ffn=dict(n_tasks=1, activation="elu"))
    g = _graph(STEP_CASES[case](), seed=15)
    n = g["n_mols"]
    y = torch.randn(n, 1, generator=torch.Generator().manual_seed(5))
    runs = {}
    for form in ("tile", "fused"):
        monkeypatch.setenv("DMPNN_HEAD_AGG", form)
        runs[form] = _step_run(cfg, g, gpu_device, y)
    state, loss, grads, model = runs["tile"]
    assert torch.equal(loss, runs["fused"][1]), (loss, runs["fused"][1])
    for i, (a, b) in enumerate(zip(grads, runs["fused"][2])):
        assert torch.equal(a, b), i
    # the restatement: agg_torch's scatter has batch.max() + 1 rows — the molecules behind it aggregate to zero rows (dmpnn.h, f1)
    scatter = agg_torch._scatter

    def padded(H, batch, reduce):
        out = scatter(H, batch, reduce)
        return torch.cat([out, out.new_zeros(n - out.shape[0], out.shape[1])]) if out.shape[0] < n else out

    monkeypatch.setattr(agg_torch, "_scatter", padded)
    ref = om.Model(state, cfg)
    ref_loss = ref.loss(_CPUBatch(g), y, torch.ones(n, 1), None, None)
    ref_loss.backward()
    assert abs(float(loss) - float(ref_loss)) <= 1e-5 * max(1.0, abs(float(ref_loss))), (float(loss), float(ref_loss))
    names = [k for k, p in model.named_parameters() if p.requires_grad]
    for i, k in enumerate(names):
        assert parity_err(grads[i].numpy(), ref.p[k].grad.numpy()) <= 2e-5, k


class _CPUBatch:
    def __init__(self, g):
        self.V, self.E, self.edge_index, self.rev_edge_index, self.batch = g["V"], g["E"], g["edge_index"], g["rev"], g["batch"]


def test_train_step_on_an_unsorted_batch_is_nan(k0, gpu_device):
    """The advisor's batch ([..., 5, 5, 1, 1]) through the one-call step on the tile plan: K0 flags it, the tile kernel and the
    aggregation poison it (dmpnn.h: "an invalid batch ... poisons the outputs with NaN") — a NaN loss and poisoned gradients,
    never a finite wrong step."""
    cfg = dict(mp=dict(d_h=D_H, activation="elu"), agg="mean", bn=True, ffn=dict(n_tasks=1, activation="elu"))
    g = _invalid("advisor", _graph(_qm9_sizes(100, 24), seed=16))
    g["n_mols"] = int(g["batch"].max()) + 1
    y = torch.randn(g["n_mols"], 1, generator=torch.Generator().manual_seed(6))
    _, loss, grads, _ = _step_run(cfg, g, gpu_device, y)
    assert torch.isnan(loss), loss
    for i, gr in enumerate(grads):
        assert not torch.isfinite(gr).all(), i
