"""Shared helpers of the boundary sweep of the TILE kernels (``tests/test_tile_boundaries.py``): no fixtures, no pytest settings — a
plain module on top of ``lean_harness`` and ``rows_harness``.

The route: ``engine.forward(plan, ..., keep=..., route="mega", out=Mat.view())`` -> ``launch_mega16_forward`` -> ``k_mpnn_tile16<WN, SA,
KEEP, NW>`` (csrc/dmpnn_mega16_impl.hpp; a molecule beyond the tile: csrc/dmpnn_spill_impl.hpp), ``engine.backward`` ->
``k_mpnn_tile16_bwd<WN, SA, NW>`` (csrc/dmpnn_mega16_bwd_impl.hpp) and the weight-gradient products, on the two plans that reach them:

* ``"full"``: ``GraphPlan.from_bmg(b)`` — the tiles are CONNECTED PIECES (the single-workgroup plan knows no molecules), the kept
  tensors are in CSR-row order;
* ``"tiles"``: ``GraphPlan.from_bmg(b, light="tiles")`` — the tiles are whole MOLECULES of the batch vector, a tile's rows are a range
  of the caller's edges (``DMPNN_F_TILE_PLAN``), the kept tensors are in the caller's edge order.

* ``tile_rule``: the packing rule restated with ``oracle.collate_numpy.blocked_molecule_tiles`` for either plan.
* ``run_tile``: one forward (+ backward passes) with ``out`` and every gradient inside NaN-prefilled ``rows_harness.Mat`` buffers, and
  the DECISIONS the run took at every ReLU-class site, read from the kept fp32 tensors (``H0`` holds the pre-activation, ``H^(t)`` the
  activation's output — after dropout — and the finalize's decision is the sign of ``out``), in the caller's edge order.
"""
import numpy as np
import torch

import lean_harness as lh
import rows_harness as rh
from oracle import collate_numpy as cn

BM, BA = 48, 32              # rows and atoms of a tile (csrc/dmpnn_common.hpp: kMegaBM, kMegaBA)
PLANS = ("full", "tiles")
HDR_NMTILES, HDR_NSPILL = 6, 8


# ---- the packing rule ------------------------------------------------------------------------------------------------------------------
def pieces(bmg, kind):
    """(atoms, rows) per packing unit: the molecules of the batch vector (``"tiles"``) or the connected runs of atoms — an atom
    boundary no bond spans starts a new one (``"full"``: csrc/dmpnn_prepare.hip, build_piece_tiles)."""
    nV = int(bmg.V.shape[0])
    src, dst = bmg.edge_index
    deg = torch.bincount(dst, minlength=nV)
    if kind == "tiles":
        unit = bmg.batch
    else:
        covered = torch.zeros(nV + 1, dtype=torch.bool)
        for u, v in zip(src.tolist(), dst.tolist()):
            covered[min(u, v) + 1:max(u, v) + 1] = True
        unit = torch.cumsum((~covered[:nV]).long(), 0) - 1
    n = int(unit.max()) + 1
    return torch.bincount(unit, minlength=n).tolist(), torch.zeros(n, dtype=torch.int64).index_add_(0, unit, deg).tolist()


def tile_rule(name, kind):
    """-> (tile_row, tile_atom, oversize tiles) of graph ``name`` on plan ``kind``: what the device's planner has to build."""
    atoms, rows = pieces(lh.graph(name), kind)
    tr, ta = cn.blocked_molecule_tiles(atoms, rows)
    over = int(((np.diff(tr) > BM) | (np.diff(ta) > BA)).sum())
    return tr, ta, over


def tile_waves_rule(n_atoms, n_edges, d_h, cus):
    """``tile_waves`` (csrc/dmpnn_mega16.hip) for a launch bounded by the plan's layout (more slots than compute units)."""
    if d_h <= 128 or d_h > 320:
        return 4
    est = max((n_edges + 39) // 40, (n_atoms + 19) // 20)
    return 8 if est + est // 16 <= cus else 4


def keeps_rows(d_h):
    """Where the tile kernel's LDS tile row (64 WN columns) IS the kept split row (64-column blocks): ``mega16_rows_width_ok``."""
    bn = 64 if d_h <= 64 else 128 if d_h <= 128 else 320
    return (d_h + 63) // 64 * 64 == bn


# ---- the route on the device -----------------------------------------------------------------------------------------------------------
_PLANS = {}


def plan_of(name, kind, dev):
    """-> (plan, the batch on the device): one plan per graph and kind."""
    from chemprop_amd import engine

    if (name, kind) not in _PLANS:
        b = lh.graph(name).__copy__()
        b.to(dev)
        plan = engine.GraphPlan.from_bmg(b, light="tiles" if kind == "tiles" else False)
        assert bool(plan.tiles_only) == (kind == "tiles"), (name, kind)
        _PLANS[(name, kind)] = (plan, b)
    return _PLANS[(name, kind)]


def grad_mats(dev, case, atom=False):
    """One NaN-prefilled buffer per gradient of the case; ``atom``: ``W_i [d_h, d_v]``, ``W_h [d_h, d_h + d_e]`` (base.py:278-289)."""
    if not atom:
        return lh._grad_mats(dev, case)
    h = case.d_h
    shapes = dict(W_i=(h, case.d_v), b_i=(1, h), W_h=(h, h + case.d_e), b_h=(1, h), W_o=(h, case.d_v + h), b_o=(1, h))
    if not case.bias:
        del shapes["b_i"], shapes["b_h"]
    return {k: rh.Mat(dev, *s, off=4) for k, s in shapes.items()}


def run_tile(dev, case, kind, keep=True, bits=True, backward=2, atom=False, inputs=None):
    """One forward on ``route="mega"`` (``keep``: a training forward, ``bits``: ``keep_bits``) and ``backward`` backward passes with every
    gradient requested -> a dict: ``st``, ``out`` (read back: the guard regions checked), ``sites`` (``depth + 1`` bool tensors — the
    decisions at H0, every H^(t) and the finalize, edge sites in the CALLER's edge order; ``None`` where the run kept sign bits or
    nothing) and ``grads``: one ``{name: tensor}`` per pass.  ``case.pad``: padding columns of ``out`` and ``G`` and of ``V`` and ``E``.
    ``atom``: atom messages (``DMPNN_F_ATOM``); ``inputs``: the operands instead of ``lean_harness.inputs(case)`` — the same keys, the
    weights in the block's own shapes."""
    from chemprop_amd import _lib, engine

    bmg, inp = lh.graph(case.graph), (lh.inputs(case) if inputs is None else inputs)
    plan, _ = plan_of(case.graph, kind, dev)
    nV, nE = int(bmg.V.shape[0]), int(bmg.edge_index.shape[1])
    mv = lambda k: None if inp[k] is None else inp[k].to(dev)
    V_m = rh.Mat(dev, nV, case.d_v, case.d_v + case.pad, data=inp["V"])
    E_m = rh.Mat(dev, nE, case.d_e, case.d_e + case.pad, data=inp["E"])
    out_m = rh.Mat(dev, nV, case.d_h, case.d_h + case.pad, off=4)
    act, slope = lh.ENGINE_ACT[case.act]
    kw = dict(depth=case.depth, act=act, slope=slope, keep=keep, keep_bits=bits, route="mega", out=out_m.view())
    if case.p:
        kw["dropout"] = (case.p, lh.DROP_SEED)
    if atom:
        kw["atom"] = True
    _, st = engine.forward(plan, V_m.view(), E_m.view(), mv("W_i"), mv("W_h"), mv("W_o"), mv("b_o"), mv("b_i"), mv("b_h"), **kw)
    assert st.route == "mega16", st.route
    assert bool(st.args.flags & _lib.F_TILE_PLAN) == (kind == "tiles" and keep), (kind, keep, hex(st.args.flags))
    assert bool(st.args.flags & _lib.F_ATOM) == bool(atom) and bool(st.plan.tiles_only) == (kind == "tiles"), (kind, hex(st.args.flags))
    torch.cuda.synchronize()
    res = dict(st=st, out=out_m.read("out"), sites=None, grads=[])
    if not keep:
        return res
    if not st.args.keep_bits:
        order = slice(None) if kind == "tiles" else plan.inv32.long()
        H0, Hs = st.H0[order, :case.d_h].cpu(), st.Hs[:, order, :case.d_h].cpu()
        res["sites"] = [H0 > 0] + [Hs[t] > 0 for t in range(case.depth - 1)] + [res["out"] > 0]
    G_m = rh.Mat(dev, nV, case.d_h, case.d_h + case.pad, off=4, data=inp["G"])
    for _ in range(backward):
        mats = grad_mats(dev, case, atom)
        bufs = {k: (m.view()[0] if k.startswith("b_") else m.view()) for k, m in mats.items()}
        got = engine.backward(st, G_m.view(), {k: True for k in lh.GRADS}, out=bufs)
        torch.cuda.synchronize()
        for k in lh.GRADS:
            assert (got[k] is None) == (k not in mats), k
            assert got[k] is None or got[k].data_ptr() == bufs[k].data_ptr(), f"{k}: the gradient did not go to the buffer handed in"
        res["grads"].append({k: (m.read("g" + k)[0] if k.startswith("b_") else m.read("g" + k)) for k, m in mats.items()})
    return res
