"""Shared helpers of the boundary sweep of the LEAN per-step training route (``tests/test_lean_boundaries.py``): no fixtures, no
pytest settings — a plain module on top of ``rows_harness``.

The route: ``engine.forward(..., keep=True, route="fused16")`` -> ``fused16_lean`` (csrc/dmpnn_step16.hip; ``k_step16`` keeps split
message rows and one sign bit per element), ``engine.backward`` -> one ``k_bstep16<WN>`` launch per depth step
(csrc/dmpnn_bstep16.hip) and the split-row products ``k_wgrad16r`` (csrc/dmpnn_wgrad16.hip).

* ``Case`` / ``graph`` / ``inputs``: a case is a graph by name, the widths, depth, activation, bias, dropout and the form of the
  gradient input; its float32 CPU operands are drawn from a seed derived from its id.  (``TILE_PIECES``, ``name@mol`` and
  ``name@rows`` are the graphs of the tile kernels' sweep, ``tests/tile_harness.py``, which shares ``Case`` and the reference.)
* ``reference``: the block in ``dtype`` from the ops of ``oracle/dmpnn_torch.py`` (``initialize`` / ``message`` / ``update`` /
  ``segment_sum_dst`` / ``finalize``), the pre-activation of every site recorded; with ``masks`` every ReLU-class activation is
  replaced by the fixed 0 / 1 decisions handed in (a kinked activation makes a gradient only as reproducible as its decisions), with
  ``keeps`` the dropout masks are replayed.
* ``run_lean``: the route on the device, ``out`` and every gradient inside NaN-prefilled buffers with guard regions (``rows_harness.Mat``).
* ``sign_check`` / ``tile_table`` / ``wgrad16r_rows``: the rule for the kept bits, and the plan's tile rule and the products' row-split
  rule restated (labels and coverage checks only).
"""
import dataclasses
import functools
import math
import zlib

import torch

import rows_harness as rh
from oracle import dmpnn_torch as ot

MARGIN = rh.MARGIN
CAP = rh.CAP
LEAKY_SLOPE = 0.1            # (``oracle.dmpnn_torch.activation_fn("leakyrelu")``)
# ``dmpnn_forward`` refuses ``DMPNN_ACT_NONE`` on every route ("activation 0 is not built in"): the branch of the lean kernels without
# kept bits cannot be reached through the ABI.  The activation that needs no decisions is LeakyReLU with slope 1: the backward step
# kernels multiply by 1 on either side of the kink, so everything holds unconditionally.
ENGINE_ACT = dict(relu=("relu", 0.0), leakyrelu=("leakyrelu", LEAKY_SLOPE), identity=("leakyrelu", 1.0),
                  tanh=("tanh", 0.0), elu=("elu", 0.0))   # (the smooth ones: the tile kernels' sweep, tests/tile_harness.py — no decisions)
RELU_CLASS = ("relu", "leakyrelu")   # the activations whose gradient is as reproducible as their decisions
BAND = 64 * 2.0 ** -24       # a kept bit may differ from the float64 sign only where |z| < BAND max|z| of its tensor
MAX_FLIPS = 2                # ... and in at most that many entries of a case
DROP_SEED = 0x1234_5678_9ABC_DEF
GRADS = ("W_i", "b_i", "W_h", "b_h", "W_o", "b_o")
BM, MAX_DEG = 48, 24         # rows of a tile, the largest in-degree the tiling holds (csrc/dmpnn_common.hpp)


@dataclasses.dataclass(frozen=True)
class Case:
    id: str
    graph: str
    d_h: int
    depth: int = 2
    d_v: int = 6
    d_e: int = 4
    bias: bool = False
    act: str = "relu"        # "relu" | "leakyrelu" (slope 0.1) | "identity": LeakyReLU with slope 1 — tau(z) = z whatever the kept bit says
    p: float = 0.0
    gmode: str = "randn"     # "zero-tiles": G is zero on every atom of tiles 0, 3, 6, .., of magnitude 1e-6 elsewhere
    pad: int = 0             # padding columns of ``out`` and of the gradient input ``G`` (NaN in ``G``'s; ``out``'s must stay untouched)
    seed: int = 0            # (bumped when the float32 oracle itself flips a sign outside the band on the first draw)


# ---- graphs --------------------------------------------------------------------------------------------------------------------------
CHAIN3 = (3, [(0, 1), (1, 2)])
BOND = (2, [(0, 1)])
DEGREES = (0, 1, 2, 3, 4, 5, 12, 24)
SPLIT_CHAINS = 700           # chains of 6 atoms of the product-split graph: 7 000 rows (see ``wgrad16r_rows``)


@functools.lru_cache(maxsize=None)
def graph(name):
    if name == "degrees":
        return rh.degree_graph(DEGREES)
    if name == "degrees-in-order":
        return rh.degree_graph(DEGREES, shuffle=False)
    if name == "degree25":
        return rh.degree_graph((1, 25))
    if name == "single-bond":
        return rh.degree_graph((1,))
    if name == "bonds24":        # in-degree 1 everywhere: tile stride 48, ONE tile of exactly 48 rows
        return rh._graph([BOND] * 24, 1, True)
    if name == "bonds25":        # ... and 50 rows: 48 + 2 (a symmetric graph has an even number of rows: 49 does not exist)
        return rh._graph([BOND] * 25, 2, True)
    if name == "one-row-tile":   # largest in-degree 2: stride 47; 48 rows whose last atom starts at row 47: tiles of 47 rows and of ONE row
        return rh._graph([CHAIN3] + [BOND] * 22, 3, True)
    if name == "isolated300":    # 300 atoms without bonds between bonded ones: one tile of 306 atoms, two passes of the kAtomCache loop
        return rh._graph([CHAIN3] + [(1, [])] * 300 + [CHAIN3], 4, True)
    if name == "chains30x6":     # 300 rows, stride 47: 7 tiles
        return rh.chain_graph(30, 6)
    if name == "chains12x10":    # paths of 9 bonds: a gradient reaches every site of a depth-8 block (a star's H^(t) is constant from t = 1 on
        return rh.chain_graph(12, 10)   # and nothing flows further back than two steps: deep cases on stars cannot tell the sites apart)
    if name == "qm9x12":         # the connectivity of twelve QM9-shaped molecules (rings, in-degrees 1 .. 4)
        from chemprop_amd import synth

        return synth.random_batch(12, "qm9", seed=3)
    if name == "chains-split":
        return rh.chain_graph(SPLIT_CHAINS, 6)
    # ---- the tile kernels' sweep (tests/tile_harness.py): the batch vector makes the molecules, the edges of ONE molecule lie side by
    # side — shuffled among themselves — as a tile plan needs them (a tile's rows are a range of the caller's edges)
    if name.endswith("@mol"):
        return molecule_order(graph(name[:-4]))
    if name.endswith("@rows"):
        return row_order(graph(name[:-5]))
    if name in TILE_PIECES:
        return molecule_order(rh._graph(TILE_PIECES[name](), zlib.crc32(name.encode()) % 1000, True))
    raise KeyError(name)


def _chain(n):
    return (n, [(i, i + 1) for i in range(n - 1)])


def _ions(n):
    """ONE molecule: a chain of three atoms and ``n - 3`` atoms without a bond (counter-ions of a salt)."""
    return (n, [(0, 1), (1, 2)])


def pieces_of(bmg):
    """``[(n_atoms, [(u, v), ..])]`` per molecule of a batch (each bond once, molecule-local atom ids)."""
    src, dst = bmg.edge_index
    first = torch.cumsum(torch.bincount(bmg.batch, minlength=len(bmg)), 0) - torch.bincount(bmg.batch, minlength=len(bmg))
    out = [(int((bmg.batch == m).sum()), []) for m in range(len(bmg))]
    for u, v in zip(src.tolist(), dst.tolist()):
        if u < v:
            m = int(bmg.batch[u])
            out[m][1].append((u - int(first[m]), v - int(first[m])))
    return out


def _mixed_oversize():
    small = pieces_of(graph("qm9x12"))
    return small[:6] + [_chain(26)] + small[6:]


ATOM = (1, [])
TILE_PIECES = {
    "chain25": lambda: [_chain(25)],                                    # ONE tile of exactly 48 rows
    "chain26": lambda: [_chain(26)],                                    # 50 rows: beyond the tile by rows — the generic path
    "star24": lambda: [(25, [(0, i) for i in range(1, 25)])],            # 48 rows, in-degree 24
    "ions32": lambda: [_ions(32)],                                      # exactly 32 atoms (4 rows)
    "ions33": lambda: [_ions(33)],                                      # beyond the tile by ATOMS (a connected molecule hits the rows first)
    "atoms40": lambda: [ATOM] * 35 + [BOND] + [ATOM] * 5,               # tiles closed by the 32-atom limit: 32 atoms without a row | 10 atoms, 2 rows
    "pack-exact": lambda: [_chain(10), _chain(10), _chain(7), BOND],    # 18 + 18 + 12 = 48 rows, then a tile of two rows
    "mixed-oversize": _mixed_oversize,                                  # regular tiles on both sides of a molecule of 50 rows
    "bonds2600": lambda: [BOND] * 2600,                                 # 5 200 atoms and rows: a launch of 4-wave WN = 5 tiles (256 CUs) — every message zero
    "chains3x1700": lambda: [CHAIN3] * 1700,                            # ... and one whose messages are not: 5 100 atoms, 6 800 rows
}


def _reordered(bmg, p):
    """The same batch with its edges in another order: position ``k`` holds edge ``p[k]``."""
    from chemprop_amd.data import BatchMolGraph

    src, dst = bmg.edge_index
    inv = torch.empty_like(p)
    inv[p] = torch.arange(p.numel())
    return BatchMolGraph.from_tensors(bmg.V, bmg.E, torch.stack((src[p], dst[p])), inv[bmg.rev_edge_index[p]], bmg.batch, len(bmg))


def molecule_order(bmg):
    """The edges of one molecule side by side (a stable sort: the shuffled order inside a molecule stays)."""
    return _reordered(bmg, torch.sort(bmg.batch[bmg.edge_index[0]], stable=True).indices)


def row_order(bmg):
    """The edges by destination atom, stable: the caller's order IS the plan's CSR-row order (and a molecule's edges lie side by side)."""
    return _reordered(bmg, torch.sort(bmg.edge_index[1], stable=True).indices)


def tile_table(bmg):
    """The plan's row tiles restated (csrc/dmpnn_prepare.hip: ``tile_geom`` / ``tile_of``) -> (tile of every atom, rows per tile);
    ``(None, None)`` when an in-degree exceeds what the tiling holds."""
    deg = rh.in_degrees(bmg)
    nE = int(bmg.edge_index.shape[1])
    md = max(int(deg.max()) if deg.numel() else 0, 1)
    if md > MAX_DEG or nE == 0:
        return None, None
    b0 = BM - md + 1
    n_tiles = -(-nE // b0)
    row_ptr = torch.cumsum(deg, 0) - deg
    tile = torch.clamp(row_ptr // b0, max=n_tiles - 1)
    return tile, torch.zeros(n_tiles, dtype=torch.int64).index_add_(0, tile, deg)


# ---- the products' row splits (csrc/dmpnn_wgrad16.hip: wgrad16r_plan_launch / plan_wgrad16r, restated) ----------------------------------
def _even_kt(K):
    nkt, n_kg = (K + 15) // 16, (K + 127) // 128
    return n_kg >= 1 and all((((g + 1) * nkt // n_kg + 1) >> 1) - ((g * nkt // n_kg) >> 1) <= 4 for g in range(n_kg))


def _stage_cost(K):
    if K <= 1:
        return 3
    nkt, nca, n_kg = (K + 15) // 16, (K + 31) // 32, (K + 127) // 128
    kt = -(-nkt // n_kg) if _even_kt(K) else 2 * -(-nca // n_kg)
    return min(max(kt, 3), 8)


def wgrad16r_rows(n_edges, d_h, d_x, depth, cus=256):
    """(rows per workgroup, row splits) of the W_h jobs and of the W_i jobs of the lean backward's ONE product launch — depth - 1 jobs
    of ``K = d_h`` and depth jobs of ``K = d_x = d_v + d_e``, ``n_edges`` rows each — and the launch's base row count ``R0`` (32: one
    stage; more: the launch grew it to stay within its workgroup budget); ``cus``: the device's compute units."""
    Ks = [d_h] * (depth - 1) + [d_x] * depth
    n_kg = lambda K: max((K + 127) // 128, 1)
    units = sum(n_edges * n_kg(K) * _stage_cost(K) / 8.0 for K in Ks)
    rounds = max(int(units / (512.0 * cus)), 1)
    budget = max(rounds * cus, 8)
    R0 = max((int(units / budget) + 31) // 32 * 32, 32)
    R_max = (n_edges + 31) // 32 * 32 * 8
    while True:
        rows = [min((R0 * 8 // _stage_cost(K) + 31) // 32 * 32, 1 << 20) for K in Ks]
        wg = sum((n_kg(K) * -(-n_edges // R) + 7) // 8 * 8 for K, R in zip(Ks, rows))
        if wg <= budget or R0 >= R_max:
            break
        R0 += 32
    rh_, ri_ = rows[0], rows[-1]
    return (rh_, -(-n_edges // rh_)), (ri_, -(-n_edges // ri_)), R0


# ---- operands ------------------------------------------------------------------------------------------------------------------------
def _lin(gen, n_out, n_in):
    """``nn.Linear``'s range with row ``n`` scaled by ``1 + n / n_out`` (a transposed or shifted tile cannot pass)."""
    k = 1.0 / math.sqrt(max(n_in, 1))
    return (2 * torch.rand(n_out, n_in, generator=gen) - 1) * k * (1 + torch.arange(n_out).float() / n_out).view(-1, 1)


@functools.lru_cache(maxsize=None)
def inputs(case: Case):
    """float32 CPU operands of a case: ``V``, ``E``, the six parameters (``b_i`` / ``b_h``: ``None`` without ``bias``), ``G``."""
    bmg = graph(case.graph)
    nV, nE = int(bmg.V.shape[0]), int(bmg.edge_index.shape[1])
    gen = torch.Generator().manual_seed(zlib.crc32(case.id.encode()) + 7919 * case.seed)
    h, dx = case.d_h, case.d_v + case.d_e
    vec = lambda n, n_in: (2 * torch.rand(n, generator=gen) - 1) / math.sqrt(max(n_in, 1))
    inp = dict(V=torch.randn(nV, case.d_v, generator=gen), E=torch.randn(nE, case.d_e, generator=gen),
               W_i=_lin(gen, h, dx), W_h=_lin(gen, h, h), W_o=_lin(gen, h, case.d_v + h), b_o=vec(h, case.d_v + h),
               b_i=vec(h, dx) if case.bias else None, b_h=vec(h, h) if case.bias else None)
    G = torch.randn(nV, h, generator=gen) * (1 + torch.arange(h).float() / h)
    if case.gmode == "zero-tiles":
        tile, _ = tile_table(bmg)
        G = G * 1e-6
        G[tile % 3 == 0] = 0.0
    else:
        assert case.gmode == "randn", case.gmode
    inp["G"] = G
    return inp


def keep_masks(case: Case, n_edges, n_atoms):
    """The dropout masks (bool: kept) from the library's host function ``dmpnn_dropout_keep``: update site ``t`` is hash site
    ``t - 1`` with the caller's edge id as the row; the finalize is hash site ``depth - 1`` with the atom id."""
    import ctypes as C

    from chemprop_amd import _lib

    lib = _lib.load()
    seed, p = C.c_uint64(DROP_SEED), C.c_float(case.p)
    one = lambda site, rows: torch.tensor([[lib.dmpnn_dropout_keep(seed, site, r, c, p) for c in range(case.d_h)] for r in range(rows)],
                                          dtype=torch.bool).view(rows, case.d_h)
    return [one(t, n_edges) for t in range(case.depth - 1)] + [one(case.depth - 1, n_atoms)]


# ---- the reference -------------------------------------------------------------------------------------------------------------------
def reference(case: Case, dtype=torch.float64, masks=None, keeps=None, grads=True):
    """-> ``(out, pre, grads)``: the output, the pre-activation of every site (H0, the updates, the finalize: ``depth + 1`` tensors,
    edge sites in the caller's edge order) and, with ``grads``, ``d sum(out * G) / d`` every parameter.  ``masks``: per site the 0 / 1
    decisions that replace a ReLU-class activation (``None``: the activation itself); ``keeps``: the dropout masks (bool) of the
    update sites and of the finalize, applied with the exact ``1 / (1 - p)``."""
    bmg, inp = graph(case.graph), inputs(case)
    nV = int(bmg.V.shape[0])
    src, dst = bmg.edge_index
    rev = bmg.rev_edge_index
    leaf = lambda t: None if t is None else t.to(dtype).clone().requires_grad_(grads)
    prm = {k: leaf(inp[k]) for k in GRADS}
    w = ot.MPWeights(prm["W_i"], prm["W_h"], prm["W_o"], prm["b_o"], prm["b_i"], prm["b_h"])
    V, E = inp["V"].to(dtype), inp["E"].to(dtype)
    slope = ENGINE_ACT[case.act][1]
    act = ot.activation_fn("none" if case.act == "identity" else case.act)
    pre = []

    def tau(z):
        i = len(pre)
        pre.append(z.detach())
        if masks is None or case.act not in RELU_CLASS:
            return act(z)
        m = masks[i].to(dtype)
        return z * (m + (1 - m) * slope)

    scale = 1.0 / (1.0 - case.p) if keeps is not None else 1.0
    H0 = ot.initialize(V, E, src, w)
    H = tau(H0)
    for t in range(1, case.depth):
        H = ot.update(ot.message(H, src, dst, rev, nV), H0, w, tau)
        if keeps is not None:
            H = H * (keeps[t - 1].to(dtype) * scale)
    out = ot.finalize(ot.segment_sum_dst(H, dst, nV), V, None, w, tau)
    if keeps is not None:
        out = out * (keeps[-1].to(dtype) * scale)
    g = None
    if grads:
        (out * inp["G"].to(dtype)).sum().backward()
        g = {k: p.grad for k, p in prm.items() if p is not None and p.grad is not None}   # (depth 1: W_h takes no part)
    return out.detach(), pre, g


def true_masks(pre):
    return [z > 0 for z in pre]


def sign_check(case_id, got, pre64, where=None):
    """``got``: per site the decisions a run took (bool), ``pre64``: the float64 pre-activations of the same sites; ``where``: per site
    ``None`` or the entries that count (bool).  A decision may differ from the float64 sign only where ``|z| < BAND max|z|`` of its
    tensor, and in at most ``MAX_FLIPS`` entries of the case -> (failures, flips)."""
    fails, flips = [], 0
    for t, (b, z) in enumerate(zip(got, pre64)):
        diff = b != (z > 0)
        if where is not None and where[t] is not None:
            diff &= where[t]
        n = int(diff.sum())
        flips += n
        if n:
            worst, band = float(z[diff].abs().max()), BAND * float(z.abs().max())
            if not worst < band:
                fails.append(f"site {t}: {n} decisions differ from the float64 sign, one at |z| = {worst:.3e} (band {band:.3e})")
    if flips > MAX_FLIPS:
        fails.append(f"{flips} decisions differ from the float64 signs (at most {MAX_FLIPS})")
    return fails, flips


@functools.lru_cache(maxsize=None)
def yardsticks(case: Case):
    """-> ``(out64, pre64, grads64, e32, fails32)``: the float64 reference with its own decisions, the float32 oracle's error against
    it per tensor (its gradients GIVEN the float64 decisions: linear algebra, no kink) and what ``sign_check`` says about the
    float32 oracle's own decisions.  No dropout (the dropout case replays its masks in the test)."""
    out64, pre64, g64 = reference(case)
    out32, pre32, _ = reference(case, torch.float32, grads=False)
    relu_class = case.act in RELU_CLASS
    _, _, g32 = reference(case, torch.float32, masks=true_masks(pre64) if relu_class else None)
    e32 = rh.yardstick(dict(out=out64, **g64), dict(out=out32, **g32))
    fails32 = sign_check(case.id, true_masks(pre32), pre64)[0] if relu_class else []
    return out64, pre64, g64, e32, fails32


# ---- the route on the device -----------------------------------------------------------------------------------------------------------
_PLANS = {}


def plan_of(name, dev):
    if name not in _PLANS:
        _PLANS[name] = rh.make_plan(graph(name), dev)
    return _PLANS[name]


def _grad_mats(dev, case: Case):
    h, dx = case.d_h, case.d_v + case.d_e
    shapes = dict(W_i=(h, dx), b_i=(1, h), W_h=(h, h), b_h=(1, h), W_o=(h, case.d_v + h), b_o=(1, h))
    if not case.bias:
        del shapes["b_i"], shapes["b_h"]
    return {k: rh.Mat(dev, *s, off=4) for k, s in shapes.items()}


def run_lean(dev, case: Case, route="fused16", backward=2):
    """The forward with ``keep`` on ``route`` and ``backward`` backward passes with every gradient requested -> a dict: ``st``, ``out``
    (read back: the guard regions of its buffer checked), ``bits`` (``[depth, n_edges, d_h]`` bool in the CALLER's edge order, or
    ``None`` off the lean route) and ``grads``: one ``{name: tensor}`` per pass."""
    from chemprop_amd import engine

    bmg, inp = graph(case.graph), inputs(case)
    plan, _ = plan_of(case.graph, dev)
    nV, nE = int(bmg.V.shape[0]), int(bmg.edge_index.shape[1])
    mv = lambda k: None if inp[k] is None else inp[k].to(dev)
    out_m = rh.Mat(dev, nV, case.d_h, case.d_h + case.pad, off=4)
    act, slope = ENGINE_ACT[case.act]
    kw = dict(depth=case.depth, act=act, slope=slope, keep=True, route=route, out=out_m.view())
    if case.p:
        kw["dropout"] = (case.p, DROP_SEED)
    _, st = engine.forward(plan, mv("V"), mv("E"), mv("W_i"), mv("W_h"), mv("W_o"), mv("b_o"), mv("b_i"), mv("b_h"), **kw)
    G_m = rh.Mat(dev, nV, case.d_h, case.d_h + case.pad, off=4, data=inp["G"])
    G = G_m.view()
    passes = []
    for _ in range(backward):
        mats = _grad_mats(dev, case)
        bufs = {k: (m.view()[0] if k.startswith("b_") else m.view()) for k, m in mats.items()}
        got = engine.backward(st, G, {k: True for k in GRADS}, out=bufs)
        torch.cuda.synchronize()
        for k in GRADS:
            assert (got[k] is None) == (k not in mats), k
            assert got[k] is None or got[k].data_ptr() == bufs[k].data_ptr(), f"{k}: the gradient did not go to the buffer handed in"
        passes.append({k: (m.read("g" + k)[0] if k.startswith("b_") else m.read("g" + k)) for k, m in mats.items()})
    torch.cuda.synchronize()
    bits = None
    if st.route == "fused16/lean":
        bits = engine.lean_sign_bits(st)[:, plan.inv32.long()].cpu()
    return dict(st=st, out=out_m.read("out"), bits=bits, grads=passes)
