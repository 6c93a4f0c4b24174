"""The TILE kernels — the whole-forward tile kernel ``k_mpnn_tile16`` (csrc/dmpnn_mega16_impl.hpp), its backward twin
``k_mpnn_tile16_bwd`` (csrc/dmpnn_mega16_bwd_impl.hpp) and the generic path of a molecule beyond the tile (csrc/dmpnn_spill_impl.hpp) —
through ``engine.forward(plan, ..., keep=..., route="mega", out=...)`` / ``engine.backward`` at the seams of their dispatch, against
float64 on the CPU (``tests/tile_harness.py``), on the FULL plan (kept tensors in CSR-row order) and on the TILE plan
(``light="tiles"``, ``DMPNN_F_TILE_PLAN``: kept tensors in the caller's edge order).  ``st.route == "mega16"`` and the plan's kind are
asserted for every run.

The contract of one case is ``_hold`` of ``tests/test_lean_boundaries.py``: the output and every gradient in the metric WITHOUT a
floor, ``err = max|got - ref| / max|ref|``, within ``min(MARGIN max(e32, 2**-23), cap)`` (``e32``: the float32 oracle on the same inputs
against float64; ``cap``: ``rows_harness.CAP``), NaN-prefilled buffers whose guard regions must come back untouched, two backward
passes bit for bit.  ReLU-class gradients are held to the float64 backward GIVEN the kernel's own decisions: these are read from the
kept fp32 ``H0`` / ``H^(t)`` (their sign) of the run WITHOUT sign bits and from the sign of ``out``, and held by ``sign_check`` (band
``64 * 2**-24 * max|z|``, at most two flips per case: a condition).  The run WITH sign bits (tile plan) must give a bit-identical
``out`` and its gradients are held to the reference given the SAME decisions: a wrong bit is a wrong gradient.  Every case also runs
the inference forward (``keep=False``: the ``KEEP = false`` builds and, beyond the tile, the spill scratch).

Dropout: the hash of an edge site takes the CALLER's edge id on either plan (``dropout_frags``: under a CSR plan row ``r`` of a tile
is edge ``perm[rs + r]``, under a tile plan edge ``rs + r``), the finalize the atom id: ``lean_harness.keep_masks`` as it stands.

Left out: atom messages (their own sweep: ``tests/test_atom_tile_boundaries.py``); the f16-operand inference form (not fp32-class); corrupted plans and batches
(``tests/test_host_plan_gpu.py``); in-degree 25; the aggregate ride of ``dmpnn_train_step``; no case poisons or faults a launch.

Instantiation -> case (forward ``launch_mega16<WN, SA, KEEP[, 8]>``; every case runs KEEP = true and KEEP = false):
``<1, true, *>`` ``h4/8/36/60/64-relu-*``; ``<1, false, *>`` ``h4..64-tanh-*``; ``<2, true, *>`` ``h68/128-relu-*``; ``<2, false, *>``
``h68/128-tanh-*``; ``<5, true, *, 8>`` ``h132..320-relu-*`` (qm9x12: 5 tiles); ``<5, false, *, 8>`` ``h132..320-tanh-*``;
``<5, true, *>`` (4 waves) ``h132/h300-waves4-relu`` (bonds2600), ``h132/h300-waves4-chains-relu``; ``<5, false, *>``
``h132/h300-waves4-tanh``, ``h300-waves4-chains-tanh``.
Backward ``launch_mega16_bwd<WN, SA[, 8]>``: the same ids.  Kept forms: fp32 rows on the full plan (every ``@full`` run) and on the
tile plan (the first run of every ``@tiles`` case), sign bits (the second run of every ReLU-class ``@tiles`` case), split message
rows on both (``test_tile_kept_forms``, and by size ``*-waves4-*``: 5 200 / 6 800 rows).  The spill path: ``*-chain26-*``,
``*-mixed-oversize-*`` on both plans, ``*-ions33@tiles``, forward, inference and backward.

What the sweep found — by READING the dispatch before the first run, not run on the GPU before the fix: the training forward copies the
kept split message rows out of its LDS tile as whole rows of the BUILD's width (``flush_rows``: ``TS = 256 WN + 16`` bytes, 1 296 for
``WN = 5``), while the buffer, the backward tile kernel and the products count rows of ``split_row_floats(d_h)`` floats (64-column
blocks: 784 bytes at ``d_h`` 132 .. 192, 1 040 at 196 .. 256).  For ``128 < d_h <= 256`` with split rows (``DMPNN_KEEP_ROWS=1``, or by
size from 4 096 message rows on) the forward wrote up to 65 % past the end of ``msplit`` and the products read rows nobody wrote.
``mega16_keeps_rows`` / ``dmpnn_train_route`` now keep split rows only where the two widths agree (``d_h <= 128``, ``256 < d_h <= 320``):
``test_tile_kept_forms[h132]`` / ``[h256]`` and ``h132-waves4-*`` (split rows by size) pin it, the refusal table states it.

MARGIN (``rows_harness.MARGIN`` = 16, unchanged).  Measured on the MI355X with the report lines of every run (125 GPU tests, 1 428
tensor comparisons): the worst ``err / max(e32, 2**-23)`` is 3.04 — ``gW_o`` of ``h4-ions33`` (err 3.6e-7 against a float32 draw of
1.0e-7) — then 2.48 (``gW_h``, ``h4-ions33``), 2.45 (``gb_h``, ``h300-waves4-relu``), 2.34 (``out``, ``h68-atoms40``), 2.30 (``gb_o``,
``h4-bonds2600``), 2.21 (``gb_i``, ``h8-relu-bias``), 1.99 (``gW_i``, ``h4-pack-exact``).  2 x 3.04 = 6.1 <= 16: MARGIN stays.  The bars
are 1.9e-6 .. 2e-5; some forty tensors sit at their cap (``out`` of the tanh cases from ``d_h`` 128 on, float32 at 0.7e-6 .. 1.6e-6, the
kernels at 0.5e-6 .. 1.0e-6; ``gW_i`` of the 5 000-row graphs, float32 at 1.3e-6 .. 3.0e-6, the kernels at 1.6e-7 .. 4.2e-7).  No run flipped
a decision (0 of at most 2 everywhere); the sign-bit run's output equalled the fp32-row run's bit for bit everywhere, the six kept
forms of a shape likewise.  ``gW_h`` of the bond-only graphs and of depth 1 is exactly zero from the kernels.  Wall time of the
module's GPU tests on the MI355X: 5.2 s (the lean module: 3.2 s).

Tried against deliberately wrong builds (scratch copies, never committed), the module run once on each.  (1) A tile of exactly 48
rows loses its last row in the forward: fails all 92 runs on graphs with a 48-row tile (``qm9x12``, ``chain25``, ``star24``,
``pack-exact``, ``mixed-oversize``, ``degrees@mol``) and none of the 33 others (36-row chains, the spilled ``chain26``, ``ions32/33``,
``atoms40``, the 32- and 40-row tiles of ``bonds2600`` / ``chains3x1700``).  (2) The chunk count of ``W_o[:, :d_v]`` floored beyond one
chunk: fails exactly ``h36-x66-v34`` on both plans (``d_v = 34``).  (3) The backward's sign bit taken from site ``t - 1``: fails the 50
runs that keep sign bits for a regular tile — every ReLU / LeakyReLU ``@tiles`` case and the five ``kept-forms`` — and nothing else
(full plan, smooth, identity, depth 1, dropout, the spilled ``chain26`` / ``ions33``: no bits).  (4) The transposed ``W_h`` of the
backward read untransposed: fails 102 — all but depth 1, ``chain26`` and ``ions33@tiles`` (the generic path reads ``W_h`` itself), and
the bond-only graphs, where no gradient passes ``W_h``.  That last line was a hole: ``bonds2600`` was the only graph on the 4-wave
``WN = 5`` builds, which therefore ran their update contraction on zero messages only; ``chains3x1700`` (in-degree 2, 6 800 rows)
closes it — build (4) fails its three cases, and build (3), run again, 51.  (5) The 4-wave ``WN = 5`` forward given another column
split (wave ``w`` starts at column tile ``3 w``, as the first four waves of the 8-wave form do): fails 7 of the 8 ``waves4`` runs and
nothing else — at ``d_h`` 300 column tiles 14 .. 18 are nobody's; at 132 the nine tiles are still covered (twice) and only the
sign-bit run fails, its words being filed by wave: ``h132-waves4-tanh`` passes, as the arithmetic says.  (Build (2) ran before the
chains were added: 122 GPU tests then.)
"""
import ctypes as C

import numpy as np
import pytest
import torch

import lean_harness as lh
import rows_harness as rh
import tile_harness as th
from lean_harness import Case

MARGIN = rh.MARGIN
gpu = pytest.mark.gpu
# d_h at the seams of the builds: WN = 1 | 2 | 5 (64 | 128 | 320), partial 32-column chunks and 16-column tiles, qn == 1 (d_h = 4)
WIDTHS = (4, 8, 36, 60, 64, 68, 128, 132, 192, 196, 256, 260, 300, 320)
EDGE_GRAPHS = tuple(n for n in lh.TILE_PIECES if n != "chains3x1700")
ACTS = ("relu", "leakyrelu", "identity", "tanh", "elu")
KEPT_WIDTHS = (36, 128, 300, 132, 256)   # one per WN — and the two widths at which split rows are NOT kept (see the docstring)
BOND_ONLY = ("bonds2600", "atoms40")     # in-degree 1 everywhere: every message, hence W_h's gradient, is exactly zero


def _runs():
    """-> [(case, plan kind)]"""
    rs = []
    bias = lambda i: dict(bias=bool(i % 2))
    nm = lambda b: "bias" if b else "nobias"
    # widths: ReLU on the tile plan (fp32 rows, then sign bits), tanh (the SA = false builds) on the full plan
    rs += [(Case(f"h{h}-relu-{nm(i % 2)}", "qm9x12", h, depth=3, **bias(i)), "tiles") for i, h in enumerate(WIDTHS)]
    rs += [(Case(f"h{h}-tanh-{nm(1 - i % 2)}", "qm9x12", h, depth=3, act="tanh", **bias(i + 1)), "full") for i, h in enumerate(WIDTHS)]
    # operand widths: d_v + d_e = 4, 34 (a partial chunk), 64, 66; nc_v, the chunk seam of W_o[:, :d_v], at d_v = 30 | 32 | 34;
    # d_v + d_h = 448, the largest shape mega_shapes_ok takes
    for i, (tag, dv, de, h) in enumerate((("x4", 2, 2, 36), ("x34-v30", 30, 4, 36), ("x64-v32", 32, 32, 36), ("x66-v34", 34, 32, 36),
                                          ("v128-h320", 128, 4, 320))):
        rs += [(Case(f"h{h}-{tag}", "qm9x12", h, d_v=dv, d_e=de, bias=bool(i % 2)), k) for k in th.PLANS]
    # activations
    for h in (36, 132):
        for act in ACTS:
            rs += [(Case(f"h{h}-act-{act}-{nm(b)}", "qm9x12", h, act=act, bias=b), "tiles" if b else "full") for b in (True, False)]
    # depth (deep cases on graphs with long paths: on a star no gradient reaches a site more than two steps back)
    rs += [(Case("h36-depth1", "qm9x12", 36, depth=1, bias=True), k) for k in th.PLANS]
    rs += [(Case("h36-depth2-chains", "chains12x10@mol", 36, depth=2), "tiles"), (Case("h36-depth8-chains", "chains12x10@mol", 36, depth=8, bias=True), "full"),
           (Case("h4-depth8-chains", "chains12x10@mol", 4, depth=8), "tiles"), (Case("h132-depth2", "qm9x12", 132, depth=2, bias=True), "full"),
           (Case("h132-depth8", "qm9x12", 132, depth=8), "tiles"), (Case("h36-depth8-leakyrelu", "qm9x12", 36, depth=8, act="leakyrelu", bias=True), "tiles")]
    rs += [(Case("h36-degrees", "degrees@mol", 36, bias=True), k) for k in th.PLANS]
    # tile edges
    rs += [(Case(f"h{h}-{g}", g, h, bias=True), k) for g in EDGE_GRAPHS for h in (4, 68) for k in th.PLANS]
    # waves: 4-wave WN = 5 tiles by shape (bonds2600); the 8-wave form is every qm9x12 case of d_h > 128 above
    rs += [(Case(f"h{h}-waves4-{act}", "bonds2600", h, act=act, bias=act == "relu"), "tiles") for h in (132, 300) for act in ("relu", "tanh")]
    rs += [(Case("h300-waves4-full", "bonds2600", 300), "full")]
    # (on bonds2600 every message is zero and W_h takes no part: the same builds on chains of three atoms)
    rs += [(Case("h132-waves4-chains-relu", "chains3x1700", 132, bias=True), "tiles"), (Case("h300-waves4-chains-tanh", "chains3x1700", 300, act="tanh"), "tiles"),
           (Case("h300-waves4-chains-relu", "chains3x1700", 300, depth=3), "full")]
    # layout
    rs += [(Case("h36-padded", "qm9x12", 36, pad=4, bias=True), "tiles"), (Case("h300-padded", "qm9x12", 300, depth=3, pad=12), "full"),
           (Case("h68-padded-chain26", "chain26", 68, pad=4, bias=True), "tiles")]
    assert len({(c.id, k) for c, k in rs}) == len(rs)
    by_id = {}
    for c, _ in rs:
        assert by_id.setdefault(c.id, c) == c, c.id
    return rs


RUNS = _runs()
CASES = list({c.id: c for c, _ in RUNS}.values())
KEPT = [Case(f"h{h}-kept-forms", "qm9x12@rows", h, depth=3, bias=True) for h in KEPT_WIDTHS]
DROPOUT = [Case(f"h{h}-dropout", "qm9x12", h, depth=3, p=0.25, bias=h == 36) for h in (36, 132)]
_ids = lambda r: f"{r[0].id}@{r[1]}" if isinstance(r, tuple) else None


def _report(s):
    print(s.replace("ROWSBAR", "TILEBAR"))


def _unused(case, g64, e32):
    """Depth 1: ``W_h`` / ``b_h`` take no part — their gradients are exactly zero."""
    g64, e32 = dict(g64), dict(e32)
    if case.depth == 1:
        g64["W_h"] = torch.zeros(case.d_h, case.d_h, dtype=torch.float64)
        if case.bias:
            g64["b_h"] = torch.zeros(case.d_h, dtype=torch.float64)
        e32.update(W_h=0.0, b_h=0.0)
    return g64, e32


def _grads(tag, case, res, ref, e32, fails):
    fails += [f"{tag}: {f}" for f in rh.compare(f"{case.id}/{tag}", dict(out=res["out"], **res["grads"][0]), ref, e32, dict(out="fwd", **{k: "grad" for k in lh.GRADS}), margin=MARGIN, report=_report)]
    a, b = res["grads"]
    for k in a:
        if not torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)):
            fails.append(f"{tag}: g{k}: two backward passes differ")


def _hold(dev, case, kind, out64, pre64, g64, e32, keeps=None):
    """The whole contract of one case on one plan."""
    relu_class = case.act in lh.RELU_CLASS
    fails = []
    a = th.run_tile(dev, case, kind, bits=False)
    assert not a["st"].args.keep_bits and a["sites"] is not None
    if relu_class:
        # the decisions the kernels took; where dropout zeroed an entry the kept tensor says nothing: the float64 decision stands in, times zero
        where = [None] * (case.depth + 1) if keeps is None else [None] + list(keeps)
        sites = [s if w is None else torch.where(w, s, z > 0) for s, w, z in zip(a["sites"], where, pre64)]
        sf, flips = lh.sign_check(case.id, sites, pre64, where)
        print(f"TILESIGN {case.id}@{kind} flips={flips}")
        fails += sf
        if flips:
            _, _, g64 = lh.reference(case, masks=sites, keeps=keeps)
    g64, e32 = _unused(case, g64, e32)
    ref = dict(out=out64, **g64)
    _grads("rows", case, a, ref, e32, fails)
    bits_apply = kind == "tiles" and not case.p and (relu_class or case.act == "identity")
    if bits_apply:   # the sign-bit form: the same output bit for bit, its gradients against the reference given the SAME decisions
        b = th.run_tile(dev, case, kind, bits=True)
        assert b["st"].args.keep_bits and b["sites"] is None
        if not torch.equal(a["out"].view(torch.int32), b["out"].view(torch.int32)):
            fails.append("bits: the output differs from the run that kept fp32 rows")
        _grads("bits", case, b, ref, e32, fails)
    else:
        assert not th.run_tile(dev, case, kind, bits=True, backward=0)["st"].args.keep_bits, "sign bits where the library refuses them"
    if not case.p:   # the inference forward (the KEEP = false builds; beyond the tile: the spill scratch)
        inf = th.run_tile(dev, case, kind, keep=False)
        fails += [f"inference: {f}" for f in rh.compare(f"{case.id}/inference", dict(out=inf["out"]), dict(out=out64), e32, "fwd", margin=MARGIN, report=_report)]
    if case.graph in BOND_ONLY:
        assert float(ref["W_h"].abs().max()) == 0.0   # (compare() then demands exactly zero)
    assert not fails, f"{case.id}@{kind}: " + "; ".join(fails)


@gpu
@pytest.mark.parametrize("run", RUNS, ids=_ids)
def test_tile_route(run, gpu_device):
    case, kind = run
    out64, pre64, g64, e32, _ = lh.yardsticks(case)
    _hold(gpu_device, case, kind, out64, pre64, g64, e32)


@gpu
@pytest.mark.parametrize("case", KEPT, ids=lambda c: c.id)
def test_tile_kept_forms(case, gpu_device, monkeypatch):
    """The three kept forms on one shape — fp32 rows, sign bits, split message rows (``DMPNN_KEEP_ROWS`` 1 | 0) — on both plans: the
    outputs of all six runs are bit-identical (the graph's caller order IS its CSR-row order: both plans see the same rows in the
    same order), every run's gradients hold the bar.  At ``d_h`` 132 and 256 the library keeps no split rows (see the module docstring)."""
    from chemprop_amd import engine

    out64, pre64, g64, e32, _ = lh.yardsticks(case)
    ref = dict(out=out64, **g64)
    fails, outs, masks = [], {}, None
    for rows in ("0", "1"):
        monkeypatch.setenv("DMPNN_KEEP_ROWS", rows)
        for kind, bits in (("full", False), ("tiles", False), ("tiles", True)):
            tag = f"{kind}-{'bits' if bits else 'fp32'}-rows{rows}"
            r = th.run_tile(gpu_device, case, kind, bits=bits)
            assert bool(r["st"].args.keep_bits) == bits
            assert bool(r["st"].args.msplit) == (rows == "1" and th.keeps_rows(case.d_h)), (tag, "split rows")
            if bool(r["st"].args.msplit):
                assert torch.isfinite(engine.split_rows_to_float(r["st"].refs[-3], case.d_h)).all(), (tag, "the kept split rows")
            if r["sites"] is not None:
                sf, flips = lh.sign_check(case.id, r["sites"], pre64)
                fails += [f"{tag}: {f}" for f in sf]
                if masks is None:
                    masks = r["sites"]
                    if flips:
                        ref = dict(out=out64, **lh.reference(case, masks=masks)[2])
                elif not all(torch.equal(x, y) for x, y in zip(masks, r["sites"])):
                    fails.append(f"{tag}: the kept decisions differ from the first run's")
            outs[tag] = r["out"]
            _grads(tag, case, r, ref, e32, fails)
    first = next(iter(outs.values()))
    fails += [f"{tag}: the output differs from the first form's" for tag, o in outs.items() if not torch.equal(o.view(torch.int32), first.view(torch.int32))]
    assert not fails, f"{case.id}: " + "; ".join(fails)


@gpu
@pytest.mark.parametrize("case", DROPOUT, ids=lambda c: c.id)
@pytest.mark.parametrize("kind", th.PLANS)
def test_tile_route_with_dropout(case, kind, gpu_device):
    """``p = 0.25`` inside the tile kernels: the masks rebuilt from ``dmpnn_dropout_keep`` — an edge site hashes the CALLER's edge id on
    either plan, the finalize the atom id — and handed to the float64 reference; what a mask dropped is exactly zero; no sign bits."""
    bmg = lh.graph(case.graph)
    keeps = lh.keep_masks(case, int(bmg.edge_index.shape[1]), int(bmg.V.shape[0]))
    out64, pre64, g64 = lh.reference(case, keeps=keeps)
    out32, _, _ = lh.reference(case, torch.float32, keeps=keeps, grads=False)
    _, _, g32 = lh.reference(case, torch.float32, masks=lh.true_masks(pre64), keeps=keeps)
    e32 = rh.yardstick(dict(out=out64, **g64), dict(out=out32, **g32))
    assert 0.6 < float(keeps[0].float().mean()) < 0.9
    res = th.run_tile(gpu_device, case, kind, backward=0)
    assert bool((res["out"][~keeps[-1]] == 0).all()), "an entry the finalize's mask drops is exactly zero"
    for t in range(case.depth - 1):
        assert not bool(res["sites"][t + 1][~keeps[t]].any()), f"site {t + 1}: an entry the mask drops is exactly zero in the kept H"
    _hold(gpu_device, case, kind, out64, pre64, g64, e32, keeps=keeps)


@gpu
def test_tile_plans_are_the_edges_the_cases_name(gpu_device):
    """The plan the device builds — either kind — has the tiles ``tile_harness.tile_rule`` restates, oversize count
    (``DMPNN_HDR_NSPILL``) included, and the launches have the wave count their case ids claim on this device."""
    from chemprop_amd import _lib

    for name in EDGE_GRAPHS + ("chains3x1700", "qm9x12", "qm9x12@rows", "chains12x10@mol", "degrees@mol"):
        for kind in th.PLANS:
            plan, _ = th.plan_of(name, kind, gpu_device)
            tr, ta, over = th.tile_rule(name, kind)
            hdr, arr = plan.header(), plan.arrays()
            n = len(tr) - 1
            assert hdr[th.HDR_NMTILES] == n and hdr[th.HDR_NSPILL] == over, (name, kind, hdr[:10], n, over)
            assert arr["mtile_row"][:n + 1].tolist() == tr.tolist() and arr["mtile_atom"][:n + 1].tolist() == ta.tolist(), (name, kind)
    lib = _lib.load()
    cus = torch.cuda.get_device_properties(gpu_device).multi_processor_count
    for name in ("bonds2600", "chains3x1700", "qm9x12"):
        bmg = lh.graph(name)
        nV, nE = int(bmg.V.shape[0]), int(bmg.edge_index.shape[1])
        for h in (132, 300):
            want = 8 if name == "qm9x12" else 4
            assert lib.dmpnn_tile_waves(nV, nE, h, 0) == th.tile_waves_rule(nV, nE, h, cus) == want, (name, h, cus)


# ---- where no GPU is needed ----------------------------------------------------------------------------------------------------------
def test_tile_graphs_on_cpu():
    """Every graph has the tiles its name claims, under the packing rule restated with ``oracle.collate_numpy``; its edges lie molecule
    by molecule, shuffled inside; ``rev`` is the involution of a symmetric graph."""
    from oracle import collate_numpy as cn

    def rule(name, kind="tiles"):
        tr, ta, over = th.tile_rule(name, kind)
        return np.diff(tr).tolist(), np.diff(ta).tolist(), over

    assert rule("chain25") == ([48], [25], 0) and rule("chain26") == ([50], [26], 1) and rule("star24") == ([48], [25], 0)
    assert int(rh.in_degrees(lh.graph("star24")).max()) == 24
    assert rule("ions32") == ([4], [32], 0) and rule("ions33") == ([4], [33], 1)
    assert rule("ions33", "full") == ([4, 0], [32, 1], 0), "the full plan packs connected pieces: no molecule of 33 atoms there"
    assert rule("atoms40") == ([0, 2], [32, 10], 0) and rule("pack-exact") == ([48, 2], [27, 2], 0)
    rows, atoms, over = rule("mixed-oversize")
    assert over == 1 and rows[2] == 50 and max(rows[:2] + rows[3:]) <= 48 and len(rows) == len(rule("qm9x12")[0]) + 1
    rows, atoms, over = rule("bonds2600")
    assert set(rows) == {32, 16} and set(atoms) == {32, 16} and len(rows) == 163 and over == 0   # (a tile starts at every block of 64 molecules)
    nV = int(lh.graph("bonds2600").V.shape[0])
    assert th.tile_waves_rule(nV, nV, 300, 256) == 4 and th.tile_waves_rule(nV - 400, nV - 400, 300, 256) == 8 and th.tile_waves_rule(nV, nV, 128, 256) == 4
    from chemprop_amd import engine
    assert engine.small_plan_fits(nV, nV) and engine.small_plan_fits(5100, 6800) and th.tile_waves_rule(5100, 6800, 300, 256) == 4
    rows, atoms, over = rule("chains3x1700")
    assert max(rows) == 40 and max(atoms) == 30 and over == 0 and int(rh.in_degrees(lh.graph("chains3x1700")).max()) == 2
    for name in EDGE_GRAPHS + ("qm9x12", "chains12x10@mol", "degrees@mol", "qm9x12@rows"):
        bmg = lh.graph(name)
        src, dst = bmg.edge_index
        rev = bmg.rev_edge_index
        assert torch.equal(src[rev], dst) and torch.equal(rev[rev], torch.arange(rev.numel())), name
        mol = bmg.batch[src]
        assert bool((mol[1:] >= mol[:-1]).all()) and torch.equal(mol, bmg.batch[dst]), f"{name}: edges molecule by molecule"
        atoms, rows = th.pieces(bmg, "tiles")
        if len(atoms) < 64:   # (one block of molecules: the device planners' rule IS the greedy loader rule)
            assert all(np.array_equal(x, y) for x, y in zip(cn.greedy_molecule_tiles(atoms, rows), cn.blocked_molecule_tiles(atoms, rows))), name
        if name in EDGE_GRAPHS and name not in ("bonds2600", "atoms40"):
            assert not torch.equal(rh.csr_tables(bmg)["perm"], torch.arange(rev.numel())), f"{name}: shuffled inside the molecules"
    assert torch.equal(rh.csr_tables(lh.graph("qm9x12@rows"))["perm"], torch.arange(int(lh.graph("qm9x12").edge_index.shape[1])))


def test_tile_references_on_cpu():
    """Every case's seed: the float32 oracle's own decisions stay inside the band, every yardstick under its cap, no reference tensor is
    identically zero unless it must be (``W_h``'s gradient on the bond-only graphs — which the kernels then have to give exactly)."""
    for case in CASES + KEPT:
        out64, pre64, g64, e32, fails32 = lh.yardsticks(case)
        assert not fails32, (case.id, fails32)
        assert len(pre64) == case.depth + 1
        assert e32["out"] < rh.CAP["fwd"] and max(v for k, v in e32.items() if k != "out") < rh.CAP["grad"], (case.id, e32)
        want = {"W_i", "W_h", "W_o", "b_o"} | ({"b_i", "b_h"} if case.bias else set())
        assert set(g64) == (want - {"W_h", "b_h"} if case.depth == 1 else want), case.id
        for k, t in dict(out=out64, **g64).items():
            assert (float(t.abs().max()) > 0) != (case.graph in BOND_ONLY and k == "W_h"), (case.id, k)
        lh.yardsticks.cache_clear()
    for case in DROPOUT:
        bmg = lh.graph(case.graph)
        _, pre64, _ = lh.reference(case, grads=False)
        _, pre32, _ = lh.reference(case, torch.float32, grads=False)
        assert not lh.sign_check(case.id, lh.true_masks(pre32), pre64)[0], case.id
    # a smooth activation takes no masks: the reference given "decisions" is the reference
    case = next(c for c in CASES if c.id == "h36-tanh-bias")
    _, pre64, g64 = lh.reference(case)
    _, _, gm = lh.reference(case, masks=lh.true_masks(pre64))
    assert all(torch.equal(g64[k], gm[k]) for k in g64)


def _args(d_h=36, d_v=6, d_e=4, depth=3, act="relu", p=0.0, ldout=None, nV=110, nE=102, flags=0):
    from chemprop_amd import _lib

    a = _lib.FwdArgs()
    a.n_atoms, a.n_edges, a.d_v, a.d_e, a.d_h, a.depth = nV, nE, d_v, d_e, d_h, depth
    a.flags = flags
    a.ldv, a.lde, a.ldh, a.ldout = d_v, d_e, (d_h + 3) // 4 * 4, d_h if ldout is None else ldout
    a.act, a.dropout_p = _lib.ACT[lh.ENGINE_ACT.get(act, (act,))[0]], p
    return a


def test_tile_refusal_table_on_cpu(monkeypatch):
    """``dmpnn_forward_can_fuse`` (2: the tile kernel), ``dmpnn_forward_keep_bits_bytes`` on a tile-plan training block and
    ``dmpnn_train_route``: every swept shape is accepted; ``d_h`` 2, 6, 324, an odd ``d_v`` / ``d_e``, ``d_v + d_h = 450``, ``ldout % 4 != 0``
    and an undirected block are not; no sign bits for a smooth activation or with dropout; split message rows only where the kernel's
    tile row is the kept row (``d_h <= 128`` or ``256 < d_h <= 320``)."""
    from chemprop_amd import _lib, engine

    lib = _lib.load()
    fuse = lambda a: int(lib.dmpnn_forward_can_fuse(C.byref(a)))
    TRAIN = _lib.F_FUSED | _lib.F_MEGA | _lib.F_SPLIT16 | _lib.F_KEEP | _lib.F_TILE_PLAN
    bits = lambda **kw: int(lib.dmpnn_forward_keep_bits_bytes(C.byref(_args(flags=TRAIN, **kw))))
    monkeypatch.delenv("DMPNN_MEGA", raising=False)
    monkeypatch.delenv("DMPNN_MFMA", raising=False)
    monkeypatch.setenv("DMPNN_KEEP_ROWS", "1")
    route = lambda c, **kw: engine.train_route(110, 102, c.d_v, c.d_e, c.d_h, c.depth, lh.ENGINE_ACT[c.act][0], 12, have_batch=True, dropout_p=c.p, **kw)
    for case in CASES + KEPT + DROPOUT:
        assert fuse(_args(case.d_h, case.d_v, case.d_e, case.depth, case.act, ldout=case.d_h + case.pad)) == 2, case.id
        nb = bits(d_h=case.d_h, d_v=case.d_v, d_e=case.d_e, depth=case.depth, act=case.act, p=case.p)
        assert (nb > 0) == (case.act in ("relu", "leakyrelu", "identity") and not case.p) and nb % (case.depth * 2048) == 0, (case.id, nb)
        info = route(case)
        assert _lib.ROUTES[info.route] == "mega16" and info.plan_kind == 2, case.id
        assert info.keep_bits == int(case.act in ("relu", "leakyrelu", "identity") and not case.p), case.id
        assert info.keep_rows == int(case.depth > 1 and th.keeps_rows(case.d_h)), case.id
    assert [h for h in WIDTHS if not th.keeps_rows(h)] == [132, 192, 196, 256]
    refused = (dict(d_h=2), dict(d_h=6), dict(d_h=324), dict(d_v=7), dict(d_e=3), dict(d_v=130, d_h=320), dict(ldout=38), dict(flags=_lib.F_UNDIRECTED))
    assert [fuse(_args(**kw)) for kw in refused] == [0, 0, 0, 0, 0, 1, 1, 0]
    assert fuse(_args(d_v=128, d_h=320)) == 2 and fuse(_args(ldout=40)) == 2
    for kw in (dict(d_h=2), dict(d_h=6), dict(d_h=324), dict(d_v=7), dict(d_e=3), dict(d_v=130, d_h=320)):
        c = Case("refused", "qm9x12", **{"d_h": 36, **kw})
        assert _lib.ROUTES[route(c).route] != "mega16", kw
    assert _lib.ROUTES[route(Case("undirected", "qm9x12", 36), undirected=True).route] != "mega16"
    assert bits(act="tanh") == 0 and bits(act="elu") == 0 and bits(p=0.25) == 0 and bits() > 0
    monkeypatch.setenv("DMPNN_KEEP_ROWS", "0")
    assert route(KEPT[0]).keep_rows == 0
