"""The LEAN per-step training route — ``fused16_lean`` / ``k_step16`` forward (csrc/dmpnn_step16.hip), one ``k_bstep16<WN>`` launch
per depth step backward (csrc/dmpnn_bstep16.hip), the split-row products ``k_wgrad16r`` (csrc/dmpnn_wgrad16.hip) — through
``engine.forward(..., keep=True, route="fused16")`` / ``engine.backward`` at the edges of its dispatch, against float64 on the CPU
(``tests/lean_harness.py``).  This is the route that trains every molecule beyond the tile.

The shapes are the smallest at which each branch can still go wrong; the id of a case names its edge.  The output and every gradient
are held in a metric WITHOUT a floor, ``err = max|got - ref| / max|ref|`` over every entry, to ``min(MARGIN max(e32, 2**-23), cap)``:
``e32`` is what the float32 oracle gives on the very same inputs against float64, ``cap`` 1e-5 for the output and 2e-5 for gradients.
``out`` and every gradient live in NaN-prefilled buffers whose guard regions must come back untouched; two backward passes must
agree bit for bit.

The ReLU kink: the kept bits (``engine.lean_sign_bits``) and the sign of the output are compared with the float64 pre-activation
signs — an entry may differ only where the float64 ``|z|`` is below ``64 * 2**-24 * max|z|`` of its tensor, and at most two entries of a
case may differ (a condition, not a measurement) — and the gradient reference is the float64 backward GIVEN the kernel's own
decisions.  ``test_lean_references_on_cpu`` holds the float32 oracle's own decisions to the same rule for every case's seed.  The
``identity`` cases (one per ``WN``) need no decisions at all and hold everything unconditionally: LeakyReLU with slope 1 —
``dmpnn_forward`` refuses ``DMPNN_ACT_NONE`` on every route, so the lean kernels' branch without kept bits is not reachable (pinned by
``test_lean_route_activation_none_is_refused_by_the_forward``).  Likewise ``d_v + d_e = 2`` would need ``d_e = 0``, whose empty ``E``
the forward refuses as a null pointer: the smallest accepted operand is ``d_v + d_e = 4``.

Every GPU test carries ``pytest.mark.gpu`` itself; the ``*_on_cpu`` tests check the references, the restated tile and row-split
rules and the refusal table where no GPU is needed.

MARGIN (``rows_harness.MARGIN`` = 16, unchanged).  Measured on the MI355X with the report lines of every case (62 GPU tests, 334
tensor comparisons): the worst ``err / max(e32, 2**-23)`` is 7.38 — ``gW_h`` of ``h4-isolated300``: two chains of three atoms whose
products cancel to ``max|ref|`` = 0.02, err 8.8e-7 of that (1.8e-8 absolute) against a float32 draw of 6.2e-8.  The next are 2.45
(``gb_i``, ``h60-bias``), 2.45 (``out``, ``h300-nobias``), 2.16 (``gW_i``, ``h36-x4``), 2.10 (``gW_o``, ``h68-single-bond`` and
``h4-bonds25``), 1.94 (``gb_h``), 1.83 (``gb_o``).  2 x 7.38 = 14.8 <= 16: MARGIN stays.  With ``e32`` of 0.5e-7 .. 5e-7 the bars are
1.9e-6 .. 8.4e-6; one tensor sits at its cap (``gW_i`` of ``h64-product-split``: float32 sums 7 000 rows to 1.6e-6, the kernels to
2.7e-7).  No case flipped a decision (0 of at most 2 everywhere).  ``gW_h`` of the bond-only graphs is exactly zero in float64 (every
message is) and exactly zero from the kernels.  Wall time of the module's GPU tests on the MI355X: 3.2 s.

What the sweep found.  (1) ``d_h = 4`` (``qn == 1``, ``qmagic_of(4) == 0``): the gather of the first backward launch took row 0 for
every DMA piece and read ``gMv[dst[rs] + lane]`` instead of ``gMv[dst[rs + lane]]``.  Before the guard in ``k_bstep16`` five cases
failed: ``h4-nobias`` (``gW_i`` err 6.4e-1, ``gW_h`` 1.0e-1), ``h4-degrees-in-order`` (7.0e-1, 6.5e-1; ``gb_i`` 4.7e-1, ``gb_h`` 1.2),
``h4-one-row-tile`` (1.1, 8.6e-1), ``h4-isolated300`` (1.9, 4.3e+1), ``h4-depth3`` (7.3e-1, 7.7e-1); ``out`` and ``gW_o`` were right, and
``h4-single-bond`` / ``h4-bonds24`` / ``h4-bonds25`` passed (in-degree 1 everywhere: row ``r`` has destination atom ``r``, so
``dst[rs] + lane`` IS ``dst[rs + lane]``).  (2) ``ldh != d_h``: ``k_bstep16``'s message mode
fetches a tile's rows as one contiguous run, so ``fused16_lean_shapes`` now refuses a padded ``ldh``
(``test_lean_refusal_table_on_cpu`` failed on its ``ldh = d_h + 4`` lines before).

Tried against deliberately wrong builds (scratch copies, never committed), the module run once on each: the ``r1 - r0 <= 4`` branch of
``k_bstep16`` taking 5 rows fails all 36 cases on ``degrees`` / ``degrees-in-order`` (the only graphs with an in-degree of 5) and
nothing else; the sign bits of site ``t - 1`` fail 45: every ReLU / LeakyReLU case but ``h4-single-bond`` (8 bits that agree between
the two sites) and none of the nine ``identity`` cases, as it must be; the zero-row flag always 0 fails exactly ``h36-zero-tiles``
and ``h300-zero-tiles``; ``T_next`` written to ``r`` and not to ``rev r`` fails 49: all but the six bond-only cases, where every message
is zero.  The first form of the depth 3 / depth 8 cases ran on the stars of ``degrees`` and PASSED the wrong-site build: on a star
``H^(t)`` is constant from ``t = 1`` on and no gradient reaches a site more than two steps back.  They now run on chains of ten atoms
and on QM9-shaped molecules, where that build fails them.
"""
import ctypes as C

import pytest
import torch

import lean_harness as lh
import rows_harness as rh
from lean_harness import Case

MARGIN = lh.MARGIN
gpu = pytest.mark.gpu
# d_h at the seams of the builds: k_bstep16<1..5> (64-column blocks), partial 32-column chunks (4, 8, 36, 60, 68, ..), partial
# 16-column tiles (4, 8, 36, 60, 68, 132, 196, 260, 300) and qn == 1 (d_h = 4: one float4 per row, no magic division)
WIDTHS = (4, 8, 36, 60, 64, 68, 128, 132, 192, 196, 256, 260, 300, 320)
IDENTITY_PER_WN = (60, 128, 192, 256, 300)
EDGE_GRAPHS = ("degrees-in-order", "single-bond", "bonds24", "bonds25", "one-row-tile", "isolated300")


def _cases():
    cs = [Case(f"h{h}-{'bias' if i % 2 else 'nobias'}", "degrees", h, bias=bool(i % 2)) for i, h in enumerate(WIDTHS)]
    cs += [Case(f"h{h}-identity-WN{(h + 63) // 64}", "degrees", h, act="identity", bias=h == 128) for h in IDENTITY_PER_WN]
    cs += [Case(f"h{h}-{act}-{'bias' if b else 'nobias'}", "degrees", h, act=act, bias=b)
           for h in (36, 132) for act in ("leakyrelu", "identity", "relu") for b in (True, False) if not (act == "relu" and not b and h == 36)]
    cs += [Case(f"h{h}-{g}", g, h, bias=True) for g in EDGE_GRAPHS for h in (4, 68)]
    # (depth > 2 on graphs with long paths: on the stars of "degrees" every H^(t) equals H^(1) and no gradient reaches a site more than
    #  two steps back — a build that mixes up the sites would pass there)
    cs += [Case("h36-depth3", "qm9x12", 36, depth=3, bias=True), Case("h4-depth3", "chains12x10", 4, depth=3),
           Case("h36-depth8-leakyrelu", "chains12x10", 36, depth=8, act="leakyrelu", bias=True), Case("h132-depth8", "qm9x12", 132, depth=8)]
    cs += [Case("h36-x4", "degrees", 36, d_v=2, d_e=2), Case("h36-x34", "degrees", 36, d_v=30, d_e=4, bias=True),
           Case("h68-x256", "degrees", 68, d_v=200, d_e=56, bias=True)]
    cs += [Case("h36-padded-out-and-gout", "degrees", 36, pad=4, bias=True), Case("h300-padded-out-and-gout", "qm9x12", 300, depth=3, pad=12)]
    cs += [Case("h36-zero-tiles", "chains30x6", 36, gmode="zero-tiles", bias=True), Case("h300-zero-tiles", "chains30x6", 300, gmode="zero-tiles")]
    cs += [Case("h64-product-split", "chains-split", 64, d_v=30, d_e=4, bias=True)]
    assert len({c.id for c in cs}) == len(cs)
    return cs


CASES = _cases()
DROPOUT = Case("h36-dropout-depth3", "qm9x12", 36, depth=3, p=0.25, bias=True)
DEG25 = Case("h36-degree25", "degree25", 36, bias=True)
NOT_LEAN = [Case("h36-depth1", "degrees", 36, depth=1, bias=True), Case("h36-depth9", "degrees", 36, depth=9, bias=True),
            Case("h36-x258", "degrees", 36, d_v=202, d_e=56, bias=True)]


def _report(s):
    print(s.replace("ROWSBAR", "LEANBAR"))


def _hold(case, res, out64, pre64, g64, e32, keeps=None):
    """The whole contract of one lean run: the route, the kept decisions, the output, every gradient, the two passes."""
    assert res["st"].route == "fused16/lean", res["st"].route
    fails = []
    masks = None
    if case.act != "identity":
        # the decisions the kernels took: the kept bits at the edge sites, the sign of the output at the finalize (where dropout zeroed an
        # entry it says nothing: the float64 decision stands in, times zero)
        fin = res["out"] > 0
        where = [None] * case.depth + [None if keeps is None else keeps[-1]]
        if keeps is not None:
            fin = torch.where(keeps[-1], fin, pre64[-1] > 0)
        masks = [res["bits"][t] for t in range(case.depth)] + [fin]
        sf, flips = lh.sign_check(case.id, masks, pre64, where)
        print(f"LEANSIGN {case.id} flips={flips}")
        fails += sf
        if flips:
            _, _, g64 = lh.reference(case, masks=masks, keeps=keeps)
    fails += rh.compare(case.id, dict(out=res["out"], **res["grads"][0]), dict(out=out64, **g64), e32,
                        dict(out="fwd", **{k: "grad" for k in lh.GRADS}), margin=MARGIN, report=_report)
    a, b = res["grads"]
    for k in a:
        if not torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)):
            fails.append(f"g{k}: two backward passes differ")
    assert not fails, f"{case.id}: " + "; ".join(fails)


@gpu
@pytest.mark.parametrize("case", CASES, ids=lambda c: c.id)
def test_lean_route(case, gpu_device):
    out64, pre64, g64, e32, _ = lh.yardsticks(case)
    _hold(case, lh.run_lean(gpu_device, case), out64, pre64, g64, e32)


@gpu
def test_lean_route_with_dropout(gpu_device):
    """``p = 0.25`` inside the step kernels: the masks rebuilt from ``dmpnn_dropout_keep`` and handed to the float64 reference; the kept
    bit is the sign BEFORE the mask; what the finalize's mask dropped is exactly zero."""
    case = DROPOUT
    bmg = lh.graph(case.graph)
    keeps = lh.keep_masks(case, int(bmg.edge_index.shape[1]), int(bmg.V.shape[0]))
    out64, pre64, g64 = lh.reference(case, keeps=keeps)
    # (the yardstick: float32 on the same inputs with the same masks, its gradients given the float64 decisions)
    out32, _, _ = lh.reference(case, torch.float32, keeps=keeps, grads=False)
    _, _, g32 = lh.reference(case, torch.float32, masks=lh.true_masks(pre64), keeps=keeps)
    e32 = rh.yardstick(dict(out=out64, **g64), dict(out=out32, **g32))
    res = lh.run_lean(gpu_device, case)
    assert bool((res["out"][~keeps[-1]] == 0).all()), "an entry the finalize's mask drops is exactly zero"
    assert 0.6 < float(keeps[0].float().mean()) < 0.9
    _hold(case, res, out64, pre64, g64, e32, keeps=keeps)


@gpu
def test_lean_route_plans_are_the_edges_the_cases_name(gpu_device):
    """The plan the device builds has the tiles the case ids claim (the restated rule of ``lean_harness.tile_table``), and the one
    product launch of the backward pass splits its rows as ``lean_harness.wgrad16r_rows`` says for this device."""
    want = {"degrees": 5, "bonds24": 1, "bonds25": 2, "one-row-tile": 2, "isolated300": 1, "single-bond": 1, "chains30x6": 7}
    for name, n_tiles in want.items():
        bmg = lh.graph(name)
        _, arr = lh.plan_of(name, gpu_device)
        tile, rows = lh.tile_table(bmg)
        assert int(arr["hdr"][4]) == n_tiles == rows.numel(), (name, int(arr["hdr"][4]), rows.tolist())
        assert torch.equal(arr["tile_row"][:n_tiles + 1], torch.cat((torch.zeros(1, dtype=torch.int64), torch.cumsum(rows, 0)))), name
        first = torch.tensor([int((tile < t).sum()) for t in range(n_tiles + 1)])
        assert torch.equal(arr["tile_atom"][:n_tiles + 1], first), name
    assert int(lh.plan_of("degree25", gpu_device)[1]["hdr"][0]) & 4, "in-degree 25: PLAN_HUGE_DEGREE"
    cus = torch.cuda.get_device_properties(gpu_device).multi_processor_count
    case = next(c for c in CASES if c.id == "h64-product-split")
    (r_h, s_h), (r_i, s_i), r0 = lh.wgrad16r_rows(10 * lh.SPLIT_CHAINS, case.d_h, case.d_v + case.d_e, case.depth, cus)
    assert r0 > 32 and min(s_h, s_i) > 1, (cus, r0, r_h, s_h, r_i, s_i)


@gpu
def test_lean_route_degree_25_is_nan_not_a_fault(gpu_device):
    """An in-degree beyond the tiling (24): the plan says so, every output and every gradient is NaN — a value, not a fault — and the
    guard regions stay untouched."""
    res = lh.run_lean(gpu_device, DEG25, backward=1)
    assert res["st"].route == "fused16/lean"
    assert bool(torch.isnan(res["out"]).all()), "out"
    for k, g in res["grads"][0].items():
        assert bool(torch.isnan(g).all()), k


@gpu
@pytest.mark.parametrize("case", NOT_LEAN, ids=lambda c: c.id)
def test_lean_route_is_not_reported_outside_its_shapes(case, gpu_device):
    """Depth 1, depth 9 (``kWProdMaxJobs`` is 8) and ``d_v + d_e = 258``: ``route="fused16"`` keeps fp32 tensors (``st.route`` is
    ``fused16``, not the lean form) and still computes the block."""
    out64, _, _, e32, _ = lh.yardsticks(case)
    res = lh.run_lean(gpu_device, case, backward=0)
    assert res["st"].route == "fused16", res["st"].route
    fails = rh.compare(case.id, dict(out=res["out"]), dict(out=out64), e32, "fwd", margin=MARGIN, report=_report)
    assert not fails, "; ".join(fails)


@gpu
def test_lean_route_activation_none_is_refused_by_the_forward(gpu_device, monkeypatch):
    """``dmpnn_forward`` takes no ``DMPNN_ACT_NONE`` on any route, the lean form included (whose size rule does answer for it): the
    identity of this sweep is LeakyReLU with slope 1."""
    from chemprop_amd import _lib

    monkeypatch.setitem(lh.ENGINE_ACT, "identity", ("none", 0.0))
    with pytest.raises(_lib.DmpnnError, match="not built in"):
        lh.run_lean(gpu_device, next(c for c in CASES if c.id == "h60-identity-WN1"), backward=0)


@gpu
def test_lean_route_refuses_an_odd_d_v(gpu_device):
    with pytest.raises(RuntimeError, match="fused16"):
        lh.run_lean(gpu_device, Case("h36-odd-d_v", "degrees", 36, d_v=7, d_e=4), backward=0)


# ---- where no GPU is needed ----------------------------------------------------------------------------------------------------------
def test_lean_references_on_cpu():
    """Every case's seed: the float32 oracle's own decisions differ from the float64 signs only inside the band (so a flip of the
    kernel's outside it is the kernel's); every yardstick stays under its cap (``MARGIN * e32`` decides, not the cap); no reference
    tensor is identically zero; the reference given the TRUE decisions is the reference."""
    for case in CASES + NOT_LEAN:
        out64, pre64, g64, e32, fails32 = lh.yardsticks(case)
        assert not fails32, (case.id, fails32)
        assert len(pre64) == case.depth + 1
        assert e32["out"] < rh.CAP["fwd"] and max(v for k, v in e32.items() if k != "out") < rh.CAP["grad"], (case.id, e32)
        want = {"W_i", "W_h", "W_o", "b_o"} | ({"b_i", "b_h"} if case.bias else set())
        assert set(g64) == (want - {"W_h", "b_h"} if case.depth == 1 else want), case.id
        only_bonds = case.graph in ("single-bond", "bonds24", "bonds25")   # in-degree 1 everywhere: every message is exactly zero, and so
        for k, t in dict(out=out64, **g64).items():                        # is W_h's gradient — which the kernels then have to give EXACTLY
            assert (float(t.abs().max()) > 0) != (only_bonds and k == "W_h"), (case.id, k)
        lh.yardsticks.cache_clear()
    case = CASES[2]
    _, pre64, g64 = lh.reference(case)
    _, _, gm = lh.reference(case, masks=lh.true_masks(pre64))
    assert all(torch.equal(g64[k], gm[k]) for k in g64)
    # one flipped decision moves a gradient far beyond every bar: what the conditioning is for
    masks = lh.true_masks(pre64)
    masks[1] = masks[1].clone()
    masks[1][3, 5] = ~masks[1][3, 5]
    _, _, gf = lh.reference(case, masks=masks)
    assert max(float((gf[k] - g64[k]).abs().max() / g64[k].abs().max()) for k in ("W_i", "W_h")) > 1e-4
    assert lh.sign_check("flip", masks, pre64)[0], "a flip away from the kink is a failure"
    # zero-gradient tiles: whole tiles of G are zero beside tiles of magnitude 1e-6
    zc = next(c for c in CASES if c.id == "h36-zero-tiles")
    tile, rows = lh.tile_table(lh.graph(zc.graph))
    G = lh.inputs(zc)["G"]
    assert rows.numel() == 7 and bool((G[tile % 3 == 0] == 0).all()) and 1e-7 < float(G[tile % 3 != 0].abs().max()) < 1e-5


def test_lean_graphs_and_split_rule_on_cpu():
    """The graphs have the in-degrees and tiles their names claim; the products' row-split rule restated: beyond 32 .. 96 rows every
    case already has ``splits > 1``; the product-split case is the smallest chain count at which the launch GROWS its rows per
    workgroup beyond the 32-row stage (256 compute units)."""
    assert set(rh.in_degrees(lh.graph("degrees")).tolist()) == set(lh.DEGREES)
    assert int(rh.in_degrees(lh.graph("degree25")).max()) == 25 and lh.tile_table(lh.graph("degree25")) == (None, None)
    rows = lambda n: lh.tile_table(lh.graph(n))[1].tolist()
    assert rows("bonds24") == [48] and rows("bonds25") == [48, 2] and rows("one-row-tile") == [47, 1] and rows("single-bond") == [2]
    assert rows("isolated300") == [8] and int(lh.graph("isolated300").V.shape[0]) == 306 > 255
    assert len(rows("degrees")) == 5 and max(rows("degrees")) <= 48 and len(rows("chains30x6")) == 7
    for name in ("degrees", "bonds25", "one-row-tile", "isolated300", "chains30x6"):
        bmg = lh.graph(name)
        src, dst = bmg.edge_index
        rev = bmg.rev_edge_index
        assert torch.equal(src[rev], dst) and torch.equal(rev[rev], torch.arange(rev.numel()))
        assert not torch.equal(rh.csr_tables(bmg)["perm"], torch.arange(rev.numel())), f"{name}: the caller's order is shuffled"
    assert torch.equal(rh.csr_tables(lh.graph("degrees-in-order"))["perm"].sort().values, torch.arange(102))
    # splits > 1: from 33 rows at the widest stage cost (K = 128: 32 rows per workgroup), from 97 at the narrowest
    first = lambda h, dx: next(n for n in range(2, 4096, 2) if max(s for _, s in lh.wgrad16r_rows(n, h, dx, 2)[:2]) > 1)
    assert first(128, 10) == 34 and first(4, 2) == 98
    assert all(max(s for _, s in lh.wgrad16r_rows(102, c.d_h, c.d_v + c.d_e, c.depth)[:2]) > 1 for c in CASES if c.graph == "degrees")
    assert max(s for _, s in lh.wgrad16r_rows(2, 4, 10, 2)[:2]) == 1
    # the product-split case: the smallest number of 6-atom chains (10 rows each) at which the launch grows its rows per workgroup
    c = next(c for c in CASES if c.id == "h64-product-split")
    grown = lambda n: lh.wgrad16r_rows(10 * n, c.d_h, c.d_v + c.d_e, c.depth)[2] > 32
    n0 = next(n for n in range(1, 3000) if grown(n))
    assert n0 <= lh.SPLIT_CHAINS <= n0 + 50 and 10 * lh.SPLIT_CHAINS < 30000, n0


def _args(d_h=36, d_v=6, d_e=4, depth=2, act="relu", p=0.0, ldh=None, nV=110, nE=102):
    from chemprop_amd import _lib

    a = _lib.FwdArgs()
    a.n_atoms, a.n_edges, a.d_v, a.d_e, a.d_h, a.depth = nV, nE, d_v, d_e, d_h, depth
    a.flags = _lib.F_FUSED | _lib.F_SPLIT16 | _lib.F_KEEP
    a.ldv, a.lde, a.ldh, a.ldout = d_v, d_e, d_h if ldh is None else ldh, d_h
    a.act, a.dropout_p = _lib.ACT[lh.ENGINE_ACT.get(act, (act,))[0]], p
    return a


def test_lean_refusal_table_on_cpu():
    """``dmpnn_forward_keep_bits_bytes`` on a lean argument block: ``depth * n_edges * block_cols(d_h) / 8`` bytes for every shape the
    sweep runs, 0 for what the route refuses — among them a padded ``ldh``: ``k_bstep16`` reads its rows as one contiguous run of
    ``d_h`` floats per row, so ``ldh = d_h + 4`` cannot be honoured (it was accepted before this test existed)."""
    from chemprop_amd import _lib

    lib = _lib.load()
    size = lambda a: int(lib.dmpnn_forward_keep_bits_bytes(C.byref(a)))
    for case in CASES + [DROPOUT, DEG25]:
        want = case.depth * 102 * ((case.d_h + 63) // 64 * 64 // 8)   # (the size rule reads no graph: 102 rows for all)
        assert size(_args(case.d_h, case.d_v, case.d_e, case.depth, case.act, case.p)) == want, case.id
    for h in WIDTHS:
        assert size(_args(h, ldh=h + 4)) == 0, f"d_h {h}: ldh = d_h + 4 must be refused"
        assert size(_args(h, ldh=h + 8, p=0.25)) == 0
    for case in NOT_LEAN:
        assert size(_args(case.d_h, case.d_v, case.d_e, case.depth)) == 0, case.id
    for kw in (dict(d_v=7), dict(d_e=3), dict(d_h=6), dict(d_h=324), dict(d_h=2), dict(act="tanh"), dict(act="none", p=0.25), dict(nE=0), dict(nV=0)):
        assert size(_args(**kw)) == 0, kw
    assert size(_args(depth=8)) == 4 * size(_args(depth=2)) > 0
