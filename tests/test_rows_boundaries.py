"""The row-level entries of ``include/dmpnn.h`` that no test called directly — ``dmpnn_linear_wgrad`` (+ ``_ws_bytes``),
``dmpnn_message_bwd``, ``dmpnn_aggregate_bwd``, ``dmpnn_gather_rows``, ``dmpnn_update_fwd`` — through the C ABI at the edges of their
dispatch, against float64 on the CPU (``tests/rows_harness.py``).

The shapes are the smallest at which each branch can still go wrong; the id of a case names its edge.  Arithmetic outputs are held
in a metric WITHOUT a floor, ``err = max|got - ref| / max|ref|`` over every entry, to ``min(MARGIN max(e32, 2**-23), cap)``: ``e32``
is what plain float32 PyTorch gives on the very same inputs against float64, ``cap`` the floored bar the suite already holds (2e-5
gradients, 1e-5 forward tensors).  Pure copies (``dmpnn_aggregate_bwd``, ``dmpnn_gather_rows``) are compared bit for bit.  Every
output lives in a NaN-prefilled buffer whose padding columns and guard region must come back untouched; the padding columns of the
inputs hold NaN.

Every GPU test carries ``pytest.mark.gpu`` itself (no module-wide mark): the two ``*_on_cpu`` tests check the references — the
adjoint identity of the message transpose, the graphs, the yardsticks against the caps — where no GPU is needed.

MARGIN (``rows_harness.MARGIN``, one number, shared with ``test_custom_activation_rows_route_gradients`` of
``tests/test_parity_gpu.py``).  Measured on the MI355X with the report lines of every case (the GPU tests here and the three
rows-route gradient cases: 1 057 tensor comparisons): the worst ``err / max(e32, 2**-23)`` is 4.74 — ``gb`` of
``f16-769chunks-target768`` (4.10 on ``f16-768chunks-target512``): the column sums of 24 608 rows, which the f16 pipe forms as the
product with a column of ones in 32-row chunks and 385 slabs, err 5.9e-7 against a float32 draw of 1.2e-7 (torch sums pairwise).  The
next are 2.09 (``Mv`` of ``dmpnn_update_fwd`` at ``d_h = 300``), 2.03 (``H_out``, tanh, ``d_h = 300``), 1.94 (``M_next``), 1.69
(``gb``, f16 pipe, graded columns), 1.59 (``gb``, fp32 pipe, 1 025 rows), 1.33 (rows-route gradients), 0.82 (``gW``, either pipe),
0.71 (``dmpnn_message_bwd``) — none stands out by an order of magnitude.  2 x 4.74 = 9.48 -> MARGIN = 16.  With ``e32`` of
1e-7 .. 5e-7 that is a relative bar of 2e-6 .. 8e-6 on every tensor, whatever its magnitude.
The per-row figures of the two graded cases (reported, not asserted): worst
``row error / float32's row error`` 0.75 on the fp32 pipe, 1.64 on the f16 pipe (a column scaled by ``2**-12``: row error 2.9e-7).
Wall time of the module's GPU tests on the MI355X: 5.5 s.

Tried against deliberately wrong builds (scratch copies, never committed): ``case 3:`` of ``k_edge_bwd`` running the in-degree-2 body
fails ``test_rows_message_and_aggregate_bwd[h4 | h64 | h260 | h300 | h8-padded-vector]`` (the scalar build has no switch: it loops
for every in-degree); the NaN row of ``k_gather_rows`` leaving its last column fails ``test_rows_gather_rows_index_out_of_range``
on both vector cases; the ones term at ``kt == K`` moved fails every fp32-pipe case with a bias; each of them also fails the
rows-route gradient test.  Dropping the ``n + 3 < a.N`` mask of ``wg_load_z`` fails nothing, ``f32-vecZ-last-float4-partial``
(which runs that line with NaN behind column ``N``) included: the mask is redundant — component ``jn`` of a lane's ``gZ`` load
feeds only output row ``n0 + 4 i + jn``, and rows ``>= N`` are dropped by the slab store.
"""
import dataclasses
import functools
import os

import pytest
import torch

import rows_harness as rh
from conftest import GOLDEN_DIR, Golden

MARGIN = rh.MARGIN
gpu = pytest.mark.gpu
DEGREES = (0, 1, 2, 3, 4, 5, 12)


def bits(t):
    return t.contiguous().view(torch.int32)


# ---- dmpnn_linear_wgrad --------------------------------------------------------------------------------------------------------------
@dataclasses.dataclass(frozen=True)
class W:
    id: str
    M: int
    N: int
    K1: int
    K2: int = 0
    bias: bool = True
    n_src: int = 0          # > 0: A1 has that many rows (< M: indices repeat) and is read through gather1
    ld: tuple = ()          # (ldz, lda1, lda2); (): dense
    off: int = 0            # element offset of gZ, A1, A2
    pipe: str = "f32"
    graded: bool = False


def _wcases():
    cs = []
    for name, s in (("one", (1, 1, 1, 0)), ("tiny-odd", (5, 7, 3, 2)), ("below-16-rows", (15, 6, 4, 0)), ("one-full-tile", (16, 64, 64, 0)),
                    ("tile+1-K63", (17, 65, 63, 0))):
        for bias in (True, False):
            cs.append(W(f"f32-{name}-{'bias' if bias else 'nobias'}", *s, bias=bias))
    cs += [W(f"f32-K63+ones-one-tile-{n}slabs", m, 64, 63) for m, n in ((448, 7), (512, 8), (576, 9))]
    cs += [W("f32-ones-own-ktile-K64", 100, 64, 64), W("f32-ones-own-ktile-K128", 100, 64, 128),
           W("f32-N129-K372", 130, 129, 372),
           W("f32-gather-full+partial-over-K1K2-seam", 257, 300, 72, 14, n_src=100),
           W("f32-K1K2-not-x4-scalar-loop", 200, 66, 6, 2),
           W("f32-vecZ-last-float4-partial", 130, 66, 64, 8, ld=(68, 64, 8)),
           W("f32-odd-ld", 130, 64, 64, 8, ld=(65, 67, 9)),
           W("f32-ptr+1float", 130, 64, 64, 8, ld=(68, 68, 12), off=1),
           W("f32-M1023-below-f16", 1023, 300, 300),
           W("f32-M1025-N-odd-stays", 1025, 301, 300),
           W("f32-M2048-K1-odd-stays", 2048, 64, 31),
           W("f16-M1024-first", 1024, 64, 64, pipe="f16"),
           W("f16-partial-chunk+block", 1025, 66, 34, pipe="f16"),
           W("f16-M1056-300x300", 1056, 300, 300, pipe="f16"),
           W("f16-gather-K1K2", 1100, 300, 72, 14, n_src=300, pipe="f16"),
           W("f16-M4097-N2-K2", 4097, 2, 2, pipe="f16"),
           W("f16-768chunks-target512", 24576, 64, 34, pipe="f16"),
           W("f16-769chunks-target768", 24608, 64, 34, pipe="f16"),
           W("f16-8B-aligned-ld-even-not-x4", 1100, 66, 34, 6, ld=(70, 38, 10), off=2, pipe="f16"),
           W("f32-graded", 512, 64, 64, graded=True), W("f16-graded", 2048, 64, 64, pipe="f16", graded=True)]
    assert len({c.id for c in cs}) == len(cs)
    return cs


WCASES = _wcases()


@functools.lru_cache(maxsize=None)
def _wref(case: W):
    """(inputs, float64 reference, float32 run, e32) of a case — computed once, shared, never written to."""
    inp = rh.wgrad_inputs(case.M, case.N, case.K1, case.K2, case.n_src or None, seed=len(case.id), graded=case.graded)
    r64, r32 = rh.wgrad_ref(inp), rh.wgrad_ref(inp, torch.float32)
    return inp, r64, r32, rh.yardstick(r64, r32)


def _run_w(dev, case: W, **kw):
    inp = _wref(case)[0]
    ld = dict(zip(("ldz", "lda1", "lda2"), case.ld))
    res = rh.run_wgrad(dev, inp, want_gb=case.bias, off=case.off, **ld, **kw)
    assert res["rc"] == 0, res["msg"]
    assert res["ws_tail_ok"], "linear_wgrad wrote behind the dmpnn_linear_wgrad_ws_bytes(...) bytes of its workspace"
    assert res["pipe"] == case.pipe, f"{case.id}: ran on {res['pipe']}, the case is about {case.pipe}"
    return res


@gpu
@pytest.mark.parametrize("case", WCASES, ids=lambda c: c.id)
def test_rows_linear_wgrad(case, gpu_device):
    """``dmpnn_linear_wgrad``: gW and gb against float64, every entry; which pipe ran is pinned by the case."""
    _, r64, r32, e32 = _wref(case)
    res = _run_w(gpu_device, case)
    got = dict(gW=res["oW"].read("gW"))
    if case.bias:
        got["gb"] = res["ob"].read("gb").view(-1)
    else:
        assert res["ob"].pristine(), "gb is NULL: nothing may be written"
    if case.graded:   # reported, not asserted: the documented contract is norm-wise (DESIGN.md section 3 holds the figures)
        rk, r3 = rh.row_errors(got["gW"], r64["gW"]), rh.row_errors(r32["gW"], r64["gW"])
        ratio = rk / r3.clamp(min=rh.EPS32)
        n = int(ratio.argmax())
        print(f"ROWSGRADED {case.id} worst-row-ratio={float(ratio[n]):.2f} at n={n} (scale 2^-{n % 16}) row-err={float(rk[n]):.3e} "
              f"fp32-row-err={float(r3[n]):.3e} worst-row-err={float(rk.max()):.3e} fp32-worst-row-err={float(r3.max()):.3e}")
    fails = rh.compare(case.id, got, r64, e32, "grad")
    assert not fails, f"{case.id}: " + "; ".join(fails)


@gpu
@pytest.mark.parametrize("which", ["f32-tile+1-K63-bias", "f16-partial-chunk+block"])
def test_rows_linear_wgrad_null_outputs(which, gpu_device):
    """A NULL gW or a NULL gb: the other output is what the full call gives, the NULL one's buffer stays untouched."""
    case = next(c for c in WCASES if c.id == which)
    _, r64, _, e32 = _wref(case)
    only_b = rh.run_wgrad(gpu_device, _wref(case)[0], want_gW=False)
    assert only_b["rc"] == 0 and only_b["ws_tail_ok"], only_b["msg"]
    assert only_b["oW"].pristine(), "gW is NULL: nothing may be written"
    only_w = _run_w(gpu_device, dataclasses.replace(case, bias=False))
    assert only_w["ob"].pristine(), "gb is NULL: nothing may be written"
    got = dict(gW=only_w["oW"].read("gW"), gb=only_b["ob"].read("gb").view(-1))
    fails = rh.compare(case.id + "-null", got, r64, e32, "grad")
    assert not fails, "; ".join(fails)


@gpu
def test_rows_linear_wgrad_no_rows_and_short_workspace(gpu_device):
    """``M == 0``: exact zeros.  A workspace one byte short: ``DMPNN_ENOSPC`` with a message, nothing written anywhere."""
    inp = rh.wgrad_inputs(0, 7, 5, 0)
    res = rh.run_wgrad(gpu_device, inp, ldgw=9)
    assert res["rc"] == 0 and res["pipe"] == "memset" and res["ws_tail_ok"], res
    assert bool((bits(res["oW"].read()) == 0).all()) and bool((bits(res["ob"].read()) == 0).all())
    for M in (130, 1100):   # (either pipe's size)
        inp = rh.wgrad_inputs(M, 66, 34, 0)
        res = rh.run_wgrad(gpu_device, inp, ws_short=1)
        assert res["rc"] == rh.ENOSPC and "workspace" in res["msg"], (res["rc"], res["msg"])
        assert res["oW"].pristine() and res["ob"].pristine() and res["ws_pristine"]
    assert int(rh._lib.load().dmpnn_linear_wgrad_ws_bytes(1100, 66, 34, 1)) >= int(rh._lib.load().dmpnn_linear_wgrad_ws_bytes(130, 66, 34, 1)) > 0


# ---- dmpnn_message_bwd / dmpnn_aggregate_bwd -------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _graph(name):
    if name == "degrees":
        return rh.degree_graph(DEGREES)
    if name == "chains33k":
        return rh.chain_graph(3000, 11)   # 33 000 atoms, 60 000 edges: beyond the 32 768 waves of the capped grid
    if name == "qm9x12":
        from chemprop_amd import synth

        return synth.random_batch(12, "qm9", seed=3)
    if name == "garbage":
        return Golden(os.path.join(GOLDEN_DIR, "garbage_h24.npz")).bmg()
    raise KeyError(name)


_PLANS = {}


def _plan(name, dev):
    if name not in _PLANS:
        _PLANS[name] = rh.make_plan(_graph(name), dev)
    return _PLANS[name]


@functools.lru_cache(maxsize=None)
def _edge_ref(name, h):
    bmg = _graph(name)
    gen = torch.Generator().manual_seed(50 + h)
    nE, nV = int(bmg.edge_index.shape[1]), int(bmg.V.shape[0])
    gM = torch.randn(nE, h, generator=gen) * (1 + torch.arange(h).float() / h)
    gMv = torch.randn(nV, h, generator=gen)
    r64, r32 = rh.message_bwd_ref(bmg, gM), rh.message_bwd_ref(bmg, gM, torch.float32)
    return gM, gMv, r64, rh.yardstick(dict(gH=r64), dict(gH=r32))


EDGE_CASES = [(f"h{h}", "degrees", h, {}) for h in (1, 3, 4, 7, 64, 260, 300)] + [
    ("h64-odd-ld-in", "degrees", 64, dict(ld_in=65, ld_out=64)),
    ("h64-odd-ld-out", "degrees", 64, dict(ld_in=64, ld_out=67)),
    ("h64-in+1float", "degrees", 64, dict(ld_in=68, ld_out=68, off_in=1)),
    ("h64-out+1float", "degrees", 64, dict(ld_in=68, ld_out=68, off_out=1)),
    ("h8-padded-vector", "degrees", 8, dict(ld_in=12, ld_out=16)),
    ("h4-33k-atoms-grid-cap", "chains33k", 4, {}),
]


@gpu
@pytest.mark.parametrize("cid,graph,h,layout", EDGE_CASES, ids=[c[0] for c in EDGE_CASES])
def test_rows_message_and_aggregate_bwd(cid, graph, h, layout, gpu_device):
    """``dmpnn_message_bwd`` against the float64 transpose of the oracle's ``message``; ``dmpnn_aggregate_bwd`` = ``gMv[dst]`` bit for bit."""
    bmg = _graph(graph)
    plan, _ = _plan(graph, gpu_device)
    gM, gMv, r64, e32 = _edge_ref(graph, h)
    rc, msg, out = rh.run_edge_bwd(gpu_device, plan, "message", gM, **layout)
    assert rc == 0, msg
    fails = rh.compare(f"message_bwd-{cid}", dict(gH=out.read("gH")), dict(gH=r64), e32, "grad")
    assert not fails, "; ".join(fails)
    rc, msg, out = rh.run_edge_bwd(gpu_device, plan, "aggregate", gMv, **layout)
    assert rc == 0, msg
    assert torch.equal(bits(out.read("gH")), bits(gMv[bmg.edge_index[1]])), "aggregate_bwd is a copy of gMv[dst]: bit for bit"


@gpu
def test_rows_message_bwd_poisons_an_asymmetric_plan(gpu_device):
    """The garbage golden's graph (not symmetric): every entry of ``dmpnn_message_bwd`` is NaN — the documented poison, a value —
    while ``dmpnn_aggregate_bwd`` on the same plan is still exact."""
    bmg = _graph("garbage")
    plan, arr = _plan("garbage", gpu_device)
    assert int(arr["hdr"][0]) & 1, "the garbage graph is expected to be flagged asymmetric"
    gen = torch.Generator().manual_seed(3)
    for h, layout in ((24, {}), (7, {}), (24, dict(ld_out=25))):
        gM, gMv = torch.randn(plan.n_edges, h, generator=gen), torch.randn(plan.n_atoms, h, generator=gen)
        rc, msg, out = rh.run_edge_bwd(gpu_device, plan, "message", gM, **layout)
        assert rc == 0, msg
        assert bool(torch.isnan(out.read("gH")).all())
        rc, msg, out = rh.run_edge_bwd(gpu_device, plan, "aggregate", gMv, **layout)
        assert rc == 0, msg
        assert torch.equal(bits(out.read("gH")), bits(gMv[bmg.edge_index[1]]))


# ---- dmpnn_gather_rows -----------------------------------------------------------------------------------------------------------------
N_SRC = 37
GATHER_LAYOUTS = [("d64-padded-vector", 64, 5, dict(ldx=68, ldo=72)), ("d64-odd-ldx", 64, 5, dict(ldx=65, ldo=64)),
                  ("d64-odd-ldo", 64, 5, dict(ldx=64, ldo=67)), ("d64-x+1float", 64, 5, dict(ldx=68, ldo=68, off_x=1)),
                  ("d64-out+1float", 64, 40000, dict(ldx=68, ldo=68, off_o=1))]
GATHER_CASES = [(f"d{d}-n{n}", d, n, {}) for d in (1, 3, 4, 64, 300) for n in (0, 1, 5, 40000)] + GATHER_LAYOUTS


@functools.lru_cache(maxsize=None)
def _gather_src(d):
    return torch.randn(N_SRC, d, generator=torch.Generator().manual_seed(d))


@gpu
@pytest.mark.parametrize("cid,d,n_out,layout", GATHER_CASES, ids=[c[0] for c in GATHER_CASES])
def test_rows_gather_rows(cid, d, n_out, layout, gpu_device):
    """``out[i] = X[idx[i]]`` bit for bit, repeated indices (37 source rows); 40 000 rows: beyond the capped grid."""
    X = _gather_src(d)
    idx = torch.randint(0, N_SRC, (n_out,), generator=torch.Generator().manual_seed(n_out + d))
    rc, msg, out = rh.run_gather(gpu_device, X, idx, **layout)
    assert rc == 0, msg
    assert torch.equal(bits(out.read("out")), bits(X[idx]))


@gpu
@pytest.mark.parametrize("d,layout", [(4, {}), (64, dict(ldx=68, ldo=72)), (3, {}), (64, dict(ldo=65))],
                         ids=["d4-vector", "d64-padded-vector", "d3-scalar", "d64-odd-ldo-scalar"])
def test_rows_gather_rows_index_out_of_range(d, layout, gpu_device):
    """Indices ``-1`` and ``n_src`` give rows that are entirely NaN; their neighbours stay exact."""
    X = _gather_src(d)
    idx = torch.tensor([0, -1, N_SRC - 1, N_SRC, 5, 5, -1, 36, 2 ** 31 - 1, -2 ** 31, 1])
    bad = (idx < 0) | (idx >= N_SRC)
    rc, msg, out = rh.run_gather(gpu_device, X, idx, **layout)
    assert rc == 0, msg
    got = out.read("out")
    assert bool(torch.isnan(got[bad]).all()), "a row of an index out of range is NaN in every column"
    assert torch.equal(bits(got[~bad]), bits(X[idx[~bad]]))


# ---- dmpnn_update_fwd ------------------------------------------------------------------------------------------------------------------
SUBSETS = [s for m in range(1, 8) for s in [tuple(k for i, k in enumerate(("H_out", "M_next", "Mv")) if m >> i & 1)]]


@functools.lru_cache(maxsize=None)
def _update_ref(graph, d_h, act, bias, perm_key):
    bmg = _graph(graph)
    perm = torch.tensor(perm_key)
    inp = rh.update_inputs(int(bmg.edge_index.shape[1]), d_h, bias, seed=d_h)
    r64, r32 = rh.update_ref(bmg, perm, inp, act), rh.update_ref(bmg, perm, inp, act, torch.float32)
    return inp, r64, rh.yardstick(r64, r32)


@gpu
@pytest.mark.parametrize("bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("act", rh.UPDATE_ACTS)
@pytest.mark.parametrize("d_h", [4, 64, 300, 320])
@pytest.mark.parametrize("graph", ["degrees", "qm9x12"])
def test_rows_update_fwd(graph, d_h, act, bias, gpu_device):
    """``dmpnn_update_fwd`` on CSR-row order against the float64 step of the oracle, for every non-empty subset of its three outputs:
    an absent output's buffer stays untouched, an output present in two subsets is bit-identical between them."""
    plan, arr = _plan(graph, gpu_device)
    assert torch.equal(arr["perm"], rh.csr_tables(_graph(graph))["perm"]), "the plan's CSR rows are the edges by destination, stable"
    inp, r64, e32 = _update_ref(graph, d_h, act, bias, tuple(arr["perm"].tolist()))
    first = {}
    for sub in SUBSETS:
        rc, msg, outs = rh.run_update(gpu_device, plan, inp, act, outputs=sub)
        assert rc == 0, msg
        got = {}
        for k, m in outs.items():
            if k not in sub:
                assert m.pristine(), f"{k} is NULL in {sub}: nothing may be written"
                continue
            got[k] = m.read(k)
            if k in first:
                assert torch.equal(bits(got[k]), first[k]), f"{k} differs between two subsets of the outputs ({sub})"
            else:
                first[k] = bits(got[k])
        fails = rh.compare(f"update_fwd-{graph}-h{d_h}-{act}-{'bias' if bias else 'nobias'}-{'+'.join(sub)}", got, r64, e32, "fwd")
        assert not fails, "; ".join(fails)


@gpu
def test_rows_update_fwd_without_edges(gpu_device):
    """``n_edges == 0``: ``Mv`` is exactly zero, the padding of its rows untouched."""
    bmg = rh.degree_graph((0, 0, 0))
    plan, _ = rh.make_plan(bmg, gpu_device)
    rc, msg, outs = rh.run_update(gpu_device, plan, rh.update_inputs(0, 8, True), "relu", ld=12)
    assert rc == 0, msg
    assert bool((bits(outs["Mv"].read("Mv")) == 0).all()) and outs["Mv"].rows == 3
    assert outs["H_out"].pristine() and outs["M_next"].pristine()


REJECTS = [("d_h6", 8, dict(d_h=6)), ("d_h324", 324, {}), ("ld-even-not-x4", 8, dict(ld=10)), ("ld-odd", 8, dict(ld=9)),
           ("ptr+2floats", 8, dict(ld=12, off=2))]
# one tensor alone outside the contract, the others dense and aligned (the contraction behind the call takes 8-byte rows of M)
REJECTS += [(f"only-{k}-{name}", 8, dict(only=(k,), **kw)) for k in ("M", "H0", "H_out", "M_next", "Mv")
            for name, kw in (("ld-even-not-x4", dict(ld=10)), ("ld-odd", dict(ld=9)), ("ptr+2floats", dict(ld=12, off=2)))]


@gpu
@pytest.mark.parametrize("cid,width,kw", REJECTS, ids=[c[0] for c in REJECTS])
def test_rows_update_fwd_rejects_undocumented_shapes(cid, width, kw, gpu_device):
    """Outside ``d_h % 4 == 0``, ``d_h <= 320``, 16-byte alignment, ``ld % 4 == 0``: ``DMPNN_EINVAL`` with a message, nothing written.
    Before ``dmpnn_update_fwd`` checked this itself, ``only-M-*`` and ``only-H0-*`` with ``ld-even-not-x4`` or ``ptr+2floats`` were
    accepted (the contraction behind it reads such rows in 8-byte pieces): those four cases failed then."""
    plan, _ = _plan("degrees", gpu_device)
    inp = rh.update_inputs(plan.n_edges, width, True)
    for sub in (("H_out", "M_next", "Mv"), ("Mv",), ("H_out",)):
        rc, msg, outs = rh.run_update(gpu_device, plan, inp, "relu", outputs=sub, **kw)
        if "only" in kw and kw["only"][0] in ("H_out", "M_next", "Mv") and kw["only"][0] not in sub:
            continue   # (that tensor is not part of this call)
        assert rc == rh.EINVAL and msg, (cid, sub, rc, msg)
        assert all(m.pristine() for m in outs.values()), "a refused call writes nothing"


# ---- the references, where no GPU is needed ------------------------------------------------------------------------------------------
def test_rows_harness_reference_on_cpu():
    """The message transpose is the adjoint of the oracle's ``message`` (``<gM, message(H)> == <message_bwd_ref(gM), H>`` to 1e-12 in
    float64); the graph builder makes symmetric graphs with the prescribed in-degrees; the CSR tables and the update reference agree
    with the oracle's own step."""
    from oracle import dmpnn_torch as ot

    g = _graph("degrees")
    deg = rh.in_degrees(g)
    assert set(deg.tolist()) == set(DEGREES), sorted(set(deg.tolist()))
    assert int((deg == 0).sum()) == 1 and int(g.batch[-1]) + 1 == len(DEGREES)
    big = _graph("chains33k")
    assert int(big.V.shape[0]) >= 33000 and set(rh.in_degrees(big).tolist()) == {1, 2}
    for bmg in (g, big, _graph("qm9x12")):
        src, dst = bmg.edge_index
        rev = bmg.rev_edge_index
        assert torch.equal(src[rev], dst) and torch.equal(dst[rev], src) and torch.equal(rev[rev], torch.arange(rev.numel()))
    for bmg, hs in ((g, (1, 4, 7)), (_graph("qm9x12"), (3,)), (rh.chain_graph(5, 4), (2,))):
        for h in hs:
            gap = rh.adjoint_gap(bmg, h)
            assert gap <= 1e-12, (h, gap)
    # the update reference in CSR-row order is the oracle's step in edge order, row i = edge perm[i]
    t = rh.csr_tables(g)
    assert torch.equal(g.edge_index[1][t["perm"]], torch.sort(g.edge_index[1]).values) and torch.equal(t["perm"][t["inv"]], torch.arange(t["perm"].numel()))
    inp = rh.update_inputs(int(g.edge_index.shape[1]), 4, True)
    r = rh.update_ref(g, t["perm"], inp, "tanh")
    w = ot.MPWeights(None, inp["W_h"].double(), None, None, b_h=inp["b_h"].double())
    H = ot.update(inp["M"].double()[t["inv"]], inp["H0"].double()[t["inv"]], w, torch.tanh)
    assert torch.equal(r["H_out"][t["inv"]], H) and torch.equal(r["Mv"], ot.segment_sum_dst(H, g.edge_index[1], int(g.V.shape[0])))
    # the wgrad reference against a loop-free restatement of its definition
    inp = rh.wgrad_inputs(9, 3, 2, 2, n_src=4)
    r = rh.wgrad_ref(inp)
    A = torch.cat((inp["A1"][inp["gather"].long()], inp["A2"]), 1).double()
    assert torch.allclose(r["gW"], torch.einsum("mn,mk->nk", inp["gZ"].double(), A), rtol=1e-14, atol=0) and r["gb"].shape == (3,)


def test_rows_yardsticks_under_the_caps_on_cpu():
    """The float32 yardstick of every listed case stays under the cap of its kind — ``MARGIN * e32`` is what decides, not the cap —
    and no reference tensor is identically zero."""
    for case in WCASES:
        _, r64, _, e32 = _wref(case)
        assert max(e32.values()) < rh.CAP["grad"], (case.id, e32)
        assert float(r64["gW"].abs().max()) > 0
        _wref.cache_clear()   # (the large cases are not kept for a run without GPU tests)
    for cid, graph, h, _ in EDGE_CASES:
        assert _edge_ref(graph, h)[3]["gH"] < rh.CAP["grad"], cid
    for graph in ("degrees", "qm9x12"):
        perm = tuple(rh.csr_tables(_graph(graph))["perm"].tolist())
        for d_h in (4, 64, 300, 320):
            for act in rh.UPDATE_ACTS:
                e32 = _update_ref(graph, d_h, act, True, perm)[2]
                assert max(e32.values()) < rh.CAP["fwd"], (graph, d_h, act, e32)
