"""The forward row kernels through the C ABI at the edges of their dispatch, against float64 on the CPU (``tests/rows_harness.py``):
``dmpnn_linear_fwd`` (every one of the 40 ``k_gemm<RT, WN, G, HAS_A2, EPI_PLAIN>`` builds), ``dmpnn_linear16_fwd`` (+ ``dmpnn_linear16_ok``,
``dmpnn_linear16_wsplit_bytes``; the 10 ``k_rows16<WN, GC>`` builds), ``dmpnn_message_fwd`` / ``dmpnn_aggregate_fwd`` (the four
``k_segment`` builds of either mode).

The shapes are the smallest that reach each branch; the id of a case names its edge and, for the build cases, the build the restated
dispatch rule (``rows_harness.linear_build`` / ``linear16_build``) says it runs — the ``*_on_cpu`` tests check that the tables reach
every build.  The vector builds of the fp32 kernel need ``N % 4 == 0`` (``vec_c``), so their shapes are the smallest ``(M, N)`` of each
``(RT, WN)`` with ``N`` rounded up to a multiple of 4 (the row counts stay); the ``G1`` builds run the odd widths themselves.

Arithmetic outputs are held as in ``tests/test_rows_boundaries.py``: ``err = max|got - ref| / max|ref|`` over every entry, unfloored,
within ``min(MARGIN max(e32, 2**-23), cap)`` with ``cap = 1e-5`` and ``e32`` the float32 run of the same restatement.  The segment
kernels add in increasing edge id, the reference's order: for none / ReLU / LeakyReLU / PReLU on load they are compared bit for bit with
the float32 run.  Where ``dmpnn_linear_fwd`` gives both outputs, ``C`` is ``(z > 0 ? z : slope z) + 0`` of the ``Zpre`` read back, bit
for bit, for the same four activations.  Outputs live in NaN-prefilled buffers whose padding and guard must come back untouched; the
padding columns of the inputs hold NaN.  Every GPU test carries ``pytest.mark.gpu`` itself.

MARGIN stays ``rows_harness.MARGIN`` = 16.  Measured on the MI355X with the report lines of every case (471 tensor comparisons): the
worst ``err / max(e32, 2**-23)`` is 2.74 — ``build-RT1-WN1-G1-M1-N1``, ONE output entry, err 3.3e-7 of a 0.09 pre-activation: the
fmaf chain of 35 products in the kernel's k order against float32's own draw of 1.3e-8 (below the ``2**-23`` floor of the ratio).  The
next are 2.39 (``Zpre`` of ``rescale-up-zero-down-GC4``, f16 pipe, four operand groups, max|ref| 792), 2.35 (``tail-K96-3chunks``, fp32
pipe), 2.15, 2.13 (``K2``, f16 pipe), 1.90 (``tail-K160-5chunks``); the segment kernels reproduce the float32 run (bit for bit
with the four exact activations; at most 1.09 with tanh / ELU on load).  2 x 2.74 = 5.5 <= 16.  The graded rows of one 48-row tile on the f16 pipe (rows scaled
by ``2**-(r % 16)``; reported, not asserted): worst ``row error / float32's row error`` 1.93 (row 42, scale
``2**-10``: 2.3e-7 against 1.1e-7; worst row error 2.9e-7, float32's 3.2e-7).
Wall time of the module's 273 GPU tests on the MI355X: 5.2 s (the slowest case 0.3 s).

One ``rocprofv3 --kernel-trace --stats`` run of the module lists all 40 ``k_gemm<RT, WN, G, HAS_A2, EPI_PLAIN>`` names, the 10
``k_rows16<WN, GC, false>`` names and ``k_segment<4, MODE, 0, NONE | RELU>``, ``k_segment<4, MODE, -1, -1>``, ``k_segment<1, MODE, -1, -1>``
for both modes.

What the sweep found: ``dmpnn_linear16_fwd`` with ``gather1_rows == 0`` (documented: unknown) built a ZERO-byte descriptor for ``A1``,
so every gathered row read zeros (``test_fwd_linear16[gather-rows-unknown]``: err 0.51); it now means what it means to
``dmpnn_linear_fwd``.  The contract fixes: see the argument-error tests and ``test_fwd_linear16_ok_table_on_cpu``.

Tried against deliberately wrong builds (scratch copies, never committed), each run once:
* the ``left == 3`` tail of ``k_gemm`` running the two-chunk tail fails ``test_fwd_linear_fp32[tail-K65-3chunks | tail-K96-3chunks |
  tail-K129-5chunks | tail-K160-5chunks | seam-in-quad-K70+14]`` (every case of 3 or 5 chunks);
* ``acc *= s / s_prev`` of ``k_rows16`` removed fails ``test_fwd_linear16[rescale-* (all four) | K386 | K770 | GC4-K130 |
  build-WN*-GC4-* (all five)]`` — every case with a second operand group of another scale;
* ``k2o`` of ``k_gemm``'s loader one element on fails 55 cases: every two-operand case of ``test_fwd_linear_fp32`` (all 28 such build
  cases) and ``test_fwd_linear_gather_index_beyond_gather1_rows[oob-G4 | oob-G2-padded-lda1 | oob-G1]``; ``k2o`` of ``k_rows16``'s
  loader fails ``test_fwd_linear16[seam-K70+14 | seam-K128+2 | gather-* | layout-operands+2floats | layout-padded-everything |
  build-WN*-GC4-*]`` and both f16 out-of-range cases;
* ``case 5:`` of ``k_segment`` running the in-degree-4 body fails ``test_fwd_message_and_aggregate`` on the 20 cases that run a hot
  vector build (``h4 .. h516`` with none / ReLU, ``h8-padded-vector``, the directed aggregate half of the undirected cases); the generic
  and scalar builds have no switch — they loop for every in-degree.
"""
import ctypes as C
import dataclasses
import functools

import pytest
import torch

import rows_harness as rh

MARGIN = rh.MARGIN
gpu = pytest.mark.gpu


def bits(t):
    return t.contiguous().view(torch.int32)


def lay(**kw):
    return tuple(sorted(kw.items()))


# ---- the cases of the two linear entries ---------------------------------------------------------------------------------------------
@dataclasses.dataclass(frozen=True)
class L:
    id: str
    M: int
    N: int
    K1: int
    K2: int = 0
    act: str = "relu"
    bias: bool = True
    cadd: bool = True
    want: tuple = ("C", "Zpre")
    n_src: int = 0            # > 0: A1 has that many rows and is read through gather1 (repeating indices)
    ld: tuple = ()            # lay(A1=..., C=...): leading dimensions, the others dense
    off: tuple = ()           # lay(...): element offsets, the others 0
    pipe: str = "f32"
    graded: object = None
    slope_ptr: bool = False
    gather_rows: int = -1     # what gather1_rows says (-1: the rows of A1; 0: unknown)
    build: tuple = None       # the build the dispatch rule gives (the build cases)


# the smallest (M, N) of every (RT, WN) of launch_linear_ex (restated rule; checked by test_fwd_case_tables_reach_every_build_on_cpu)
BUILD_SHAPES = {(1, 1): (1, 1), (1, 2): (2049, 65), (1, 4): (2049, 193), (1, 5): (1633, 257),
                (2, 1): (1361, 129), (2, 2): (4097, 65), (2, 4): (4097, 193), (2, 5): (4097, 257),
                (3, 1): (2721, 129), (3, 2): (8193, 65), (3, 4): (8193, 193), (3, 5): (8193, 257)}
VARIANTS = {"G4": (36, 0), "G4+A2": (32, 8), "G2": (34, 6), "G1": (33, 2)}   # (K1, K2)
# (tanh runs at the small shapes only: over thousands of rows the float32 yardstick of a saturating activation — pre-activations of
#  magnitude 6 behind outputs below 1 — reaches 1e-6 of max|ref|, and 16 times that would be decided by the cap, not the yardstick)
BUILD_ACTS = ("none", "relu", "leakyrelu", "prelu", "elu")
ALL_F32_BUILDS = {(rt, wn, v) for rt in (1, 2, 3) for wn in (1, 2, 4, 5) for v in VARIANTS if rt != 2 or v.startswith("G4")}
ALL_F16_BUILDS = {(wn, gc) for wn in (1, 2, 3, 4, 5) for gc in (12, 4)}


def _f32_build_cases():
    cs, i = [], 0
    for (rt, wn), (M, N) in BUILD_SHAPES.items():
        for v, (K1, K2) in VARIANTS.items():
            if rt == 2 and not v.startswith("G4"):
                continue   # (with G2 / G1 these shapes fall to RT = 3: the RT = 3 row runs them)
            n = N if v == "G1" else (N + 3) // 4 * 4
            cs.append(L(f"build-RT{rt}-WN{wn}-{v}-M{M}-N{n}", M, n, K1, K2, act=BUILD_ACTS[i % 5], bias=i % 2 == 0, cadd=i % 3 != 0,
                        n_src=500 if (v == "G4+A2" and rt == 3) or (v == "G1" and rt == 1) else 0, build=(rt, wn, v)))
            i += 1
    return cs


def _f32_cases():
    cs = _f32_build_cases()
    for M in (1, 15, 16, 17, 33):
        cs += [L(f"rows-M{M}-G4", M, 12, 8), L(f"rows-M{M}-G1", M, 7, 5, 3)]
    cs += [L(f"cols-N{N}", 5, N, 36) for N in (1, 3, 4, 63, 64, 65, 300, 320, 321)]     # N = 300, 5 rows: WN = 1, five column blocks
    cs += [L(f"tail-K{K}-{-(-K // 32)}chunks", 17, 20, K) for K in (1, 31, 32, 33, 64, 65, 96, 97, 128, 129, 160, 161, 192)]
    cs += [L("seam-on-chunk-K32+8", 17, 20, 32, 8), L("seam-on-quad-K36+8", 17, 20, 36, 8), L("seam-in-quad-K3+2", 17, 20, 3, 2),
           L("seam-in-quad-K70+14", 17, 20, 70, 14), L("seam-K1-0-operand-in-A2", 17, 20, 0, 36),
           L("gather-repeating-G4", 40, 20, 32, 8, n_src=9), L("gather-repeating-G1", 40, 7, 33, 3, n_src=9),
           L("gather-rows-unknown", 40, 20, 32, 8, n_src=9, gather_rows=0),
           L("gather-padded-lda1-G2", 40, 20, 34, 6, n_src=9, ld=lay(A1=38))]
    for act in rh.LINEAR_ACTS:
        cs += [L(f"act-{act}-slope-by-pointer", 17, 20, 36, act=act, slope_ptr=True)]
        if act != "prelu":
            cs += [L(f"act-{act}-slope-by-value", 17, 20, 36, act=act)]
    cs += [L("act-tanh-G1", 17, 7, 5, 3, act="tanh"), L("act-elu-G1", 17, 7, 5, 3, act="elu"), L("act-prelu-G1", 17, 7, 5, 3, act="prelu"),
           L("act-leakyrelu-G2", 17, 20, 34, 6, act="leakyrelu")]
    cs += [L(f"epi-{'bias' if b else 'nobias'}-{'cadd' if c else 'nocadd'}", 17, 20, 36, bias=b, cadd=c) for b in (True, False) for c in (True, False)]
    for name, kw in (("G4", dict(N=20, K1=36)), ("G1", dict(N=7, K1=5, K2=3))):
        cs += [L(f"want-C-only-{name}", 17, want=("C",), **kw), L(f"want-Zpre-only-{name}", 17, want=("Zpre",), **kw)]
    cs += [L("layout-odd-ldc-G1", 33, 20, 36, ld=lay(C=21)), L("layout-odd-ldz-G1", 33, 20, 36, ld=lay(Zpre=23)),
           L("layout-C+1float-G1", 33, 20, 36, ld=lay(C=24), off=lay(C=1)),
           L("layout-all+2floats-G2", 33, 20, 36, 8, ld=lay(A1=38, A2=10, W=46, Cadd=22, C=24, Zpre=24), off=lay(A1=2, A2=2, W=2, Cadd=2)),
           L("layout-W+2floats-G2", 33, 20, 36, 8, off=lay(W=2)), L("layout-Cadd+1float-G1", 33, 20, 36, 8, ld=lay(Cadd=21), off=lay(Cadd=1)),
           L("layout-padded-everything-G4", 33, 20, 36, 8, ld=lay(A1=40, A2=12, W=48, Cadd=24, C=28, Zpre=32)),
           L("layout-padded-everything-two-blocks", 70, 132, 36, 8, ld=lay(A1=40, A2=12, W=48, Cadd=136, C=140, Zpre=144))]
    assert len({c.id for c in cs}) == len(cs)
    return cs


def _f16_cases():
    f = functools.partial(L, pipe="f16")
    cs = [f(f"build-WN{wn}-GC12-N{N}", 50, N, 34, build=(wn, 12)) for wn, N in ((1, 2), (2, 66), (3, 130), (4, 194), (5, 258))]
    cs += [f(f"build-WN{wn}-GC4-M{M}-N{N}-two-groups", M, N, 128, 2, act=act, build=(wn, 4))
           for wn, M, N, act in ((1, 24577, 2, "relu"), (2, 24577, 66, "prelu"), (3, 12289, 322, "leakyrelu"), (4, 24577, 194, "none"), (5, 24577, 258, "elu"))]
    cs += [f(f"rows-M{M}", M, 16, 32) for M in (1, 47, 48, 49)]
    cs += [f(f"cols-N{N}", 49, N, 34) for N in (1, 7, 16, 17, 300, 320, 322, 512, 641)]   # 1, 7, 17, 322 / 2 odd ...: scalar epilogue
    cs += [f(f"K{K}", 49, 20, K) for K in (2, 30, 32, 34, 64, 66, 128, 130, 384, 386, 770)]
    cs += [f(f"GC4-K{K}", 24577, 2, K, build=(1, 4)) for K in (128, 130)]
    g12, g4 = ("groups", 384), ("groups", 128)
    cs += [f("rescale-up-down-GC12", 49, 20, 770, graded=g12 + ((0, 8, -8),)), f("rescale-down-up-GC12", 49, 20, 770, graded=g12 + ((0, -8, 8),)),
           f("rescale-zero-group-between-GC12", 49, 20, 770, graded=g12 + ((0, None, 0),)),
           f("rescale-up-zero-down-GC4", 24577, 2, 386, graded=g4 + ((0, 8, None, -8),), build=(1, 4))]
    cs += [f("seam-K70+14", 49, 20, 70, 14), f("seam-K128+2", 49, 20, 128, 2), f("seam-K1-0-operand-in-A2", 49, 20, 0, 34),
           f("gather-repeating", 100, 20, 70, 14, n_src=9), f("gather-rows-unknown", 100, 20, 70, 14, n_src=9, gather_rows=0),
           f("gather-padded-lda1", 100, 20, 70, 14, n_src=9, ld=lay(A1=74))]
    for act in rh.LINEAR_ACTS:
        cs += [f(f"act-{act}-vector", 49, 20, 34, act=act, slope_ptr=act == "leakyrelu"), f(f"act-{act}-scalar", 49, 7, 34, act=act)]
    cs += [f(f"epi-{'bias' if b else 'nobias'}-{'cadd' if c else 'nocadd'}", 49, 20, 34, bias=b, cadd=c) for b in (True, False) for c in (True, False) if not (b and c)]
    cs += [f("want-C-only", 49, 20, 34, want=("C",)), f("want-Zpre-only", 49, 20, 34, want=("Zpre",)), f("want-Zpre-only-scalar", 49, 7, 34, want=("Zpre",)),
           f("layout-odd-ldc-scalar", 49, 20, 34, ld=lay(C=21)), f("layout-Cadd+2floats-scalar", 49, 20, 34, ld=lay(Cadd=22), off=lay(Cadd=2)),
           f("layout-operands+2floats", 49, 20, 70, 14, ld=lay(A1=74, A2=18), off=lay(A1=2, A2=2)),
           f("layout-padded-everything", 49, 20, 70, 14, ld=lay(A1=72, A2=16, W=88, Cadd=24, C=28, Zpre=32)),
           f("graded-rows", 48, 64, 64, graded="rows", bias=False, cadd=False, act="none")]
    assert len({c.id for c in cs}) == len(cs)
    return cs


F32_CASES, F16_CASES = _f32_cases(), _f16_cases()


@functools.lru_cache(maxsize=6)
def _lin(M, N, K1, K2, n_src, graded, bias, cadd, act):
    """(inputs, float64 reference, float32 run, e32) — computed once per distinct problem, shared, never written to."""
    inp = rh.linear_inputs(M, N, K1, K2, n_src or None, seed=(M * 7 + N * 3 + K1 * 5 + K2) % 1000, graded=graded, bias=bias, cadd=cadd)
    r64, r32 = rh.linear_ref(inp, act), rh.linear_ref(inp, act, torch.float32)
    return inp, r64, r32, rh.yardstick(r64, r32)


def _lref(c: L):
    return _lin(c.M, c.N, c.K1, c.K2, c.n_src, c.graded, c.bias, c.cadd, c.act)


def _label(c: L):
    if c.pipe == "f16":
        return rh.linear16_build(c.M, c.N)
    shape = dict(M=c.M, N=c.N, K1=c.K1, K2=c.K2, Cadd=True if c.cadd else None)
    return rh.linear_build(c.M, c.N, *rh.linear_g(shape, dict(c.ld), dict(c.off), c.want))


def _run(dev, c: L, inp=None, **kw):
    inp = _lref(c)[0] if inp is None else inp
    res = rh.run_linear(dev, inp, c.act, c.pipe, c.want, dict(c.ld), dict(c.off), slope_ptr=c.slope_ptr,
                        gather_rows=None if c.gather_rows < 0 else c.gather_rows, **kw)
    assert res["rc"] == 0, (c.id, res["msg"])
    assert res["ws_tail_ok"], "dmpnn_linear16_fwd wrote behind the dmpnn_linear16_wsplit_bytes(...) bytes of wsplit"
    return res


def _outputs(c: L, res):
    got = {}
    for k, m in res["outs"].items():
        if k in c.want:
            got[k] = m.read(f"{c.id} {k}")
        else:
            assert m.pristine(), f"{c.id}: {k} is NULL, nothing may be written"
    return got


def _check_epilogue(c: L, got):
    """``C`` from the ``Zpre`` read back: the one branch-free formula of the fp32 kernel's epilogue, in float32 on the CPU."""
    if c.act not in rh.SIMPLE_ACTS or set(c.want) != {"C", "Zpre"}:
        return
    z = got["Zpre"]
    y = torch.where(z > 0, z, torch.tensor(rh.act_slope(c.act), dtype=torch.float32) * z) + 0.0
    assert torch.equal(bits(got["C"]), bits(y)), f"{c.id}: C is not (z > 0 ? z : slope z) + 0 of the Zpre the same call stored"
    if c.act == "relu":
        assert not bool((bits(got["C"]) == -2 ** 31).any()), f"{c.id}: a ReLU zero must be +0"


@gpu
@pytest.mark.parametrize("case", F32_CASES, ids=lambda c: c.id)
def test_fwd_linear_fp32(case, gpu_device):
    """``dmpnn_linear_fwd``: ``C`` and ``Zpre`` against float64, every entry; one launch; the epilogue's consistency."""
    _, r64, _, e32 = _lref(case)
    res = _run(gpu_device, case)
    assert res["launches"] == 1, res["launches"]
    print(f"FWDBUILD {case.id} k_gemm{_label(case)}")
    got = _outputs(case, res)
    fails = rh.compare("linear-" + case.id, got, r64, e32, "fwd", MARGIN)
    assert not fails, f"{case.id}: " + "; ".join(fails)
    _check_epilogue(case, got)


@gpu
@pytest.mark.parametrize("case", F16_CASES, ids=lambda c: c.id)
def test_fwd_linear16(case, gpu_device):
    """``dmpnn_linear16_fwd`` (weight split + contraction: two launches) against float64, every entry; ``dmpnn_linear16_ok`` said yes."""
    _, r64, r32, e32 = _lref(case)
    res = _run(gpu_device, case)
    assert res["launches"] == 2, res["launches"]
    print(f"FWDBUILD {case.id} k_rows16{_label(case)}")
    got = _outputs(case, res)
    if case.graded == "rows":   # reported, not asserted: the tile-wide scale is a documented property
        rk, r3 = rh.row_errors(got["C"], r64["C"]), rh.row_errors(r32["C"], r64["C"])
        ratio = rk / r3.clamp(min=rh.EPS32)
        n = int(ratio.argmax())
        print(f"FWDGRADED {case.id} worst-row-ratio={float(ratio[n]):.2f} at r={n} (scale 2^-{n % 16}) row-err={float(rk[n]):.3e} "
              f"fp32-row-err={float(r3[n]):.3e} worst-row-err={float(rk.max()):.3e} fp32-worst-row-err={float(r3.max()):.3e}")
    fails = rh.compare("linear16-" + case.id, got, r64, e32, "fwd", MARGIN)
    assert not fails, f"{case.id}: " + "; ".join(fails)


OOB = [L("oob-G4", 40, 20, 32, 8, n_src=9), L("oob-G2-padded-lda1", 40, 20, 34, 6, n_src=9, ld=lay(A1=38)), L("oob-G1", 40, 7, 33, 3, n_src=9),
       L("oob-f16", 100, 20, 70, 14, n_src=9, pipe="f16"), L("oob-f16-padded-lda1", 100, 20, 70, 14, n_src=9, ld=lay(A1=74), pipe="f16")]


@gpu
@pytest.mark.parametrize("case", OOB, ids=lambda c: c.id)
def test_fwd_linear_gather_index_beyond_gather1_rows(case, gpu_device):
    """``include/dmpnn.h``: a gather index ``>= gather1_rows`` reads a row of zeros.  Indices ``gather1_rows`` and ``gather1_rows + 1``,
    with NaN rows stored right behind the source rows: the output rows are those of a zero ``A1`` row (finite), the others unchanged."""
    inp = dict(_lref(case)[0])
    g = inp["gather"].clone()
    g[::7] = case.n_src
    inp["gather"] = g
    r64, r32 = rh.linear_ref(inp, case.act), rh.linear_ref(inp, case.act, torch.float32)
    g2 = g.clone()
    g2[::14] = case.n_src + 1      # (the same zero row: the reference maps every such index to it)
    res = _run(gpu_device, case, inp=dict(inp, gather=g2), a1_tail=3)
    fails = rh.compare("linear-" + case.id, _outputs(case, res), r64, rh.yardstick(r64, r32), "fwd", MARGIN)
    assert not fails, f"{case.id}: " + "; ".join(fails)


@gpu
def test_fwd_linear16_wsplit_ready(gpu_device):
    """A second call with ``wsplit_ready = 1`` on the same workspace and a ``W`` buffer full of NaN: one launch, the same bits."""
    for case in (next(c for c in F16_CASES if c.id == i) for i in ("seam-K70+14", "cols-N322", "K770")):
        inp = _lref(case)[0]
        a = _run(gpu_device, case)
        b = _run(gpu_device, case, inp=dict(inp, W=torch.full_like(inp["W"], float("nan"))), ws=a["ws"], wsplit_ready=1)
        assert a["launches"] == 2 and b["launches"] == 1
        for k in case.want:
            assert torch.equal(bits(a["outs"][k].read()), bits(b["outs"][k].read())), (case.id, k)
        nb = int(rh._lib.load().dmpnn_linear16_wsplit_bytes(case.N, case.K1 + case.K2))
        assert nb == a["ws_bytes"] and nb % 256 == 0 and nb >= -(-case.N // 16) * -(-(case.K1 + case.K2) // 32) * 2048 + 4 * case.N


# ---- argument errors -----------------------------------------------------------------------------------------------------------------
ERR_SHAPE = dict(M=17, N=20, K1=36, K2=8)
ERRORS = [(f"{f}-below-width", dict(override={f: w - 4})) for f, w in (("lda1", 36), ("lda2", 8), ("ldw", 44), ("ldcadd", 20), ("ldc", 20), ("ldz", 20))]
ERRORS += [("lda1-zero", dict(override=dict(lda1=0))), ("no-output", dict(want=())), ("empty-contraction", dict(override=dict(K1=0, K2=0))),
           ("null-W", dict(override=dict(W=None)))]
ERRORS_F32 = ERRORS + [("null-A1", dict(override=dict(A1=None))), ("null-A2", dict(override=dict(A2=None))),
                       ("prelu-without-pointer", dict(override=dict(act=rh._lib.ACT["prelu"], act_slope_ptr=None)))]
ERRORS_F16 = ERRORS + [("wsplit-one-byte-short", dict(ws_short=1)), ("odd-K1-refused-by-linear16_ok", dict(shape=dict(M=17, N=20, K1=35, K2=9))),
                       ("A1+1float-refused-by-linear16_ok", dict(off=dict(A1=1), ld=dict(A1=38))),
                       ("gather-without-A1", dict(shape=dict(M=17, N=20, K1=0, K2=36), override=dict(gather1=1 << 20)))]


def _refused(dev, pipe, kw):
    kw = dict(kw)
    inp = rh.linear_inputs(**kw.pop("shape", ERR_SHAPE))
    res = rh.run_linear(dev, inp, "relu", pipe, **{"want": ("C", "Zpre"), **kw})
    assert res["rc"] == rh.EINVAL and res["msg"], (res["rc"], res["msg"])
    assert all(m.pristine() for m in res["outs"].values()), "a refused call writes no output"
    assert res["ws_tail_ok"] and res["ws_pristine"], "a refused call leaves wsplit as it was"


@gpu
@pytest.mark.parametrize("cid,kw", ERRORS_F32, ids=[e[0] for e in ERRORS_F32])
def test_fwd_linear_fp32_argument_errors(cid, kw, gpu_device):
    """``DMPNN_EINVAL`` with a message, nothing written.  The ``*-below-width`` and ``lda1-zero`` cases were accepted (and run with
    overlapping rows) before ``dmpnn_linear_fwd`` checked its leading dimensions."""
    _refused(gpu_device, "f32", kw)


@gpu
@pytest.mark.parametrize("cid,kw", ERRORS_F16, ids=[e[0] for e in ERRORS_F16])
def test_fwd_linear16_argument_errors(cid, kw, gpu_device):
    """The same for ``dmpnn_linear16_fwd``, ``wsplit`` included: before the entry decided everything ahead of the weight split, a shape
    ``dmpnn_linear16_ok`` refuses was answered ``DMPNN_EINVAL`` AFTER ``k_split_weights`` had written ``wsplit``; ``no-output`` and
    the leading dimensions were accepted."""
    _refused(gpu_device, "f16", kw)


@gpu
@pytest.mark.parametrize("which", ["A1", "A2", "A2-with-K1-0"])
def test_fwd_linear16_null_operand(which, gpu_device):
    """A NULL operand with a live width: ``DMPNN_EINVAL`` before any launch (``dmpnn_linear_fwd`` always refused it; the f16 entry
    used to build a descriptor on the null base — see ``test_fwd_linear16_ok_table_on_cpu`` for the host side of the same rule)."""
    kw = dict(override={which[:2]: None})
    if which == "A2-with-K1-0":
        kw["shape"] = dict(M=17, N=20, K1=0, K2=36)
    _refused(gpu_device, "f16", kw)


@gpu
@pytest.mark.parametrize("pipe", ["f32", "f16"])
def test_fwd_linear_without_rows(pipe, gpu_device):
    """``M == 0``: ``DMPNN_OK``, no output written, nothing behind ``wsplit``."""
    res = rh.run_linear(gpu_device, rh.linear_inputs(**ERR_SHAPE), "relu", pipe, override=dict(M=0))
    assert res["rc"] == 0 and res["ws_tail_ok"], res["msg"]
    assert all(m.pristine() for m in res["outs"].values())


def _ok_args(**kw):
    """``dmpnn_gemm_args`` of a call ``dmpnn_linear16_ok`` takes (host side only: the addresses are never read)."""
    g = rh._lib.GemmArgs()
    g.M, g.N, g.K1, g.K2 = 100, 20, 70, 14
    g.A1, g.lda1, g.A2, g.lda2, g.W, g.ldw, g.C, g.ldc = 1 << 20, 70, 2 << 20, 14, 3 << 20, 84, 4 << 20, 20
    for k, v in kw.items():
        setattr(g, k, v)
    return g


OK_TABLE = [("baseline", {}, 1), ("8B-aligned-operands", dict(A1=(1 << 20) + 8, A2=(2 << 20) + 8), 1), ("K2-0", dict(K2=0, A2=None, lda2=0), 1),
            ("K1-0-operand-in-A2", dict(K1=0, A1=None, lda1=0), 1), ("gathered", dict(gather1=5 << 20, gather1_rows=1000), 1),
            ("gathered-rows-unknown", dict(gather1=5 << 20, gather1_rows=0), 1),
            ("odd-K1", dict(K1=71, lda1=72), 0), ("odd-K2", dict(K2=13), 0), ("odd-lda1", dict(lda1=71), 0), ("odd-lda2", dict(lda2=15), 0),
            ("A1+1float", dict(A1=(1 << 20) + 4), 0), ("A2+1float", dict(A2=(2 << 20) + 4), 0),
            ("K1-0-odd-K2", dict(K1=0, A1=None, K2=13), 0), ("K1-0-A2+1float", dict(K1=0, A1=None, A2=(2 << 20) + 4), 0),
            ("gathered-source-2GiB", dict(gather1=5 << 20, gather1_rows=(1 << 31) // (4 * 70) + 1), 0),
            ("gathered-source-below-2GiB", dict(gather1=5 << 20, gather1_rows=(1 << 31) // (4 * 70) - 1), 1),
            ("no-rows", dict(M=0), 0), ("no-columns", dict(N=0), 0), ("empty-contraction", dict(K1=0, K2=0), 0),
            ("null-A1", dict(A1=None), 0), ("null-A2", dict(A2=None), 0), ("K1-0-null-A2", dict(K1=0, A1=None, A2=None), 0)]


@pytest.mark.parametrize("cid,kw,want", OK_TABLE, ids=[t[0] for t in OK_TABLE])
def test_fwd_linear16_ok_table_on_cpu(cid, kw, want):
    """``dmpnn_linear16_ok`` is a host-side rule.  ``null-A1``, ``null-A2`` and ``K1-0-null-A2`` were answered 1 before it looked at the
    pointers of a live width (``dmpnn_linear_fwd`` refuses the same call)."""
    lib = rh._lib.load()
    assert int(lib.dmpnn_linear16_ok(C.byref(_ok_args(**kw)))) == want
    assert int(lib.dmpnn_linear16_ok(None)) == 0


# ---- dmpnn_message_fwd / dmpnn_aggregate_fwd -------------------------------------------------------------------------------------------
DEGREES = (0, 1, 2, 3, 4, 5, 6, 7, 12)   # the straight-line bodies 1..6, the loop (7, 12), no incoming edge
WIDTHS = (1, 3, 4, 64, 129, 252, 256, 260, 300, 512, 516)   # 516: second 128-lane pass of the vector build; 129: of the scalar build


@functools.lru_cache(maxsize=None)
def _graph(name):
    if name == "degrees":
        return rh.degree_graph(DEGREES)
    if name == "isolated+bonds+chains33k":
        # 33 000 atoms — isolated atoms, single bonds and, so that the message is not identically zero, chains of three: beyond
        # the 32 768 waves of the capped grid
        return rh.degree_graph((0, 1, 2) * 5500)
    if name == "no-edges":
        return rh.degree_graph((0, 0, 0))
    raise KeyError(name)


_PLANS = {}


def _plan(name, dev):
    if name not in _PLANS:
        _PLANS[name] = rh.make_plan(_graph(name), dev)[0]
    return _PLANS[name]


@dataclasses.dataclass(frozen=True)
class S:
    id: str
    h: int
    act: str = "none"
    by_ptr: bool = False
    undirected: bool = False
    layout: tuple = ()
    graph: str = "degrees"
    build: str = "vec"        # vec-none / vec-relu (the hot builds), vec-generic, scalar


def _scases():
    cs = []
    for h in WIDTHS:
        v = h % 4 == 0
        cs += [S(f"h{h}-none", h, build="vec-none" if v else "scalar"), S(f"h{h}-relu", h, "relu", build="vec-relu" if v else "scalar")]
    cs += [S("h516-tanh-generic", 516, "tanh", build="vec-generic"), S("h260-undirected-generic", 260, undirected=True, build="vec-generic")]
    for h, b in ((64, "vec-generic"), (3, "scalar")):
        for act in rh.LINEAR_ACTS[2:]:
            cs += [S(f"h{h}-{act}-slope-by-pointer", h, act, True, build=b)]
            if act != "prelu":
                cs += [S(f"h{h}-{act}-slope-by-value", h, act, build=b)]
        cs += [S(f"h{h}-relu-slope-by-pointer", h, "relu", True, build="vec-relu" if h == 64 else b),
               S(f"h{h}-{'relu'}-undirected", h, "relu", undirected=True, build=b), S(f"h{h}-elu-undirected", h, "elu", undirected=True, build=b)]
    cs += [S("h64-odd-ld-in-scalar", 64, "relu", layout=lay(ld_in=65, ld_out=64), build="scalar"),
           S("h64-even-ld-out-scalar", 64, layout=lay(ld_in=64, ld_out=66), build="scalar"),
           S("h64-in+1float-scalar", 64, "relu", layout=lay(ld_in=68, ld_out=68, off_in=1), build="scalar"),
           S("h64-out+2floats-scalar", 64, layout=lay(ld_in=68, ld_out=68, off_out=2), build="scalar"),
           S("h256-in+2floats-scalar-two-passes", 256, "leakyrelu", layout=lay(ld_in=260, ld_out=260, off_in=2), build="scalar"),
           S("h8-padded-vector", 8, "relu", layout=lay(ld_in=12, ld_out=16), build="vec-relu"),
           S("h4-33k-atoms-grid-stride", 4, "relu", graph="isolated+bonds+chains33k", build="vec-relu"),
           S("h3-33k-atoms-grid-stride-scalar", 3, graph="isolated+bonds+chains33k", build="scalar"),
           S("h4-33k-atoms-grid-stride-generic", 4, "tanh", graph="isolated+bonds+chains33k", build="vec-generic")]
    assert len({c.id for c in cs}) == len(cs)
    return cs


SCASES = _scases()


@functools.lru_cache(maxsize=None)
def _hin(graph, h):
    nE = int(_graph(graph).edge_index.shape[1])
    return torch.randn(nE, h, generator=torch.Generator().manual_seed(70 + h)) * (1 + torch.arange(h).float() / h)


@functools.lru_cache(maxsize=8)
def _sref(graph, h, which, act, undirected):
    bmg, Hin = _graph(graph), _hin(graph, h)
    r64, r32 = rh.segment_fwd_ref(bmg, Hin, which, act, undirected), rh.segment_fwd_ref(bmg, Hin, which, act, undirected, torch.float32)
    return r64, r32, rh.yardstick(dict(out=r64), dict(out=r32))


@gpu
@pytest.mark.parametrize("case", SCASES, ids=lambda c: c.id)
def test_fwd_message_and_aggregate(case, gpu_device):
    """Both segment entries on the same input: against float64 for every activation on load; bit for bit against the float32 run of the
    restatement where tau is exact (none, ReLU, LeakyReLU, PReLU) — the rows of an atom are added in increasing edge id.  The row of
    an atom without incoming edges is zero in ``Mv``."""
    plan, Hin = _plan(case.graph, gpu_device), _hin(case.graph, case.h)
    slope = rh.act_slope(case.act) or 0.0
    kw = dict(act=case.act, slope=rh.DECOY_SLOPE if case.by_ptr else slope, slope_ptr=slope if (case.by_ptr or case.act == "prelu") else None,
              **dict(case.layout))
    for which in ("message", "aggregate"):
        undirected = case.undirected and which == "message"
        r64, r32, e32 = _sref(case.graph, case.h, which, case.act, undirected)
        rc, msg, out = rh.run_segment_fwd(gpu_device, plan, which, Hin, undirected=undirected, **kw)
        assert rc == 0, msg
        got = out.read(f"{case.id} {which}")
        fails = rh.compare(f"{which}_fwd-{case.id}", dict(out=got), dict(out=r64), e32, "fwd", MARGIN)
        assert not fails, f"{case.id} {which}: " + "; ".join(fails)
        if case.act in rh.SIMPLE_ACTS:
            same = bits(got) == bits(r32)
            assert bool(same.all()), f"{case.id} {which}: {int((~same).sum())} entries differ from the float32 run of the same sums"


@gpu
def test_fwd_message_and_aggregate_without_edges(gpu_device):
    """``n_edges == 0`` with atoms: ``dmpnn_aggregate_fwd`` writes zero rows (their padding untouched), ``dmpnn_message_fwd`` nothing."""
    plan = _plan("no-edges", gpu_device)
    for h, layout in ((4, {}), (3, {}), (8, dict(ld_out=12))):
        Hin = torch.zeros(0, h)
        rc, msg, out = rh.run_segment_fwd(gpu_device, plan, "aggregate", Hin, "relu", **layout)
        assert rc == 0 and out.rows == 3, msg
        assert bool((bits(out.read("Mv")) == 0).all())
        rc, msg, out = rh.run_segment_fwd(gpu_device, plan, "message", Hin, "relu", **layout)
        assert rc == 0 and out.pristine(), msg


# ---- the tables and the references, where no GPU is needed ---------------------------------------------------------------------------
def test_fwd_case_tables_reach_every_build_on_cpu():
    """Under the restated dispatch rules the case tables reach all 40 ``k_gemm<.., EPI_PLAIN>`` builds and all 10 ``k_rows16`` builds,
    every build case runs the build its id names, the issue's shapes are the smallest of their ``(RT, WN)``, and the graphs have the
    in-degrees the segment kernels switch on."""
    for c in F32_CASES + F16_CASES:
        if c.build is not None:
            assert _label(c) == c.build, (c.id, _label(c))
    assert {_label(c) for c in F32_CASES} == ALL_F32_BUILDS and len(ALL_F32_BUILDS) == 40
    assert {_label(c) for c in F16_CASES} == ALL_F16_BUILDS and len(ALL_F16_BUILDS) == 10
    assert {c.build for c in F32_CASES if c.build} == ALL_F32_BUILDS and {c.build for c in F16_CASES if c.build} == ALL_F16_BUILDS
    for (rt, wn), (M, N) in BUILD_SHAPES.items():
        assert rh.linear_build(M, N, 4, False)[:2] == (rt, wn)
        if M > 1:
            assert rh.linear_build(M - 1, N, 4, False)[:2] != (rt, wn), "one row less runs another build"
        if rt == 2:
            assert rh.linear_build(M, N, 2, True)[0] == rh.linear_build(M, N, 1, True)[0] == 3
    assert rh.linear_build(5, 300, 4, False)[:2] == (1, 1), "few rows of 300 columns: the short-matrix redirect to WN = 1"
    assert rh.linear16_build(24576, 2) == (1, 12) and rh.linear16_build(24577, 2) == (1, 4) and rh.linear16_build(12288, 322)[1] == 12
    # every scalar / vector epilogue of k_rows16 and every layout-forced G1 / G2 of k_gemm appears
    assert {_label(c)[2] for c in F32_CASES if c.id.startswith("layout-")} == {"G1", "G2", "G4+A2"}
    g = _graph("degrees")
    assert set(rh.in_degrees(g).tolist()) == set(DEGREES)
    big = _graph("isolated+bonds+chains33k")
    assert int(big.V.shape[0]) > 32768 and set(rh.in_degrees(big).tolist()) == {0, 1, 2}
    assert int(_graph("no-edges").edge_index.shape[1]) == 0 and int(_graph("no-edges").V.shape[0]) == 3
    assert {c.build for c in SCASES} == {"vec-none", "vec-relu", "vec-generic", "scalar"}
    for c in SCASES:   # the build label of a segment case, from launch_segment's rule
        ld = dict(c.layout)
        vec = c.h % 4 == 0 and ld.get("ld_in", c.h) % 4 == 0 and ld.get("ld_out", c.h) % 4 == 0 and ld.get("off_in", 0) % 4 == 0 and ld.get("off_out", 0) % 4 == 0
        # (dmpnn_aggregate_fwd has no undirected flag: an undirected case runs its aggregate half on the directed build)
        want = "scalar" if not vec else ("vec-generic" if c.undirected or c.act not in ("none", "relu") else f"vec-{c.act}")
        assert c.build == want, (c.id, want)


def test_fwd_references_and_yardsticks_on_cpu():
    """Every reference is finite and not identically zero, and ``MARGIN * e32`` stays under the cap for every case: the float32
    yardstick decides the bar, never the cap.  The linear reference is the loop-free definition; an index equal to the number of source
    rows is a zero row."""
    for c in F32_CASES + F16_CASES + OOB:
        _, r64, _, e32 = _lref(c)
        for k in ("C", "Zpre"):
            assert bool(torch.isfinite(r64[k]).all()) and float(r64[k].abs().max()) > 0, (c.id, k)
            assert MARGIN * e32[k] <= rh.CAP["fwd"], (c.id, k, e32[k])
    _lin.cache_clear()
    for c in SCASES:
        for which in ("message", "aggregate"):
            r64, _, e32 = _sref(c.graph, c.h, which, c.act, c.undirected and which == "message")
            assert bool(torch.isfinite(r64).all()) and float(r64.abs().max()) > 0, (c.id, which)
            assert MARGIN * e32["out"] <= rh.CAP["fwd"], (c.id, which, e32)
    _sref.cache_clear()
    inp = rh.linear_inputs(9, 5, 3, 2, n_src=4, seed=1)
    inp["gather"][2] = 4
    r = rh.linear_ref(inp, "leakyrelu")
    a1 = torch.cat((inp["A1"], torch.zeros(1, 3)))[inp["gather"].long()]
    z = torch.einsum("mk,nk->mn", torch.cat((a1, inp["A2"]), 1).double(), inp["W"].double()) + inp["bias"].double() + inp["Cadd"].double()
    assert torch.allclose(r["Zpre"], z, rtol=1e-14, atol=1e-15) and torch.equal(r["C"], torch.where(r["Zpre"] > 0, r["Zpre"], 0.1 * r["Zpre"]))
    assert torch.equal(r["Zpre"][2], (inp["A2"][2].double() @ inp["W"][:, 3:].double().t() + inp["bias"].double() + inp["Cadd"][2].double()))
    g = _graph("degrees")
    H = _hin("degrees", 3).double()
    m = rh.segment_fwd_ref(g, H, "message", "none", True)
    Hu = (H + H[g.rev_edge_index]) / 2
    S = torch.zeros(int(g.V.shape[0]), 3, dtype=torch.float64).index_add_(0, g.edge_index[1], Hu)
    assert torch.allclose(m, S[g.edge_index[0]] - Hu[g.rev_edge_index], rtol=1e-13, atol=1e-13)
