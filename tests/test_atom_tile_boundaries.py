"""The TILE kernels with ATOM messages — ``AtomMessagePassing`` (base.py:254-289, mixins.py:21-30) as ``DMPNN_F_ATOM`` on the
whole-forward tile kernel ``k_mpnn_tile16`` (csrc/dmpnn_mega16_impl.hpp, the ``if (G.atom_de)`` block) and its backward twin
``k_mpnn_tile16_bwd`` (csrc/dmpnn_mega16_bwd_impl.hpp, ``g.atom``) with ``W_h``'s weight-gradient product over ``[M^(t) || ME]``
(csrc/dmpnn_backward.hip, ``lda2 = 16``) — through ``engine.forward(plan, ..., atom=True, keep=..., route="mega", out=...)`` /
``engine.backward`` at the seams of their dispatch, against float64 on the CPU (``atom_harness.block_ref``), on the FULL plan (kept
tensors in CSR-row order) and on the TILE plan (``DMPNN_F_TILE_PLAN``: the caller's edge order).  ``tile_harness.run_tile`` asserts
``st.route == "mega16"``, ``DMPNN_F_ATOM``, the plan's kind and ``DMPNN_F_TILE_PLAN`` for every run.

The contract of one case is the bond sweep's (``tests/test_tile_boundaries.py``), unchanged: ``out``, every gradient, ``gW_h`` as a whole
and its two column blocks ``[:, :d_h]`` / ``[:, d_h:]`` on their own (``atom_harness.named``) in the metric WITHOUT a floor, ``err =
max|got - ref64| / max|ref64|``, within ``min(MARGIN max(e32, 2**-23), cap)`` — ``MARGIN = rows_harness.MARGIN``, ``cap =
rows_harness.CAP``, ``e32`` the same restatement in float32 under the same decisions.  NaN-prefilled buffers with an offset and
padding columns whose guard regions must come back untouched; two backward passes bit for bit; ReLU-class gradients against float64
GIVEN the run's own decisions (the sign of the kept fp32 ``H0`` / ``H^(t)`` and of ``out``), those held by ``lean_harness.sign_check``
(band ``BAND``, at most ``MAX_FLIPS`` per case: a condition).  On the tile plan the run WITH sign bits gives ``out`` and every gradient
bit-identical to the fp32-row run.  Every case also runs inference (the ``KEEP = false`` builds).  The kept ``ME`` (``msplit``: ``depth -
1`` slots of ``[n_edges][16]``): every slot equals slot 0 bit for bit, columns ``>= d_e`` are exactly 0, the rows meet float64
``atom_message_ref(bmg, E)`` at the gradient bar in the kept order, and on the tile plan they EQUAL ``atom_message_seq32`` — read in the
kernel: ``SE[a]`` adds the rows of the tile with ``aor[r] == a`` for ``r = 0, 1, ..`` starting from ``0.f``, and on that plan row ``r`` is
the caller's edge ``rs + r`` (on the full plan it is CSR row ``rs + r``: stable by destination, hence the same order within an atom,
and the test asserts equality there as well).

Read before the first run (the dispatch against the case list; nothing found, so no kernel or host code changes here):
* LDS: ``lds_bytes<WN>`` reserves ``(3 BM + BA + 24) 4 = 800`` bytes of metadata where ``cfrag`` starts at ``ceil16((3 BM + BA + 9) 4) =
  752``; ``Et = cfrag + 10 * 64`` (16-byte units) and ``SE`` take ``kAtomLds = 5 120`` bytes and end at ``tile + 752 + 10 240 + 5 120 <=
  lds_bytes_atom<WN>``.  Every ``<WN, SA, KEEP, NW>`` launcher — the 8-wave one goes through the same macro — passes
  ``lds_bytes_atom<WN>()`` when ``g.atom_de`` and raises the function's limit to it (78 368 bytes at ``WN = 5``: two per CU).
* ``k_split_weights``: the grid is ``ceil(N / 16) * 4 * n_jobs`` blocks of four waves = ``Np * n_jobs`` waves, wave -> job ``wave / Np``:
  it covers ``n_jobs`` = 5 (inference) and 7 (training); K0's riders (csrc/dmpnn_prepare.hip) size theirs from ``sp.n_jobs`` too.  The
  seventh job reads ``W_h`` with leading dimension ``d_h + d_e`` from column ``d_h``, one chunk, its own row scales.
* ``ws_layout`` adds ``whe`` (``NT * 2048``) and ``sc_e`` for ``DMPNN_F_ATOM``; ``dmpnn_forward_wsplit_bytes`` — what the engine
  allocates, AFTER it has set ``DMPNN_F_ATOM`` and ``DMPNN_F_KEEP`` — is that total plus the backward's two transposed matrices, which
  ``launch_mega16_backward`` finds behind ``mega16_fwd_wsplit_bytes`` (the same total).
* ``atom_me``: ``for i < nrows * 16`` writes every row ``rs + r`` of a regular tile into every slot on both plans (source atom
  ``asrc[r]`` | ``aor[revl[r]]``); a tile without rows has none.  Depth 1 passes no ``atom_me``.
* The product: ``k_wsplit16`` reads ``[M^(t) || ME]`` as column pairs — ``K1 = d_h`` and ``K2 = d_e`` are even, no pair straddles the two
  operands, ``ME``'s rows are 16 floats apart; ``plan_wgrad16`` gets ``kt_h = d_h + d_e (+ 1)``; depth 1 zeroes ``gW_h`` as ``[d_h, d_h + d_e]``.
* A molecule beyond the tile (lines 363-377): with ``G.atom_de`` the workgroup writes NaN to ``out`` rows ``va .. vb - 1`` (``vb <= n_atoms``
  was checked two lines above), with ``KEEP`` also to the kept ``H^(t)`` of its rows, and returns: defined output.

Left out: dropout and molecules beyond the tile in TRAINING (refused — ``test_atom_tile_refusals*`` — or loud by design; the module never
sends such a batch there: ``tests/test_atom_mp.py``); the f16-operand inference form (bond messages only, not fp32-class); the aggregate
ride of ``dmpnn_train_step`` (``tests/test_atom_step.py``); no case poisons or faults a launch.

Instantiation -> case (forward ``launch_mega16<WN, SA, KEEP[, 8]>`` with ``lds_bytes_atom``; every case runs KEEP = true and KEEP = false):
``<1, true, *>`` ``h4/8/36/60/64-relu-*``, ``h16-e16``, ``h60-e2``, ``h60-e16``, ``h64-e14``, ``h36-v*``, ``h36-act-relu/leakyrelu/identity``,
``h4/h36-depth*``, ``h4-<edge graph>``, ``h36-E0*``, ``h36-padded``; ``<1, false, *>`` ``h4..64-tanh-*``, ``h36-act-tanh/elu``;
``<2, true, *>`` ``h68/128-relu-*``, ``h68-<edge graph>``; ``<2, false, *>`` ``h68/128-tanh-*``; ``<5, true, *, 8>`` ``h132..320-relu-*``,
``h300-e16``, ``h320-v128``, ``h132-act-relu/leakyrelu/identity``, ``h132-depth8`` (qm9x12: at most one tile per CU); ``<5, false, *, 8>``
``h132..320-tanh-*``, ``h132-act-tanh/elu``, ``h300-padded``; ``<5, true, *>`` (4 waves) ``h132-waves4-relu`` (bonds2600),
``h300-waves4-chains-relu``; ``<5, false, *>`` ``h300-waves4-tanh``.  Backward ``launch_mega16_bwd<WN, SA[, 8]>``: the same ids.  Kept
forms: fp32 rows (every ``@full`` run, the first run of every ``@tiles`` case) and sign bits (the second run of every ReLU-class /
identity ``@tiles`` case).  The wave counts of these graphs are asserted by ``test_tile_boundaries.py::test_tile_plans_are_the_edges_the_cases_name``.

The bar's resolution (``test_atom_wrong_references_fail_on_cpu``: wrong REFERENCES as test code, never a wrong kernel): the block
restated with the reverse-edge term subtracted (bond semantics), ``ME`` taken at ``dst``, ``ME`` dropped, the ``d_e`` columns of ``W_h``
rolled by one, and the bond-feature sum added to ``H0`` before the first activation — each fails the same ``compare`` under the same
``e32`` on every case where it differs mathematically (not at depth 1 for the first four, not at ``E = 0`` for the last four; there it
is identical and passes).  That says the case set and the bar can tell these apart, nothing about the kernels.

MARGIN (``rows_harness.MARGIN`` = 16, unchanged).  Measured on the MI355X from the ``ATOMBAR`` report lines of every run (109 GPU tests, 1 411
tensor comparisons): the worst ``err / max(e32, 2**-23)`` is 2.92 — ``out`` of ``h4-pack-exact@tiles`` (err 3.5e-7 against a float32 draw of
1.0e-7, below ``2**-23``) — then 2.63 (``gW_h[:, :d_h]``, ``h4-pack-exact@tiles``), 2.47 (``out``, ``h36-depth1``), 2.20 (``out``,
``h36-mixed-oversize``), 2.10 (``out``, ``h4-chain25@tiles``), 2.08 (``gb_i``, ``h300-relu-bias@tiles`` and ``h68-degrees@mol@tiles``), 2.03 (``out``,
``h68-pack-exact@full``), 1.95 (``gW_h[:, d_h:]``, ``h36-depth8-chains@full``).  2 x 2.92 = 5.8 <= 16: MARGIN stays.  The bars are 1.9e-6 .. 2e-5
(38 comparisons sit at their cap, 18 references are exactly zero and so is what the kernels give).  Decisions: 2 flips in all, both in
``h300-waves4-chains-relu@full`` (6.1 million decisions, inside the band; the limit is 2 per case), 0 in every other run.  The
sign-bit run equalled the fp32-row run bit for bit in ``out`` and every gradient everywhere; the kept ``ME`` equalled the float32 sum in
increasing edge id on BOTH plans.  Nothing faulted or hung; the sweep found no error in the kernels.  Wall time of the module's GPU
tests on the MI355X: 3.8 s (the bond tile module: 5.2 s); the slowest test takes 0.4 s.
"""
import ctypes as C
import functools
import zlib

import numpy as np
import pytest
import torch

import atom_harness as ah
import lean_harness as lh
import rows_harness as rh
import tile_harness as th
from lean_harness import Case

MARGIN = rh.MARGIN
gpu = pytest.mark.gpu
# d_h at the seams of the builds: WN = 1 | 2 | 5 (64 | 128 | 320), partial 32-column chunks and 16-column tiles, qn == 1 (d_h = 4)
WIDTHS = (4, 8, 36, 60, 64, 68, 128, 132, 192, 256, 260, 300, 320)
EDGE_GRAPHS = ("chain25", "star24", "ions32", "atoms40", "pack-exact", "degrees@mol")
OVERSIZE = ("chain26", "ions33", "mixed-oversize")
ACTS = ("relu", "leakyrelu", "identity", "tanh", "elu")
ZERO_MOL = 5                 # "E0-mol": the molecule of qm9x12 whose bond features are all zero
WRONG = ("rev", "dst", "drop", "shift", "early")


def _runs():
    """-> [(case, plan kind)]"""
    rs = []
    nm = lambda b: "bias" if b else "nobias"
    # widths: ReLU on the tile plan (fp32 rows, then sign bits), tanh (the SA = false builds) on the full plan
    rs += [(Case(f"h{h}-relu-{nm(i % 2)}", "qm9x12", h, depth=3, bias=bool(i % 2)), "tiles") for i, h in enumerate(WIDTHS)]
    rs += [(Case(f"h{h}-tanh-{nm(1 - i % 2)}", "qm9x12", h, depth=3, act="tanh", bias=bool(1 - i % 2)), "full") for i, h in enumerate(WIDTHS)]
    # d_e: the ME row is 16 wide, one chunk of W_h[:, d_h:] (16: no zero padding at all); d_h + d_e on, below and above a 32-column chunk
    for i, (h, de) in enumerate(((16, 16), (60, 2), (60, 16), (64, 14), (300, 16))):
        rs += [(Case(f"h{h}-e{de}", "qm9x12", h, d_e=de, bias=bool(i % 2)), k) for k in th.PLANS]
    # d_v: the K1 operand is V alone (nc_i counts d_v only); d_v + d_h = 448, the largest shape mega_shapes_ok takes
    for i, (h, dv, de) in enumerate(((36, 2, 4), (36, 30, 4), (36, 32, 4), (36, 34, 4), (320, 128, 2))):
        rs += [(Case(f"h{h}-v{dv}", "qm9x12", h, d_v=dv, d_e=de, bias=bool(1 - i % 2)), k) for k in th.PLANS]
    # activations: one plan each, alternating
    for h in (36, 132):
        rs += [(Case(f"h{h}-act-{act}", "qm9x12", h, act=act, bias=bool(i % 2)), th.PLANS[(i + h // 100) % 2]) for i, act in enumerate(ACTS)]
    # depth (deep cases on graphs with long paths)
    rs += [(Case("h36-depth1", "qm9x12", 36, depth=1, bias=True), k) for k in th.PLANS]
    rs += [(Case("h4-depth2-chains", "chains12x10@mol", 4, depth=2, bias=True), "full"), (Case("h4-depth8-chains", "chains12x10@mol", 4, depth=8), "tiles"),
           (Case("h36-depth2-chains", "chains12x10@mol", 36, depth=2), "tiles"), (Case("h36-depth8-chains", "chains12x10@mol", 36, depth=8, bias=True), "full"),
           (Case("h132-depth8", "qm9x12", 132, depth=8), "tiles")]
    # tile edges
    rs += [(Case(f"h{h}-{g}", g, h, bias=True), k) for g in EDGE_GRAPHS for h in (4, 68) for k in th.PLANS]
    # zero bond features: on every edge of one molecule; everywhere (sE of an all-zero operand, gW_h[:, d_h:] exactly zero)
    rs += [(Case("h36-E0-mol", "qm9x12", 36, depth=3, gmode="E0-mol"), k) for k in th.PLANS]
    rs += [(Case("h36-E0", "qm9x12", 36, depth=3, bias=True, gmode="E0"), k) for k in th.PLANS]
    # waves: 4-wave WN = 5 tiles by shape (with atom messages a bond's message is H[rev e]: nothing is zero on bonds2600)
    rs += [(Case("h132-waves4-relu", "bonds2600", 132, bias=True), "tiles"), (Case("h300-waves4-tanh", "bonds2600", 300, act="tanh"), "tiles"),
           (Case("h300-waves4-chains-relu", "chains3x1700", 300, depth=3), "full")]
    # layout
    rs += [(Case("h36-padded", "qm9x12", 36, pad=4, bias=True), "tiles"), (Case("h300-padded", "qm9x12", 300, depth=3, act="tanh", pad=12), "full")]
    assert len({(c.id, k) for c, k in rs}) == len(rs)
    by_id = {}
    for c, _ in rs:
        assert by_id.setdefault(c.id, c) == c, c.id
    return rs


RUNS = _runs()
CASES = list({c.id: c for c, _ in RUNS}.values())
LOUD = [(Case(f"h{h}-{g}", g, h, act=act, bias=h == 36), k) for g in OVERSIZE for h, act in ((36, "relu"), (132, "tanh")) for k in th.PLANS]
_ids = lambda r: f"{r[0].id}@{r[1]}" if isinstance(r, tuple) else None
_relu_class = lambda case: case.act in lh.RELU_CLASS


# ---- operands and references -----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _operands(case: Case):
    """-> (the batch with ``V`` / ``E`` redrawn at the case's ``d_v`` / ``d_e``, the float32 operands as ``run_tile`` takes them): a
    seeded generator per case id; rows of the weights graded as in ``lean_harness.inputs`` (a transposed or shifted tile cannot pass)."""
    from chemprop_amd.data import BatchMolGraph

    g = lh.graph(case.graph)
    nV, nE = int(g.V.shape[0]), int(g.edge_index.shape[1])
    gen = torch.Generator().manual_seed(zlib.crc32(("atom/" + case.id).encode()) + 7919 * case.seed)
    h, dv, de = case.d_h, case.d_v, case.d_e
    vec = lambda n_in: (2 * torch.rand(h, generator=gen) - 1) / max(n_in, 1) ** 0.5
    V, E = torch.randn(nV, dv, generator=gen), torch.randn(nE, de, generator=gen)
    if case.gmode == "E0":
        E = torch.zeros_like(E)
    elif case.gmode == "E0-mol":
        E[g.batch[g.edge_index[0]] == ZERO_MOL] = 0.0
    else:
        assert case.gmode == "randn", case.gmode
    inp = dict(V=V, E=E, W_i=lh._lin(gen, h, dv), W_h=lh._lin(gen, h, h + de), W_o=lh._lin(gen, h, dv + h), b_o=vec(dv + h),
               b_i=vec(dv) if case.bias else None, b_h=vec(h + de) if case.bias else None)
    inp["G"] = torch.randn(nV, h, generator=gen) * (1 + torch.arange(h).float() / h)
    bmg = BatchMolGraph.from_tensors(V, E, g.edge_index, g.rev_edge_index, g.batch, len(g))
    return bmg, inp


def _named(case, dtype, decisions=None):
    bmg, inp = _operands(case)
    out, L, pre, made = ah.block_ref(bmg, inp, case.depth, case.act, dtype, decisions=decisions)
    return ah.named(out, ah.block_grads(out, L, inp["G"]), case.d_h), pre, made


@functools.lru_cache(maxsize=None)
def _yard(case: Case):
    """-> ``(ref64, pre64, e32, fails32)``: the float64 restatement with its own decisions (named tensors), its pre-activations, the
    float32 restatement's error against it per tensor (under the float64 decisions: linear algebra, no kink) and what ``sign_check``
    says about the float32 restatement's OWN decisions."""
    ref64, pre64, made = _named(case, torch.float64)
    ref32, _, _ = _named(case, torch.float32, made if _relu_class(case) else None)
    fails32 = []
    if _relu_class(case):
        bmg, inp = _operands(case)
        pre32 = ah.block_ref(bmg, inp, case.depth, case.act, torch.float32)[2]
        fails32 = lh.sign_check(case.id, lh.true_masks(pre32), pre64)[0]
    return ref64, pre64, ah.yardstick(ref64, ref32), fails32


def _must_be_zero(case):
    """The compared tensors whose reference is identically zero — and which the kernels then have to give exactly."""
    z = set()
    if case.depth == 1:
        z |= {"gW_h", "gW_h[:, :d_h]", "gW_h[:, d_h:]"} | ({"gb_h"} if case.bias else set())
    if case.gmode == "E0":
        z.add("gW_h[:, d_h:]")
    return z


def _me_yard(case):
    bmg, _ = _operands(case)
    me64 = ah.atom_message_ref(bmg, bmg.E)
    return me64, ah.yardstick(dict(ME=me64), dict(ME=ah.atom_message_ref(bmg, bmg.E, torch.float32)))


def _wrong_block(case: Case, variant):
    """The block restated apart from ``atom_harness.block_ref`` (``variant = "right"``: the same function) with one deliberate error:
    ``rev`` the reverse-edge term subtracted from the hidden half of the message (bond semantics), ``dst`` ``ME`` taken at the
    destination atom, ``drop`` no ``ME``, ``shift`` the ``d_e`` columns of ``W_h`` rolled by one, ``early`` the bond-feature term joins
    ``H0`` BEFORE the first activation.  float64, the activation's own decisions -> the named tensors."""
    from oracle import dmpnn_torch as ot

    bmg, inp = _operands(case)
    f = lambda t: None if t is None else t.detach().double().requires_grad_(True)
    L = {k: f(inp[k]) for k in ah.PARAMS}
    V, E = bmg.V.double(), bmg.E.double()
    src, dst = bmg.edge_index
    rev, nV, h = bmg.rev_edge_index, int(V.shape[0]), case.d_h
    tau = ot.activation_fn(case.act)
    lin = torch.nn.functional.linear
    Wh_H, Wh_E = L["W_h"][:, :h], L["W_h"][:, h:]
    if variant == "shift":
        Wh_E = torch.roll(Wh_E, 1, dims=1)
    SE = ot.segment_sum_dst(E, dst, nV)
    ME = SE[dst] if variant == "dst" else SE[src]
    xE = (torch.zeros_like(ME) if variant == "drop" else ME) @ Wh_E.t()
    H0 = lin(V[src], L["W_i"], L["b_i"])
    if variant == "early":
        H0 = H0 + xE
    H = tau(H0)
    for _ in range(1, case.depth):
        MH = ot.segment_sum_dst(H, dst, nV)[src]
        if variant == "rev":
            MH = MH - H[rev]
        z = H0 + lin(MH, Wh_H, L["b_h"])
        H = tau(z if variant == "early" else z + xE)
    out = tau(lin(torch.cat((V, ot.segment_sum_dst(H, dst, nV)), 1), L["W_o"], L["b_o"]))
    return ah.named(out, ah.block_grads(out, L, inp["G"]), h)


def _differs(case, variant):
    """Where a wrong restatement is NOT the right one: the first four touch the messages only (depth > 1), the last four the
    bond features only (``E != 0``)."""
    return (variant == "early" or case.depth > 1) and (variant == "rev" or case.gmode != "E0")


# ---- the route on the device -----------------------------------------------------------------------------------------------------------
def _got(case, res, i=0):
    return ah.named(res["out"], res["grads"][i], case.d_h)


def _grads(tag, case, kind, res, ref, e32, fails, worst):
    got = _got(case, res)
    assert set(got) == set(ref), (set(got) ^ set(ref))
    f, w = ah.compare(f"{case.id}@{kind}/{tag}", got, ref, e32, MARGIN)
    fails += [f"{tag}: {x}" for x in f]
    worst.append(w)
    for k in _must_be_zero(case):
        assert not bool(got[k].any()), f"{tag}: {k} must be exactly zero"
    a, b = res["grads"]
    for k in a:
        if not torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)):
            fails.append(f"{tag}: g{k}: two backward passes differ")


def _kept_me(case, kind, res, fails):
    """The kept bond-feature half of the messages: ``depth - 1`` identical slots of ``[n_edges][16]`` rows in the kept order."""
    bmg, _ = _operands(case)
    st = res["st"]
    if case.depth == 1:   # no message, no slot to write: the gradient of W_h is zeroed, not computed
        return
    ME = st.refs[15].cpu()
    nE = int(bmg.E.shape[0])
    assert tuple(ME.shape) == (case.depth - 1, nE, 16) and st.args.msplit == st.refs[15].data_ptr() and st.args.msplit_bytes == ME.numel() * 4
    for t in range(1, case.depth - 1):
        if not torch.equal(ME[t].view(torch.int32), ME[0].view(torch.int32)):
            fails.append(f"ME: slot {t} differs from slot 0")
    if bool(ME[0][:, case.d_e:].view(torch.int32).any()):
        fails.append("ME: a column >= d_e is not exactly zero")
    rows = ME[0] if kind == "tiles" else ME[0][st.plan.inv32.long().cpu()]   # -> the caller's edge order
    me64, e32 = _me_yard(case)
    f, _ = ah.compare(f"{case.id}@{kind}/kept", dict(ME=rows[:, :case.d_e]), dict(ME=me64), e32, MARGIN)
    fails += f
    # the kernel adds a tile's rows in increasing row order from 0.f: the caller's edge order on the tile plan, the stable CSR order
    # (increasing edge id within an atom) on the full plan — either way the float32 sum in increasing edge id
    if not bool((rows[:, :case.d_e] == ah.atom_message_seq32(bmg, bmg.E)).all()):
        fails.append("ME: not the float32 sum of the incoming rows in increasing edge id")


def _hold(dev, case, kind):
    """The whole contract of one case on one plan."""
    _, inp = _operands(case)
    ref, pre64, e32, _ = _yard(case)
    fails, worst = [], []
    run = lambda **kw: th.run_tile(dev, case, kind, atom=True, inputs=inp, **kw)
    a = run(bits=False)
    assert not a["st"].args.keep_bits and a["sites"] is not None
    flips = 0
    if _relu_class(case):
        sf, flips = lh.sign_check(case.id, a["sites"], pre64)
        fails += sf
        if flips:
            ref = _named(case, torch.float64, a["sites"])[0]
    print(f"ATOMSIGN {case.id}@{kind} flips={flips}")
    _grads("rows", case, kind, a, ref, e32, fails, worst)
    _kept_me(case, kind, a, fails)
    if kind == "tiles" and (_relu_class(case) or case.act == "identity"):
        # the sign-bit form: the same output AND the same gradients bit for bit; held to the reference given the SAME decisions as well
        b = run(bits=True)
        assert b["st"].args.keep_bits and b["sites"] is None
        for k, x in _got(case, a).items():
            if not torch.equal(x.view(torch.int32), _got(case, b)[k].view(torch.int32)):
                fails.append(f"bits: {k} differs from the run that kept fp32 rows")
        _grads("bits", case, kind, b, ref, e32, fails, worst)
        _kept_me(case, kind, b, fails)
    else:
        assert not run(bits=True, backward=0)["st"].args.keep_bits, "sign bits where the library refuses them"
    inf = run(keep=False)   # the KEEP = false builds
    f, w = ah.compare(f"{case.id}@{kind}/inference", dict(out=inf["out"]), dict(out=ref["out"]), e32, MARGIN)
    fails += [f"inference: {x}" for x in f]
    print(f"ATOMBAR {case.id}@{kind} worst-ratio={max(worst + [w]):.2f}")
    assert not fails, f"{case.id}@{kind}: " + "; ".join(fails)


@gpu
@pytest.mark.parametrize("run", RUNS, ids=_ids)
def test_atom_tile_route(run, gpu_device):
    _hold(gpu_device, *run)


@gpu
@pytest.mark.parametrize("run", LOUD, ids=_ids)
def test_atom_molecule_beyond_the_tile_is_loud(run, gpu_device):
    """Inference only: the generic path knows bond messages only, so every atom of a tile beyond 48 rows / 32 atoms comes back NaN —
    loud, never wrong — and every other atom meets the forward bar.  (The full plan packs connected pieces: ``ions33`` has no tile
    beyond the limits there and is computed whole.)"""
    case, kind = run
    _, inp = _operands(case)
    ref, _, e32, _ = _yard(case)
    tr, ta, over = th.tile_rule(case.graph, kind)
    loud = torch.zeros(ref["out"].shape[0], dtype=torch.bool)
    for i in range(len(tr) - 1):
        if tr[i + 1] - tr[i] > th.BM or ta[i + 1] - ta[i] > th.BA:
            loud[int(ta[i]):int(ta[i + 1])] = True
    assert int(loud.sum()) == {"chain26": 26, "ions33": 33 if kind == "tiles" else 0, "mixed-oversize": 26}[case.graph] and (over > 0) == bool(loud.any())
    res = th.run_tile(gpu_device, case, kind, keep=False, atom=True, inputs=inp)
    out = res["out"]
    assert bool(torch.isnan(out[loud]).all()), "an atom of a molecule beyond the tile must come back NaN"
    if bool((~loud).any()):
        fails, _ = ah.compare(f"{case.id}@{kind}/inference", dict(out=out[~loud]), dict(out=ref["out"][~loud]), e32, MARGIN)
        assert not fails, f"{case.id}@{kind}: " + "; ".join(fails)


# ---- refusals: an argument error writes nothing ------------------------------------------------------------------------------------------
def _flags(keep):
    from chemprop_amd import _lib

    return _lib.F_FUSED | _lib.F_MEGA | _lib.F_SPLIT16 | _lib.F_ATOM | (_lib.F_KEEP if keep else 0)


def _with_wd(a):
    a.W_d, a.b_d, a.V_d, a.Hv, a.d_vd, a.ldvd = a.W_h, a.b_o, a.V, a.Mv, 2, a.ldv   # (never dereferenced: the call is refused)
    a.ldout = max(a.ldout, (a.d_h + 2 + 3) // 4 * 4)


def _set(**kw):
    def f(a):
        for k, v in kw.items():
            setattr(a, k, v)
    return f


def _short(a):
    a.msplit_bytes -= 64


def _unaligned(a):
    a.msplit += 4


# (name, DMPNN_F_KEEP, the change to a valid argument block, a word of the message)
REFUSALS = (("d_e = 0", False, _set(d_e=0), "DMPNN_F_ATOM"), ("d_e = 18", False, _set(d_e=18, lde=18), "DMPNN_F_ATOM"),
            ("dropout", True, _set(dropout_p=0.25), "DMPNN_F_ATOM"), ("W_d", False, _with_wd, "DMPNN_F_ATOM"),
            ("keep, odd d_v", True, _set(d_v=7, ldv=8), "even d_v"), ("keep, odd d_e", True, _set(d_e=3), "even d_v"),
            ("keep, d_h = 6", True, _set(d_h=6, ldh=8, ldout=8), "shapes"), ("msplit one row short", True, _short, "msplit"),
            ("msplit not 16-byte aligned", True, _unaligned, "msplit"))


def _refused(lib, base, stream=None):
    """Every entry of ``REFUSALS`` applied to a copy of ``base``: ``DMPNN_EINVAL`` with the message each time."""
    for name, keep, change, word in REFUSALS:
        a = type(base).from_buffer_copy(base)
        a.flags = (a.flags & ~_flags(True)) | _flags(keep)
        change(a)
        rc = int(lib.dmpnn_forward(C.byref(a), stream))
        msg = lib.dmpnn_last_error_string().decode(errors="replace")
        assert rc == rh.EINVAL and word in msg, (name, rc, msg)


def test_atom_tile_refusals_before_touching_the_device():
    """``dmpnn_forward`` with the tile flags and ``DMPNN_F_ATOM`` checks its arguments before anything reaches the device (no GPU here,
    as ``tests/test_head_descriptors.py`` does for the head): every entry of ``REFUSALS`` is ``DMPNN_EINVAL`` with a message, and the
    host buffers standing in for ``out`` and ``msplit`` keep every word.  (No ``wsplit``: even an accepted call would end with
    ``DMPNN_ENOSPC`` before its first launch.)"""
    from chemprop_amd import _lib

    lib = _lib.load()
    nV, nE, dv, de, h, depth = 110, 102, 6, 4, 36, 3
    mem = np.zeros(1 << 16, dtype=np.float32)            # stands in for every operand: the checks look at pointers, never behind them
    out = np.full(nV * h + 64, np.float32(7.0))
    me = np.full((depth - 1) * nE * 16 + 64, np.float32(7.0))
    assert all(x.ctypes.data % 16 == 0 for x in (mem, out, me))
    a = _lib.FwdArgs()
    a.n_atoms, a.n_edges, a.d_v, a.d_e, a.d_h, a.depth = nV, nE, dv, de, h, depth
    a.flags, a.act = _flags(True), _lib.ACT["relu"]
    a.ldv, a.lde, a.ldh, a.ldout = dv, de, h, h
    for k in ("plan", "V", "E", "W_i", "W_h", "W_o", "b_o", "H0", "Hs", "Ms", "Mv", "Hv", "edge_index", "rev_edge_index"):
        setattr(a, k, mem.ctypes.data)
    a.n_hslots = a.n_mslots = depth - 1
    a.out, a.msplit, a.msplit_bytes = out.ctypes.data, me.ctypes.data, (depth - 1) * nE * 64
    assert int(lib.dmpnn_forward_can_fuse(C.byref(a))) == 2
    _refused(lib, a)
    assert bool((out == 7.0).all()) and bool((me == 7.0).all()) and not mem.any()
    # the valid block gets past every argument check (and stops at the missing weight pre-split workspace, before any launch)
    rc = int(lib.dmpnn_forward(C.byref(a), None))
    assert rc == rh.ENOSPC and "wsplit" in lib.dmpnn_last_error_string().decode(), rc


@gpu
def test_atom_tile_refusals(gpu_device):
    """The same table on the argument block the engine prepares (``launch=False``), buffers on the device: ``out`` (NaN-prefilled
    ``Mat``) and ``msplit`` keep every word through all refusals; the unchanged block then runs.  ``engine.forward(..., atom=True,
    route="mega", dropout=...)`` raises ``RouteUnavailable`` before any launch."""
    from chemprop_amd import _lib, engine

    dev = gpu_device
    lib = _lib.load()
    case = Case("h36-refusals", "qm9x12", 36, depth=3, bias=True)
    bmg, inp = _operands(case)
    nV, nE = int(bmg.V.shape[0]), int(bmg.E.shape[0])
    for kind in th.PLANS:
        plan, _ = th.plan_of(case.graph, kind, dev)
        plan.ensure_launched()
        d = {k: (None if v is None else v.to(dev)) for k, v in inp.items()}
        out_m = rh.Mat(dev, nV, case.d_h, off=4)
        fwd = lambda **kw: engine.forward(plan, d["V"], d["E"], d["W_i"], d["W_h"], d["W_o"], d["b_o"], d["b_i"], d["b_h"], depth=case.depth,
                                          act="relu", keep=True, keep_bits=False, route="mega", atom=True, out=out_m.view(), **kw)
        n0 = int(lib.dmpnn_last_launch_count())
        with pytest.raises(engine.RouteUnavailable):
            fwd(dropout=(0.25, lh.DROP_SEED))
        assert int(lib.dmpnn_last_launch_count()) == n0 and out_m.pristine()
        _, st = fwd(launch=False)
        me = st.refs[15]
        assert tuple(me.shape) == (case.depth - 1, nE, 16)
        me.view(torch.int32).fill_(rh.PREFILL)
        with engine._OnDevice(dev):
            _refused(lib, st.args, engine._stream_ptr(dev))
            torch.cuda.synchronize()
            assert out_m.pristine() and bool((me.view(torch.int32) == rh.PREFILL).all()), "a refused call writes nothing"
            rc = int(lib.dmpnn_forward(C.byref(st.args), engine._stream_ptr(dev)))
        torch.cuda.synchronize()
        assert rc == 0, lib.dmpnn_last_error_string().decode(errors="replace")
        ref, _, e32, _ = _yard(case)
        fails, _ = ah.compare(f"{case.id}@{kind}/after-refusals", dict(out=out_m.read("out")), dict(out=ref["out"]), e32, MARGIN)
        assert not fails, fails
        assert bool(torch.isfinite(me).all())


# ---- where no GPU is needed ----------------------------------------------------------------------------------------------------------
def test_atom_tile_references_on_cpu():
    """Every case: ``block_ref`` in float64 is ``oracle.dmpnn_torch.atom_forward``; the float32 restatement meets the caps under the
    float64 decisions and its own decisions stay within ``MAX_FLIPS`` inside the band; no compared reference tensor is identically
    zero unless it must be (depth 1: ``gW_h`` / ``gb_h``; ``E = 0``: ``gW_h[:, d_h:]``) — those the kernels have to give exactly."""
    from oracle import dmpnn_torch as ot

    for case in CASES + [c for c, _ in LOUD[::2]]:
        bmg, inp = _operands(case)
        ref, pre64, e32, fails32 = _yard(case)
        assert not fails32, (case.id, fails32)
        assert len(pre64) == case.depth + 1
        mw = ot.MPWeights(*(None if inp[k] is None else inp[k].double() for k in ("W_i", "W_h", "W_o", "b_o", "b_i", "b_h")))
        o = ot.atom_forward(bmg.V.double(), bmg.E.double(), bmg.edge_index, bmg.rev_edge_index, mw, depth=case.depth, activation=case.act)
        assert torch.allclose(ref["out"], o, rtol=1e-12, atol=1e-14), case.id
        want = {"out", "gW_i", "gW_h", "gW_o", "gb_o", "gW_h[:, :d_h]", "gW_h[:, d_h:]"} | ({"gb_i", "gb_h"} if case.bias else set())
        assert set(ref) == set(e32) == want, case.id
        assert tuple(ref["gW_i"].shape) == (case.d_h, case.d_v) and tuple(ref["gW_h"].shape) == (case.d_h, case.d_h + case.d_e), case.id
        for k, t in ref.items():
            assert e32[k] < rh.CAP["fwd" if k == "out" else "grad"], (case.id, k, e32[k])
            assert (float(t.abs().max()) > 0) != (k in _must_be_zero(case)), (case.id, k)
        if case.depth > 1:
            me64, me32 = _me_yard(case)
            assert me32["ME"] < rh.CAP["grad"] and (float(me64.abs().max()) > 0) != (case.gmode == "E0"), case.id
        _yard.cache_clear()
    # the zero-feature cases are what they say
    bmg, _ = _operands(next(c for c in CASES if c.id == "h36-E0-mol"))
    on = bmg.batch[bmg.edge_index[0]] == ZERO_MOL
    assert 0 < int(on.sum()) < on.numel() and not bool(bmg.E[on].any()) and bool(bmg.E[~on].abs().min() > 0)
    # a smooth activation takes no decisions: the reference given "decisions" is the reference
    case = next(c for c in CASES if c.id == "h36-tanh-bias")
    ref, pre64, _, _ = _yard(case)
    given = _named(case, torch.float64, lh.true_masks(pre64))[0]
    assert all(torch.equal(ref[k], given[k]) for k in ref)
    # ... and fixed decisions of the ReLU class reproduce the free run: factor 1 or the slope
    for cid in ("h36-act-relu", "h36-act-leakyrelu"):
        case = next(c for c in CASES if c.id == cid)
        ref, pre64, _, _ = _yard(case)
        given = _named(case, torch.float64, lh.true_masks(pre64))[0]
        assert all(torch.equal(ref[k], given[k]) for k in ref), cid


def test_atom_wrong_references_fail_on_cpu():
    """The bar can tell wrong restatements apart (see the module docstring): each of ``WRONG`` against the right float64 reference, by
    the same ``compare`` under the same ``e32``, fails on every case where it differs mathematically — everywhere but at depth 1
    (``rev``, ``dst``, ``drop``, ``shift``) and at ``E = 0`` (``dst``, ``drop``, ``shift``, ``early``), where it is the right one and passes."""
    quiet = lambda s: None
    excepted = set()
    for case in CASES:
        ref, _, e32, _ = _yard(case)
        right = _wrong_block(case, "right")
        assert all(torch.allclose(right[k], ref[k], rtol=1e-10, atol=1e-13) for k in ref), case.id
        for variant in WRONG:
            fails, _ = ah.compare(f"{case.id}/{variant}", _wrong_block(case, variant), ref, e32, MARGIN, report=quiet)
            assert bool(fails) == _differs(case, variant), (case.id, variant, fails)
            if not fails:
                excepted.add((case.id, variant))
        _yard.cache_clear()
    assert excepted == {("h36-depth1", v) for v in ("rev", "dst", "drop", "shift")} | {("h36-E0", v) for v in ("dst", "drop", "shift", "early")}


def test_atom_tile_shapes_are_accepted_on_cpu():
    """``dmpnn_forward_can_fuse`` takes every swept shape for the tile kernel (2), padding included."""
    from chemprop_amd import _lib

    lib = _lib.load()
    for case in CASES + [c for c, _ in LOUD]:
        a = _lib.FwdArgs()
        a.n_atoms, a.n_edges, a.d_v, a.d_e, a.d_h, a.depth = 110, 102, case.d_v, case.d_e, case.d_h, case.depth
        a.flags = _lib.F_ATOM
        a.ldv, a.lde, a.ldh, a.ldout = case.d_v + case.pad, case.d_e + case.pad, case.d_h, case.d_h + case.pad
        a.act = _lib.ACT[lh.ENGINE_ACT[case.act][0]]
        assert int(lib.dmpnn_forward_can_fuse(C.byref(a))) == 2, case.id
    assert {c.d_e for c in CASES} == {2, 4, 14, 16} and {c.d_v for c in CASES} == {2, 6, 30, 32, 34, 128}
    assert max(c.d_v + c.d_h for c in CASES) == 448 and {c.act for c in CASES} == set(ACTS) and {c.depth for c in CASES} == {1, 2, 3, 8}
