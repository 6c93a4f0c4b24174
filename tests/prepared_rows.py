"""What a PREPARED call is, written down: the rows of ``tests/golden/prepared_calls.json`` (``tests/golden/make_prepared_calls.py``
writes them, ``tests/test_prepared_calls.py`` rebuilds and compares them).  A plain module: no fixtures, no pytest settings.

``engine.forward(..., launch=False)``, ``engine.backward(..., launch=False)``, ``GraphPlan(..., launch=False)`` and
``FusedTrainer._blocks`` only run host code — the route rule, the ``*_bytes`` rules, allocation, the argument blocks — so on CPU tensors,
with ``engine._require_device`` replaced by a no-op (the CALLER's job: the test uses ``monkeypatch``), they produce everything a call
would launch with.  A row is the full signature of one such call (the file writes it as what differs from an earlier row, see ``build_rows``):

* forward: route, slot counts, the shapes of the state's tensors, every ``FwdArgs`` field that is not zero / null — a pointer as
  ``name of the tensor it points into[+byte offset]`` — and shape and dtype of every entry of ``st.refs`` that is not ``None``; with ``keep`` the
  ``BwdArgs`` of ``engine.backward`` on it too; for a refusal the exception class and message;
* step: per block part the route, the plan's kind, the step's ``(p, seed)``, the forward row of its kept state — and for the step
  how many values it drew from torch's CPU generator (a refusal must have drawn none).

Nothing in a row depends on the machine: shapes, host rules of the library (whose CU-count fallback is the MI355X's own count) and
torch's CPU generator.

Which row reaches what (``forward/`` and ``step/`` prefixes left out; every refusal, workspace layout and flag has at least one):

* refusals of the forward — plan of another batch ``plan/other-batch``; atom weights ``atom/bond-weights``; ``out=`` ``out/misaligned``,
  ``out/slice/h30``; the rule on a light / tile plan ``rule/qm9x8/h30/light/keep0``, ``rule/qm9x8/h644/tiles/keep0``; demanded route
  ``route=fused/h30/keep0``, ``route=mega/h324``, ``route=fused16/h30/keep0``; a demand on a light / tile plan
  ``route=general/h32/light/keep0``, ``route=fused/h32/tiles/keep0``, ``mfma=f32/h32/tiles``; atom messages ``atom/de17/keep0``,
  ``atom/W_d``; dropout ``dropout/tanh/p0.25/tile`` (plain), ``dropout/lean/depth1`` (with the lean reason), ``dropout/rows/h31`` and
  ``dropout/relu/p1.0/rows`` (with the row kernels' reason).  The guard "a tile plan serves a training forward only on the tile
  kernel" behind the flags is reached by no input: the route stage refuses every such call first;
* workspace layouts — inference tile kernel ``rule/qm9x8/h32/tiles/keep0`` (spill scratch: ``rule/tiles/oversize=None``; none:
  ``rule/tiles/oversize=False``); lean ``route=fused16/h32/keep1`` (``xrow``: also ``route=fused16/h4/keep1``); kept fused16
  ``route=fused16/keep1/bits0/relu``, ``route=fused16/h324/keep1``; inference fused16 ``route=fused16/h32/keep0``, row quads beyond
  ``n_edges`` rows ``route=fused16/h324/keep0``, ``env/DMPNN_H0=x/route=fused16/keep0``; plain ``rule/qm9x8/h30/full/keep1`` (pad
  columns), fused on the fp32 pipe ``mfma=f32/fused/depth5/keep0`` (two message slots); atom on the general route
  ``atom/de1/general/keep0``, kept atom tile forward ``atom/de14/keep1``; split rows from 4 096 message rows ``rule/chain9x256/keep1``;
* flags — ``F_LOADER_TILES`` ``rule/chain9x1250/keep0``; ``F_ATOM`` ``atom/de14/keep0``; ``F_UNDIRECTED_MASK``
  ``undirected/dropout/mask1``; ``F_FUSED | F_MEGA | F_SPLIT16`` ``rule/qm9x8/h32/full/keep0``; ``F_MEGA`` alone ``mfma=f32/h32/keep0``;
  ``F_KEEP`` ``rule/qm9x8/h32/full/keep1``; ``F_TILE_PLAN`` and its sign bits ``rule/qm9x8/h32/tiles/keep1`` (none:
  ``rule/tiles/keep1/bits0/depth4``, ``rule/tiles/keep1/tanh``); ``F_STORE16`` ``env/DMPNN_STORE=f16/route=fused16/keep0``,
  ``env/DMPNN_STORE=f16/rule/keep0``; form bits ``route=fused16/form512``; the crossovers of the rule at 2 048 / 20 000 directed edges
  ``rule/chain9x127/level1`` | ``rule/chain9x128/level1``, ``route=general/chain9x1249`` | ``route=general/chain9x1250``;
* the step — bond: tile ``bond/p>0/tile``, lean ``bond/p>0/lean/oversize``, lean before rows ``bond/p>0/lean-before-rows``, rows
  ``bond/p>0/rows/tanh``, refusals ``bond/p>0/refused/*`` (these come from the forwards the step tried: the seed is drawn),
  ``bond/p>0/env-mfma-f32`` (the demanded route's own refusal translated); undirected gate ``undirected/p>0/refused/*``; atom: features
  ``atom/refused/features``, gate ``atom/p>0/refused/*``, tile ``atom/p0/tile``, general ``atom/p0/oversize``, no tile plan
  ``atom/p0/tile_plan=False/beyond-small-plan``; ``W_d/*``; ``multi/*``.  Not reached on CPU tensors: the device count of
  ``nn.batch_oversize``, ``validate=True`` (both launch kernels: the GPU tests' business), and three translations of refusals that the
  gates before them make unreachable (undirected and atom ``RouteUnavailable`` behind a passed gate, a tile plan without tile kernels).
"""
import contextlib
import ctypes as C
import os

import numpy as np
import torch

from chemprop_amd import _lib, engine, synth
from chemprop_amd.data import BatchMolGraph

ENV_KEYS = ("DMPNN_GENERAL", "DMPNN_MEGA", "DMPNN_MFMA", "DMPNN_H0", "DMPNN_STORE", "DMPNN_VALIDATE", "DMPNN_KEEP_ROWS", "DMPNN_TRAIN_PLAN")


@contextlib.contextmanager
def environment(env: dict):
    """The switches of ``env`` and none of the others, for the duration of one row."""
    old = {k: os.environ.get(k) for k in ENV_KEYS}
    try:
        for k in ENV_KEYS:
            os.environ.pop(k, None)
        os.environ.update(env)
        yield
    finally:
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


# ---- batches -------------------------------------------------------------------------------------------------------------------------
_batches: dict = {}


def batch(name: str, d_v: int = 72, d_e: int = 14) -> BatchMolGraph:
    """``qm9x8``; ``mixed`` (one single-atom molecule, QM9-shaped ones, one 40-atom molecule beyond the tile); ``empty`` (no edges);
    ``chainNxM`` (M chains of N atoms: 2 (N - 1) M directed edges exactly — the edge counts AT and just BELOW the route rule's
    crossovers); ``dense`` (40-atom molecules: more than 30 directed edges per molecule)."""
    key = (name, d_v, d_e)
    if key not in _batches:
        rng = np.random.default_rng(1234)
        if name == "qm9x8":
            b = synth.random_batch(8, "qm9", d_v=d_v, d_e=d_e)
        elif name == "mixed":
            mols = [synth.random_molgraph(rng, d_v=d_v, d_e=d_e, n_atoms=1)] + [synth.random_molgraph(rng, 9.0, d_v, d_e) for _ in range(6)]
            mols.insert(3, synth.random_molgraph(rng, d_v=d_v, d_e=d_e, n_atoms=40))
            b = BatchMolGraph(mols)
        elif name == "empty":
            b = BatchMolGraph([synth.random_molgraph(rng, d_v=d_v, d_e=d_e, n_atoms=1) for _ in range(3)])
        elif name == "dense":
            b = synth.random_batch(4, "synth40", d_v=d_v, d_e=d_e)
        elif name.startswith("chain"):
            n, m = (int(x) for x in name[5:].split("x"))
            b = BatchMolGraph([synth.chain_molgraph(n, d_v, d_e)] * m)
        else:
            raise KeyError(name)
        _batches[key] = b
    return _batches[key].__copy__()


def make_plan(bmg, kind: str, oversize="batch"):
    """A plan object without K0: full, ``tiles`` (``light="tiles"``) or ``light`` — ``GraphPlan(launch=False)`` refuses that kind (it
    is no training plan), so a full one is marked the way the constructor marks a light plan: ``plan.buf`` keeps a full plan's size
    and header, and the ``light`` rows pin only the branches that read the ``light`` / ``tiles_only`` marks."""
    if kind == "light":
        plan = engine.GraphPlan.from_bmg(bmg, launch=False)
        plan.light = engine.small_plan_fits(plan.n_atoms, plan.n_edges)
    else:
        plan = engine.GraphPlan.from_bmg(bmg, light="tiles" if kind == "tiles" else False, launch=False)
    plan.oversize = bmg.oversize if oversize == "batch" else oversize
    return plan


# ---- signatures ----------------------------------------------------------------------------------------------------------------------
def _extent(t) -> int:
    if t.numel() == 0:
        return 0
    return (sum((n - 1) * s for n, s in zip(t.shape, t.stride())) + 1) * t.element_size()


def _where(p, named):
    """``name`` or ``name+byte offset`` of the first tensor of ``named`` that ``p`` points into (``None``: a null pointer)."""
    if not p:
        return None
    for name, t in named:
        if t is None:
            continue
        base = t.data_ptr()
        if base and base <= p < base + max(_extent(t), 1):
            return name if p == base else f"{name}+{p - base}"
    raise AssertionError(f"a pointer into no tensor of the call ({[n for n, t in named if t is not None]})")


def struct_sig(a, named, skip=()) -> dict:
    """Every field of a ctypes argument block that is not zero / null; pointers by name and offset."""
    sig = {}
    for n, t in a._fields_:
        if n in skip:
            continue
        v = getattr(a, n)
        if t is C.c_void_p:
            v = _where(v, named)
        if v:
            sig[n] = v
    return sig


def _shape(t):
    return None if t is None else list(t.shape)


def state_sig(st, named) -> dict:
    named = list(named) + [(f"refs[{i}]", t) for i, t in enumerate(st.refs)]
    return dict(route=st.route, fused=bool(st.fused), dims=st.dims, ldh=st.ldh, n_hslots=st.n_hslots, n_mslots=st.n_mslots,
                shapes={k: _shape(getattr(st, k)) for k in ("H0", "Hs", "Ms", "Mv", "Hv") if getattr(st, k) is not None},
                args=struct_sig(st.args, named),
                n_refs=len(st.refs), refs={str(i): f"{list(t.shape)} {str(t.dtype)[6:]}" for i, t in enumerate(st.refs) if t is not None})


def backward_sig(st, named) -> dict:
    d = st.dims
    gout = torch.zeros(int(st.args.n_atoms), d["d_h"] + d["d_vd"])
    grads, b, (ws, gout) = engine.backward(st, gout, dict.fromkeys(("W_i", "b_i", "W_h", "b_h", "W_o", "b_o", "W_d", "b_d"), True), launch=False)
    named = list(named) + [("gout", gout), ("ws", ws)] + [("g" + k, g) for k, g in grads.items()]
    return dict(args=struct_sig(b, named, skip=("f",)), same_f=bytes(b.f) == bytes(st.args), ws=list(ws.shape),
                grads={k: _shape(g) for k, g in grads.items() if g is not None})


def refusal(e: BaseException) -> dict:
    return {"raises": type(e).__name__, "message": str(e)}


# ---- forward rows --------------------------------------------------------------------------------------------------------------------
def _weights(d_v, d_e, d_h, bias, atom_w, vd):
    z = torch.zeros
    w = dict(W_i=z(d_h, d_v if atom_w else d_v + d_e), W_h=z(d_h, d_h + d_e if atom_w else d_h), W_o=z(d_h, d_v + d_h), b_o=z(d_h))
    if bias:
        w.update(b_i=z(d_h), b_h=z(d_h))
    if vd:
        w.update(W_d=z(d_h + vd, d_h + vd), b_d=z(d_h + vd))
    return w


def forward_call(s: dict):
    """The call of spec ``s``: returns ``(out, st, named)``.  ``s``: ``b`` batch, ``dv`` / ``de`` / ``h`` widths, ``plan`` kind, ``bias``,
    ``vd`` (``d_vd``), ``oversize`` (the plan's; default the batch's), ``kw`` the demands of ``engine.forward``, ``out`` (``slice`` /
    ``misaligned``), ``atom_w`` (weights of an atom block; default ``kw["atom"]``), ``trim`` (V one row short), ``wcache``."""
    kw = dict(s.get("kw", {}))
    d_v, d_e, d_h, vd = s.get("dv", 72), s.get("de", 14), s.get("h", 32), s.get("vd", 0)
    bmg = batch(s.get("b", "qm9x8"), d_v, d_e)
    plan = make_plan(bmg, s.get("plan", "full"), s.get("oversize", "batch"))
    nV = int(bmg.V.shape[0])
    w = _weights(d_v, d_e, d_h, s.get("bias", False), s.get("atom_w", bool(kw.get("atom"))), vd)
    V = bmg.V[:-1] if s.get("trim") else bmg.V
    named = [("V", V), ("E", bmg.E), ("plan.buf", plan.buf), ("plan.edge_index", plan.edge_index), ("plan.rev_edge_index", plan.rev_edge_index)]
    if vd:
        kw["V_d"] = torch.zeros(nV, vd)
        named.append(("V_d", kw["V_d"]))
    if s.get("out") == "slice":      # the rows of a bigger buffer, as a multicomponent step hands them out
        kw["out"] = torch.zeros(nV + 5, d_h + vd)[2:2 + nV]
    elif s.get("out") == "misaligned":
        kw["out"] = torch.zeros(nV, d_h + vd + 1)[:, 1:]
    if "dropout" in kw:
        kw["dropout"] = tuple(kw["dropout"])
    named += list(w.items())
    if "wcache" in s:
        kw["wcache"] = s["wcache"]
    out, st = engine.forward(plan, V, bmg.E, w["W_i"], w["W_h"], w["W_o"], w["b_o"], w.get("b_i"), w.get("b_h"), w.get("W_d"), w.get("b_d"),
                             launch=False, **kw)
    return out, st, named + [("out", out)]


def forward_row(s: dict) -> dict:
    with environment(s.get("env", {})):
        try:
            if s.get("wcache_case"):
                return wcache_row(s)
            out, st, named = forward_call(s)
        except Exception as e:   # (the row IS the refusal)
            return refusal(e)
        row = state_sig(st, named)
        row["out"] = f"{list(out.shape)} stride {list(out.stride())}"
        if s.get("kw", {}).get("keep"):
            row["backward"] = backward_sig(st, named)
        return row


def wcache_row(s: dict) -> dict:
    """``wcache``: a second inference call takes the buffer of the first; a kept call in between takes one of its own."""
    wc: dict = {}
    base = {k: v for k, v in s.items() if k != "wcache_case"}
    _, st1, _ = forward_call(dict(base, wcache=wc))
    buf1 = wc.get("buf")
    _, stk, named = forward_call(dict(base, wcache=wc, kw=dict(base.get("kw", {}), keep=True)))
    _, st2, _ = forward_call(dict(base, wcache=wc))
    return dict(state_sig(stk, named), first_is_cached=st1.refs[-1] is buf1, kept_has_its_own=stk.refs[-1] is not buf1 and wc.get("buf") is buf1,
                second_same_object=st2.refs[-1] is buf1)


# ---- step rows -----------------------------------------------------------------------------------------------------------------------
def make_trainer(s: dict):
    """The model and ``FusedTrainer`` of a step spec: ``block`` (constructor arguments of the block; ``atom``: an atom block), ``tr``
    (the trainer's switches), ``multi`` (``"shared"`` / ``"each"``), ``p_after`` (``dropout.p`` raised after construction).  A step spec's
    ``odd_stride`` hands the step ``V`` as the columns of a matrix one column wider (rows of an odd stride)."""
    from chemprop_amd import agg as cagg
    from chemprop_amd.model import MPNN, FusedTrainer, MulticomponentMPNN, RegressionFFN
    from chemprop_amd.nn import AtomMessagePassing, BondMessagePassing, MulticomponentMessagePassing

    torch.manual_seed(5)
    blk = dict(d_v=s.get("dv", 72), d_e=s.get("de", 14), d_h=s.get("h", 32))
    blk.update(s.get("block", {}))
    cls = AtomMessagePassing if s.get("atom") else BondMessagePassing
    if s.get("multi"):
        mp = MulticomponentMessagePassing([cls(**blk) for _ in range(1 if s["multi"] == "shared" else 2)], 2, shared=s["multi"] == "shared")
        model = MulticomponentMPNN(mp, cagg.SumAggregation(), RegressionFFN(1, mp.output_dim, 16))
    else:
        mp = cls(**blk)
        model = MPNN(mp, cagg.SumAggregation(), RegressionFFN(1, mp.output_dim, 16))
    model.train()
    tr = FusedTrainer(model, **s.get("tr", {}))
    if "p_after" in s:
        for b in tr.blocks:
            b.dropout.p = s["p_after"]
    return model, tr


def _draws(before, after) -> int:
    torch.set_rng_state(before)
    for n in range(3):
        if torch.equal(torch.get_rng_state(), after):
            return n
        torch.randint(0, 2 ** 62, (1,), dtype=torch.int64)
    return -1


def step_row(s: dict) -> dict:
    with environment(dict(s.get("env", {}), DMPNN_VALIDATE="never")):
        model, tr = make_trainer(s)
        names = s.get("bs") or [s.get("b", "qm9x8")]
        bmgs = [batch(n, s.get("dv", 72), s.get("de", 14)) for n in names]
        for b in bmgs:
            if "oversize" in s:
                b.oversize = s["oversize"]
            if s.get("odd_stride"):
                ov = b.oversize
                b.V = torch.cat((b.V, b.V[:, :1]), 1)[:, :-1]
                b.oversize = ov
        V_d = torch.zeros(int(bmgs[0].V.shape[0]), s["block"]["d_vd"]) if s.get("block", {}).get("d_vd") else None
        torch.manual_seed(77)
        before = torch.get_rng_state()
        try:
            comps, blocks, n_mols = tr._components(bmgs if s.get("multi") else bmgs[0], None)
            Vd = tr._atom_descriptors(V_d, comps[0])
            parts, out, gout, vd, vd_keep = tr._blocks(comps, blocks, False, Vd)
        except Exception as e:
            row = refusal(e)
            row["draws"] = _draws(before, torch.get_rng_state())
            return row
        row = dict(draws=_draws(before, torch.get_rng_state()), last_route=tr.last_route, out=_shape(out), gout=_shape(gout), parts=[])
        for part, mp in zip(parts, blocks):
            cb, plan, st = part.bmg, part.plan, part.st
            named = [("V", cb.V), ("E", cb.E), ("plan.buf", plan.buf), ("plan.edge_index", plan.edge_index), ("plan.rev_edge_index", plan.rev_edge_index)]
            named += [(k, getattr(getattr(mp, lin), n)) for k, (lin, n) in dict(W_i=("W_i", "weight"), b_i=("W_i", "bias"), W_h=("W_h", "weight"),
                                                                               b_h=("W_h", "bias"), W_o=("W_o", "weight"), b_o=("W_o", "bias")).items()]
            named += [("out", part.out), ("gout", part.gout), ("ws", part.keep_b[0]), ("flat grads", tr.sync.flat)]
            row["parts"].append(dict(route=part.route, tiles_only=bool(plan.tiles_only), light=plan.light, any_size=bool(plan.any_size),
                                     oversize=plan.oversize, plan_bytes=part.plan_bytes, drop=None if part.drop is None else list(part.drop),
                                     st=state_sig(st, named), bwd=struct_sig(part.bwd, named, skip=("f",)), same_f=bytes(part.bwd.f) == bytes(st.args)))
        if vd is not None:
            row["vd"] = dict(d_vd=int(vd.d_vd), dropout_p=float(vd.dropout_p), dropout_seed=int(vd.dropout_seed), ws_bytes=int(vd.ws_bytes))
        return row


# ---- the rows ------------------------------------------------------------------------------------------------------------------------
F_H0_RESIDUAL, F_ROW_FINALIZE = _lib.F_H0_RESIDUAL, _lib.F_ROW_FINALIZE


def forward_specs() -> dict:
    R: dict = {}

    def add(name, **s):
        assert name not in R, name
        R[name] = s

    # the default rule over widths x plans x keeping, on the headline batch and on the one with a molecule beyond the tile
    for h in (4, 30, 32, 300, 324, 644):
        for plan in ("full", "light", "tiles") if h in (30, 32, 644) else ("full",):
            for keep in (False, True):
                add(f"rule/qm9x8/h{h}/{plan}/keep{int(keep)}", h=h, plan=plan, kw=dict(keep=keep))
        for keep in (False, True):
            if h in (32, 324):
                add(f"rule/mixed/h{h}/full/keep{int(keep)}", b="mixed", h=h, kw=dict(keep=keep))
            if h == 32:
                add(f"rule/qm9x8/h{h}/full/keep{int(keep)}/level1", h=h, kw=dict(keep=keep, max_level=1))
                add(f"rule/qm9x8/h{h}/full/keep{int(keep)}/level0", h=h, kw=dict(keep=keep, max_level=0))
    # demands
    for h in (4, 324):
        for keep in (False, True):
            add(f"route=fused16/h{h}/keep{int(keep)}", h=h, kw=dict(route="fused16", keep=keep))
        add(f"route=general/mfma=split16/h{h}/keep1", h=h, kw=dict(route="general", mfma="split16", keep=True))
        add(f"route=mega/h{h}", h=h, kw=dict(route="mega"))
    for h in (30, 32):
        for route in ("general", "fused", "mega", "fused16"):
            for keep in (False, True):
                add(f"route={route}/h{h}/keep{int(keep)}", h=h, kw=dict(route=route, keep=keep))
        for fused in (True, False):
            add(f"fused={fused}/h{h}", h=h, kw=dict(fused=fused))
        for mfma in ("f32", "split16"):
            for keep in ((False, True) if h == 32 else (True,)):
                add(f"mfma={mfma}/h{h}/keep{int(keep)}", h=h, kw=dict(mfma=mfma, keep=keep))
            add(f"route=general/mfma={mfma}/h{h}/keep1", h=h, kw=dict(route="general", mfma=mfma, keep=True))
    for plan in ("light", "tiles"):
        for route in ("general", "fused", "mega", "fused16"):
            for keep in (False, True):
                add(f"route={route}/h32/{plan}/keep{int(keep)}", plan=plan, kw=dict(route=route, keep=keep))
        add(f"mfma=f32/h32/{plan}", plan=plan, kw=dict(mfma="f32"))
        add(f"mfma=split16/h32/{plan}/keep1", plan=plan, kw=dict(mfma="split16", keep=True))
    add("mfma=split16/level1", kw=dict(mfma="split16", max_level=1))
    add("mfma=split16/level0/keep1", kw=dict(mfma="split16", max_level=0, keep=True))
    add("fused=True/level0", kw=dict(fused=True, max_level=0))
    add("route=mega/level0", kw=dict(route="mega", max_level=0))
    add("route=fused16/mfma=f32", kw=dict(route="fused16", mfma="f32"))
    add("route=fused16/undirected", kw=dict(route="fused16", undirected=True))
    for keep_bits in (True, False):
        for act in ("relu", "tanh"):
            add(f"route=fused16/keep1/bits{int(keep_bits)}/{act}", kw=dict(route="fused16", keep=True, keep_bits=keep_bits, act=act))
        add(f"rule/tiles/keep1/bits{int(keep_bits)}/depth4", plan="tiles", kw=dict(keep=True, keep_bits=keep_bits, depth=4))
    add("rule/tiles/keep1/tanh", plan="tiles", kw=dict(keep=True, act="tanh"))
    add("route=fused16/keep1/depth1", kw=dict(route="fused16", keep=True, depth=1))
    for form in (F_H0_RESIDUAL, F_ROW_FINALIZE, F_H0_RESIDUAL | F_ROW_FINALIZE):
        add(f"route=fused16/form{form}", kw=dict(route="fused16", form=form))
        add(f"route=fused16/h324/form{form}", h=324, kw=dict(route="fused16", form=form))
        add(f"rule/form{form}", kw=dict(form=form))
    for depth in (1, 2, 5):
        for keep in (False, True):
            add(f"rule/depth{depth}/keep{int(keep)}", kw=dict(depth=depth, keep=keep))
            if depth != 2:
                add(f"mfma=f32/fused/depth{depth}/keep{int(keep)}", kw=dict(mfma="f32", max_level=1, depth=depth, keep=keep))
    add("rule/bias/leakyrelu", bias=True, kw=dict(act="leakyrelu", slope=0.01, keep=True))
    # batches: no edges, the crossovers of the rule (2 048 and 20 000 directed edges, and 16 edges below each), dense molecules, odd widths
    for b in ("empty", "chain9x127", "chain9x128", "chain9x256", "chain9x1249", "chain9x1250", "dense"):
        for keep in (False, True):
            add(f"rule/{b}/keep{int(keep)}", b=b, kw=dict(keep=keep))
        add(f"route=general/{b}", b=b, kw=dict(route="general"))
        if b in ("chain9x127", "chain9x128", "dense"):
            add(f"rule/{b}/level1", b=b, kw=dict(max_level=1))
        add(f"rule/{b}/tiles", b=b, plan="tiles")
    add("rule/chain9x256/tiles/keep1", b="chain9x256", plan="tiles", kw=dict(keep=True))
    add("rule/chain9x1250/tiles/keep1", b="chain9x1250", plan="tiles", kw=dict(keep=True))
    add("route=fused16/chain9x1250/keep1", b="chain9x1250", kw=dict(route="fused16", keep=True))
    add("route=fused16/empty", b="empty", kw=dict(route="fused16"))
    for dv, de in ((71, 14), (72, 13)):
        for keep in (False, True):
            add(f"rule/dv{dv}de{de}/keep{int(keep)}", dv=dv, de=de, kw=dict(keep=keep))
        add(f"route=fused/dv{dv}de{de}", dv=dv, de=de, kw=dict(route="fused"))
        add(f"mfma=split16/dv{dv}de{de}/keep1", dv=dv, de=de, kw=dict(mfma="split16", keep=True))
    # what the host knows about molecules beyond the tile: the inference tile kernel's spill scratch
    for ov in (None, False, True):
        add(f"rule/tiles/oversize={ov}", plan="tiles", oversize=ov)
        add(f"rule/full/oversize={ov}", oversize=ov)
    # semantics: atom messages, undirected, dropout, W_d
    for de in (1, 14, 17):
        for keep in (False, True):
            add(f"atom/de{de}/keep{int(keep)}", de=de, kw=dict(atom=True, keep=keep))
            add(f"atom/de{de}/general/keep{int(keep)}", de=de, kw=dict(atom=True, route="general", mfma="split16", keep=keep))
    add("atom/tiles/keep1", plan="tiles", kw=dict(atom=True, keep=True))
    add("atom/tiles/keep0", plan="tiles", kw=dict(atom=True))
    add("atom/fused=False/mfma=f32", kw=dict(atom=True, fused=False, mfma="f32"))
    add("atom/env-general-is-no-demand", env=dict(DMPNN_GENERAL="1"), kw=dict(atom=True))
    add("atom/general/undirected", kw=dict(atom=True, route="general", undirected=True))
    add("atom/W_d", vd=5, kw=dict(atom=True))
    add("atom/h30/keep1", h=30, kw=dict(atom=True, keep=True))
    add("atom/h30/general/keep1", h=30, kw=dict(atom=True, route="general", keep=True))
    add("atom/bond-weights", atom_w=False, kw=dict(atom=True))
    add("atom/general/dropout", kw=dict(atom=True, route="general", mfma="split16", keep=True, dropout=(0.25, 99)))
    add("atom/general/dropout/de1", de=1, kw=dict(atom=True, route="general", mfma="split16", keep=True, dropout=(0.25, 99)))
    add("atom/dropout/tile", kw=dict(atom=True, keep=True, dropout=(0.25, 99)))
    for keep in (False, True):
        add(f"undirected/keep{int(keep)}", kw=dict(undirected=True, keep=keep))
        add(f"undirected/h324/keep{int(keep)}", h=324, kw=dict(undirected=True, keep=keep))
    add("undirected/route=fused", kw=dict(undirected=True, route="fused"))
    add("undirected/light", plan="light", kw=dict(undirected=True))
    for ud in (False, True):
        add(f"undirected/dropout/mask{int(ud)}", kw=dict(undirected=True, route="general", mfma="split16", keep=True, dropout=(0.1, 7), undirected_dropout=ud))
    for act in ("relu", "tanh"):
        for p in (0.0, 0.25, 1.0):
            add(f"dropout/{act}/p{p}/tile", plan="tiles", kw=dict(keep=True, act=act, dropout=(p, 2 ** 63 + 5)))
            add(f"dropout/{act}/p{p}/lean", b="mixed", kw=dict(keep=True, act=act, route="fused16", dropout=(p, 12345)))
            add(f"dropout/{act}/p{p}/rows", b="mixed", kw=dict(keep=True, act=act, route="general", mfma="split16", dropout=(p, -3)))
    add("dropout/inference", kw=dict(dropout=(0.25, 1)))
    add("dropout/rule-lean-is-no-demand", b="mixed", kw=dict(keep=True, max_level=1, dropout=(0.25, 1)))
    add("dropout/lean/bits0", b="mixed", kw=dict(keep=True, keep_bits=False, route="fused16", dropout=(0.25, 1)))
    add("dropout/lean/depth1", b="mixed", kw=dict(keep=True, depth=1, route="fused16", dropout=(0.25, 1)))
    add("dropout/rows/mfma=None", b="mixed", kw=dict(keep=True, route="general", dropout=(0.25, 1)))
    add("dropout/rows/h31", b="mixed", h=31, kw=dict(keep=True, route="general", mfma="split16", dropout=(0.25, 1)))
    add("dropout/rows/dv71", b="mixed", dv=71, kw=dict(keep=True, route="general", mfma="split16", dropout=(0.25, 1)))
    add("dropout/rows/W_d", b="mixed", vd=5, kw=dict(keep=True, route="general", mfma="split16", dropout=(0.25, 1)))
    add("dropout/tile/W_d", vd=5, kw=dict(keep=True, dropout=(0.25, 1)))
    for plan in ("full", "light", "tiles"):
        for keep in (False, True):
            add(f"W_d/{plan}/keep{int(keep)}", plan=plan, vd=5, kw=dict(keep=keep))
    add("W_d/general/keep1", vd=5, kw=dict(route="general", keep=True))
    add("W_d/fused16", vd=5, kw=dict(route="fused16"))
    add("W_d/h30", h=30, vd=3, kw=dict(keep=True))
    # buffers
    add("out/slice", out="slice", kw=dict(keep=True))
    add("out/slice/W_d", out="slice", vd=4)
    add("out/slice/h30", h=30, out="slice")
    add("out/misaligned", out="misaligned")
    add("plan/other-batch", trim=True)
    add("wcache/mega16", wcache_case=True)
    add("wcache/general16", wcache_case=True, kw=dict(route="general", mfma="split16"))
    # environment switches
    for env in (dict(DMPNN_GENERAL="1"), dict(DMPNN_MEGA="0"), dict(DMPNN_MFMA="f32"), dict(DMPNN_H0="x"), dict(DMPNN_STORE="f16")):
        tag = "/".join(f"{k}={v}" for k, v in env.items())
        for keep in (False, True):
            add(f"env/{tag}/rule/keep{int(keep)}", env=env, kw=dict(keep=keep))
            if not keep or "DMPNN_MFMA" in env:
                add(f"env/{tag}/route=fused16/keep{int(keep)}", env=env, kw=dict(route="fused16", keep=keep))
        add(f"env/{tag}/route=mega", env=env, kw=dict(route="mega"))
        add(f"env/{tag}/fused=True", env=env, kw=dict(fused=True))
        add(f"env/{tag}/tiles", env=env, plan="tiles")
        add(f"env/{tag}/route=fused16/h324", env=env, h=324, kw=dict(route="fused16"))
    return R


def step_specs() -> dict:
    R: dict = {}

    def add(name, **s):
        assert name not in R, name
        R[name] = s

    RD = dict(rows_dropout=True)
    # bond blocks
    for b in ("qm9x8", "mixed", "dense", "empty", "chain9x256", "chain9x1250"):
        add(f"bond/p0/{b}", b=b)
    add("bond/p0/h30", h=30)
    add("bond/p0/h324", h=324)
    add("bond/p0/dv71", dv=71)
    add("bond/p0/tile_plan=False", tr=dict(tile_plan=False))
    add("bond/p0/env-mega0", env=dict(DMPNN_MEGA="0"))
    add("bond/p0/env-general", env=dict(DMPNN_GENERAL="1"))
    add("bond/p0/env-train-plan-full", env=dict(DMPNN_TRAIN_PLAN="full"))
    add("bond/p>0/tile", block=dict(dropout=0.2))
    add("bond/p>0/tile/tile_plan=False", block=dict(dropout=0.2), tr=dict(tile_plan=False))
    add("bond/p>0/lean/oversize", b="mixed", block=dict(dropout=0.2))
    add("bond/p>0/lean/dense", b="dense", block=dict(dropout=0.2))
    add("bond/p>0/lean-before-rows", b="mixed", block=dict(dropout=0.2), tr=RD)
    add("bond/p>0/lean-then-rows/h324", b="mixed", h=324, block=dict(dropout=0.2), tr=RD)
    add("bond/p>0/rows/tanh", block=dict(dropout=0.2, activation="tanh"), tr=RD)
    add("bond/p>0/rows/tanh/oversize", b="mixed", block=dict(dropout=0.2, activation="tanh"), tr=RD)
    add("bond/p>0/refused/no-rows_dropout", b="mixed", h=324, block=dict(dropout=0.2))
    add("bond/p>0/rows/h30", b="mixed", h=30, block=dict(dropout=0.2), tr=RD)
    add("bond/p>0/refused/shape/rows_dropout", b="mixed", h=31, block=dict(dropout=0.2), tr=RD)
    add("bond/p>0/refused/dv71/rows_dropout", dv=71, block=dict(dropout=0.2), tr=RD)
    add("bond/p>0/refused/tile/dv71", dv=71, block=dict(dropout=0.2))
    add("bond/p>0/refused/tanh-raised-after", block=dict(activation="tanh"), p_after=0.2)
    add("bond/p>0/refused/p=1", b="mixed", block=dict(dropout=0.2), p_after=1.0, tr=RD)
    add("bond/p>0/env-mfma-f32", b="mixed", block=dict(dropout=0.2), env=dict(DMPNN_MFMA="f32"))
    add("bond/p>0/env-mfma-f32/rows_dropout", b="mixed", block=dict(dropout=0.2), env=dict(DMPNN_MFMA="f32"), tr=RD)
    add("bond/p>0/odd-stride/rows_dropout", b="mixed", odd_stride=True, block=dict(dropout=0.2, activation="tanh"), tr=RD)
    add("bond/p>0/env-mega0", block=dict(dropout=0.2), env=dict(DMPNN_MEGA="0"))
    # undirected blocks
    UN = dict(undirected=True)
    add("undirected/p0", block=dict(undirected=True), tr=UN)
    add("undirected/p0/h324", h=324, block=dict(undirected=True), tr=UN)
    add("undirected/p>0/taken", block=dict(undirected=True, dropout=0.2), tr=dict(undirected=True, rows_dropout=True))
    add("undirected/p>0/refused/raised-after", block=dict(undirected=True), p_after=0.2, tr=UN)
    add("undirected/p>0/refused/shape", h=31, block=dict(undirected=True, dropout=0.2), tr=dict(undirected=True, rows_dropout=True))
    add("undirected/p>0/refused/p=1", block=dict(undirected=True, dropout=0.2), p_after=1.0, tr=dict(undirected=True, rows_dropout=True))
    add("undirected/p>0/refused/odd-stride", odd_stride=True, block=dict(undirected=True, dropout=0.2), tr=dict(undirected=True, rows_dropout=True))
    # atom blocks
    AT = dict(atom_messages=True)
    add("atom/p0/tile", atom=True, tr=AT)
    add("atom/p0/tile/tile_plan=False", atom=True, tr=dict(atom_messages=True, tile_plan=False))
    add("atom/p0/tile_plan=False/beyond-small-plan", atom=True, b="chain9x1250", tr=dict(atom_messages=True, tile_plan=False))
    add("atom/p0/chain9x1250", atom=True, b="chain9x1250", tr=AT)
    add("atom/p0/oversize", atom=True, b="mixed", tr=AT)
    add("atom/p0/dense", atom=True, b="dense", tr=AT)
    add("atom/p0/empty", atom=True, b="empty", tr=AT)
    add("atom/p0/de13", atom=True, de=13, tr=AT)
    add("atom/p0/de1", atom=True, de=1, tr=AT)
    add("atom/p0/h30", atom=True, h=30, tr=AT)
    add("atom/p0/h31", atom=True, h=31, tr=AT)
    add("atom/p0/h324", atom=True, h=324, tr=AT)
    add("atom/p0/env-mega0", atom=True, tr=AT, env=dict(DMPNN_MEGA="0"))
    add("atom/p0/env-mfma-f32", atom=True, tr=AT, env=dict(DMPNN_MFMA="f32"))
    add("atom/p>0/taken", atom=True, block=dict(dropout=0.2), tr=dict(atom_messages=True, rows_dropout=True))
    add("atom/p>0/taken/oversize", atom=True, b="mixed", block=dict(dropout=0.2), tr=dict(atom_messages=True, rows_dropout=True))
    add("atom/p>0/refused/raised-after", atom=True, p_after=0.2, tr=AT)
    add("atom/p>0/refused/de13", atom=True, de=13, block=dict(dropout=0.2), tr=dict(atom_messages=True, rows_dropout=True))
    add("atom/p>0/refused/p=1", atom=True, block=dict(dropout=0.2), p_after=1.0, tr=dict(atom_messages=True, rows_dropout=True))
    add("atom/p>0/refused/odd-stride", atom=True, odd_stride=True, block=dict(dropout=0.2), tr=dict(atom_messages=True, rows_dropout=True))
    add("atom/refused/features", atom=True, block=dict(d_e=12), tr=AT)
    # W_d behind the block
    add("W_d/p0", block=dict(d_vd=5))
    add("W_d/p>0/vd_dropout", block=dict(d_vd=5, dropout=0.2), tr=dict(vd_dropout=True))
    add("W_d/p>0/refused/raised-after", block=dict(d_vd=5), p_after=0.2)
    # multicomponent
    add("multi/shared", multi="shared", bs=["qm9x8", "qm9x8"])
    add("multi/each", multi="each", bs=["qm9x8", "qm9x8"])
    add("multi/each/h30/misaligned-rows", multi="each", h=30, bs=["qm9x8", "qm9x8"])
    return R


def _flat(d: dict, pre=""):
    for k, v in d.items():
        if isinstance(v, dict):
            yield from _flat(v, f"{pre}{k}.")
        else:
            yield pre + k, v


def _delta(sig: dict, base: dict) -> dict:
    """The fields of the flat signature ``sig`` that differ from ``base``'s (one that ``base`` has and ``sig`` lacks: ``None``)."""
    return {k: sig.get(k) for k in sig.keys() | base.keys() if sig.get(k) != base.get(k)}


def build_rows() -> dict:
    """Every row, by name.  ``engine._require_device`` must already be a no-op.  The first signature of a kind (a forward row, a part of a
    step row) stands in full; every later one is written by dotted key as what differs from the EARLIER signature nearest to it,
    named under ``like`` — the two together are the full signature, and the file stays small enough to read.  A refusal stands as it is."""
    def compact(full, name, sig):
        if "raises" in sig:
            return sig
        sig = dict(_flat(sig))
        like = min(full, key=lambda n: len(_delta(sig, full[n])), default=None)
        full[name] = sig
        return sig if like is None else dict(_delta(sig, full[like]), like=like)

    calls, parts = {}, {}     # the flat signatures so far: forward rows lean on forward rows, parts on parts
    with torch.random.fork_rng(devices=[]):   # (the step rows seed torch's CPU generator: leave it as it was)
        rows = {"forward/" + k: compact(calls, k, forward_row(s)) for k, s in forward_specs().items()}
        for k, s in step_specs().items():
            row = rows["step/" + k] = step_row(s)
            if "parts" in row:
                row["parts"] = [compact(parts, f"{k}#{i}", p) for i, p in enumerate(row["parts"])]
    return rows


def expand(rows: dict, name: str):
    """The full signature of row ``name`` of a compact table (a test's failure report): every ``like`` followed to the row in full
    (a field that is ``None`` is left out)."""
    def full(pool, sig):
        if "like" not in sig:
            return sig
        base = dict(full(pool, pool[sig["like"]]))
        base.update({k: v for k, v in sig.items() if k != "like"})
        return {k: v for k, v in base.items() if v is not None}

    row = rows[name]
    if name.startswith("forward/"):
        return full({k[8:]: v for k, v in rows.items() if k.startswith("forward/")}, row)
    pool = {f"{k[5:]}#{i}": p for k, v in rows.items() if k.startswith("step/") for i, p in enumerate(v.get("parts", ()))}
    return dict(row, parts=[full(pool, p) for p in row["parts"]]) if "parts" in row else row


def dumps(rows: dict) -> str:
    """One row per line, so that a change reads as a diff of the rows it touches."""
    import json

    return "{\n" + ",\n".join(f"{json.dumps(k)}: {json.dumps(v, sort_keys=True, separators=(',', ':'))}" for k, v in rows.items()) + "\n}\n"
