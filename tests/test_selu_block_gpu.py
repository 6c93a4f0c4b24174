"""A SELU block (``DMPNN_ACT_SELU``) on every route ELU takes — forward, every parameter gradient and, where the route has them, the
input gradients — against ``F.selu`` in float64: the smallest ELU cases of the existing sweeps with the activation replaced.

* tile kernels (``route="mega"``): bond messages through the contract of ``tests/test_tile_boundaries.py`` (``_hold``: training on the
  full and on the tile plan, two backward passes bit for bit, no sign bits, the inference forward), atom messages through
  ``tile_harness.run_tile(atom=True)`` against ``oracle.dmpnn_torch.atom_forward``;
* the per-step fused route on the f16 pipe, not lean (``route="fused16"``: a smooth activation keeps fp32 rows), training and inference;
* the per-step general route, fp32 and on the f16 pipe (``general`` / ``general16``): directed, undirected, with ``W_d``, with the
  gradients w.r.t. ``V``, ``E`` and ``V_d`` (``dmpnn_backward_inputs``); and with ``p = 0.25`` under a fixed seed, the masks rebuilt
  from ``dmpnn_dropout_keep`` and replayed in the reference, directed and undirected (``DMPNN_F_UNDIRECTED_MASK``);
* the mol-atom-bond blocks on the tile route, both read-outs, bond and atom messages;
* one block on two routes, tile and ``general16``: their outputs to each other at the suite's ``TOL``.

The harnesses' references call ``oracle.dmpnn_torch.activation_fn`` by module attribute: this file adds ``"selu"`` to it and to
``lean_harness.ENGINE_ACT`` at run time (``monkeypatch``), and records every pre-activation the reference forms.  Every case asserts
on those float64 pre-activations, before it runs anything on the device: at every site at least a quarter negative and a quarter
positive; over the case one below -5 and one exactly 0.  The sweeps' stock inputs (unit features) reach neither: ``V`` and ``E`` are
scaled by 4 and row ``C0`` of ``W_i`` (and of ``b_i``) is zeroed — column ``C0`` of ``H0`` is then exactly 0 on every edge, with
non-zero inputs behind it, so ``tau'(0) = lambda alpha`` (and not ``lambda``) decides row ``C0`` of ``gW_i`` and ``gb_i``.

Judged by the suite's rule and its one number: ``err = max|got - ref| / max|ref|`` within ``min(rows_harness.MARGIN max(e32, 2**-23),
cap)``, ``e32`` the float32 restatement's error; one ``...BAR`` line per tensor printed before judging.  The from-output gradient
``y + lambda alpha`` cancels at very negative ``z`` (ELU's ``y + 1`` again): the factor there is below ``2**-23 lambda alpha`` in
absolute terms, which the max-norm rule does not see.

Measured on the MI355X (209 comparisons): the worst ``err / max(e32, 2**-23)`` is 2.57 — ``gW_i`` of ``h36-atom-selu-nobias@full`` (err
7.0e-7 against a float32 draw of 2.7e-7) — then 2.32 (``gb_o``, ``h36-atom-selu-bias@tiles``), 2.08 (``gb_o``, ``h132-fused16-selu`` on the per-step
fused route) and 1.92 (``gW_h``, ``h36-act-selu-nobias``): the figures of the ELU / tanh cases these were made from, far below the shared margin
of 16.  The tile route and ``general16`` differ by 1.7e-7 in the output (bar ``TOL`` = 1e-5)."""
import functools

import pytest
import torch
import torch.nn.functional as F

import atom_harness as ah
import lean_harness as lh
import rows_harness as rh
import test_input_grad_gpu as ig
import test_tile_boundaries as tb
import tile_harness as th
from conftest import TOL, parity_err
from lean_harness import Case
from oracle import dmpnn_torch as ot

pytestmark = pytest.mark.gpu

SCALE, C0 = 4.0, 1
PRE = []   # every pre-activation the references form, in order (cleared by the case that reads it)


def _selu(z):
    PRE.append(z.detach())
    return F.selu(z)


_ORIG_ACT, _ORIG_INPUTS = ot.activation_fn, lh.inputs


def _activation_fn(name, w=None):
    return _selu if str(name).lower() == "selu" else _ORIG_ACT(name, w)


def _shape_inputs(inp):
    """The stock operands of a case made to meet the condition (see the module docstring); a copy."""
    inp = {k: (None if v is None else v.clone()) for k, v in inp.items()}
    inp["V"] *= SCALE
    inp["E"] *= SCALE
    inp["W_i"][C0] = 0.0
    if inp.get("b_i") is not None:
        inp["b_i"][C0] = 0.0
    return inp


@functools.lru_cache(maxsize=None)
def _bond_inputs(case):
    return _shape_inputs(_ORIG_INPUTS(case)) if case.act == "selu" else _ORIG_INPUTS(case)


@pytest.fixture(autouse=True)
def _selu_in_the_harnesses(monkeypatch):
    monkeypatch.setattr(ot, "activation_fn", _activation_fn)
    monkeypatch.setitem(lh.ENGINE_ACT, "selu", ("selu", 0.0))
    monkeypatch.setattr(lh, "inputs", _bond_inputs)
    del PRE[:]


def condition(pre, case_id):
    """On the float64 pre-activations of a case (site by site)."""
    assert pre, case_id
    for i, z in enumerate(pre):
        n = z.numel()
        neg, pos = int((z < 0).sum()), int((z > 0).sum())
        assert neg * 4 >= n and pos * 4 >= n, (case_id, i, neg, pos, n)
    assert any(bool((z < -5).any()) for z in pre), (case_id, [float(z.min()) for z in pre])
    assert bool((pre[0][:, C0] == 0).all()), (case_id, "column C0 of H0 is exactly 0")


def _report(s):
    print(s.replace("ROWSBAR", "SELUBAR"))


# ---- 1. the tile kernels, bond messages ---------------------------------------------------------------------------------------------
TILE = [(Case("h36-act-selu-bias", "qm9x12", 36, act="selu", bias=True), "tiles"), (Case("h36-act-selu-nobias", "qm9x12", 36, act="selu"), "full"),
        (Case("h132-act-selu-bias", "qm9x12", 132, act="selu", bias=True), "tiles"), (Case("h132-act-selu-nobias", "qm9x12", 132, act="selu"), "full"),
        (Case("h68-selu-chain26", "chain26", 68, act="selu", bias=True), "tiles")]   # (a molecule beyond the tile: the generic path)
_ids = lambda r: f"{r[0].id}@{r[1]}"


@pytest.mark.parametrize("run", TILE, ids=_ids)
def test_selu_tile_route(run, gpu_device):
    case, kind = run
    out64, pre64, g64, e32, _ = lh.yardsticks(case)
    condition(pre64, case.id)
    tb._hold(gpu_device, case, kind, out64, pre64, g64, e32)


# ---- 2. the tile kernels, atom messages ----------------------------------------------------------------------------------------------
ATOM = [(Case("h36-atom-selu-bias", "qm9x12", 36, act="selu", bias=True), "tiles"), (Case("h36-atom-selu-nobias", "qm9x12", 36, act="selu"), "full"),
        (Case("h132-atom-selu-bias", "qm9x12", 132, act="selu", bias=True), "full"), (Case("h132-atom-selu-nobias", "qm9x12", 132, act="selu"), "tiles")]


@functools.lru_cache(maxsize=None)
def _atom_operands(case):
    from chemprop_amd.data import BatchMolGraph
    from test_atom_tile_boundaries import _operands

    g, inp = _operands(case)
    inp = _shape_inputs(inp)
    return BatchMolGraph.from_tensors(inp["V"], inp["E"], g.edge_index, g.rev_edge_index, g.batch, len(g)), inp


def _atom_ref(case, dtype):
    bmg, inp = _atom_operands(case)
    L = {k: (None if inp[k] is None else inp[k].to(dtype).requires_grad_()) for k in ah.PARAMS}
    w = ot.MPWeights(L["W_i"], L["W_h"], L["W_o"], L["b_o"], L["b_i"], L["b_h"])
    del PRE[:]
    out = ot.atom_forward(bmg.V.to(dtype), bmg.E.to(dtype), bmg.edge_index, bmg.rev_edge_index, w, depth=case.depth, activation="selu")
    pre = list(PRE)
    return ah.named(out, ah.block_grads(out, L, inp["G"]), case.d_h), pre


@pytest.mark.parametrize("run", ATOM, ids=_ids)
def test_selu_atom_tile_route(run, gpu_device):
    case, kind = run
    _, inp = _atom_operands(case)
    ref, pre64 = _atom_ref(case, torch.float64)
    condition(pre64, case.id)
    e32 = ah.yardstick(ref, _atom_ref(case, torch.float32)[0])
    res = th.run_tile(gpu_device, case, kind, bits=False, atom=True, inputs=inp)
    assert not res["st"].args.keep_bits
    assert not th.run_tile(gpu_device, case, kind, bits=True, backward=0, atom=True, inputs=inp)["st"].args.keep_bits, "sign bits for a smooth activation"
    fails, _ = ah.compare(f"{case.id}@{kind}", ah.named(res["out"], res["grads"][0], case.d_h), ref, e32, rh.MARGIN)
    a, b = res["grads"]
    fails += [f"g{k}: two backward passes differ" for k in a if not torch.equal(a[k].view(torch.int32), b[k].view(torch.int32))]
    inf = th.run_tile(gpu_device, case, kind, keep=False, atom=True, inputs=inp)
    fails += ah.compare(f"{case.id}@{kind}/inference", dict(out=inf["out"]), dict(out=ref["out"]), e32, rh.MARGIN)[0]
    assert not fails, f"{case.id}@{kind}: " + "; ".join(fails)


# ---- 3. the per-step fused route on the f16 pipe (not lean) --------------------------------------------------------------------------
FUSED16 = [Case("h36-fused16-selu-bias", "chains30x6", 36, depth=3, act="selu", bias=True), Case("h132-fused16-selu", "degrees", 132, act="selu")]


@pytest.mark.parametrize("route", ["fused16", "fused"])
@pytest.mark.parametrize("case", FUSED16, ids=lambda c: c.id)
def test_selu_per_step_fused_route(case, route, gpu_device):
    from chemprop_amd import engine

    out64, pre64, g64, e32, _ = lh.yardsticks(case)
    condition(pre64, case.id)
    res = lh.run_lean(gpu_device, case, route=route)
    assert res["st"].route == route and res["bits"] is None and not res["st"].args.keep_bits, res["st"].route
    kinds = dict(out="fwd", **{k: "grad" for k in lh.GRADS})
    fails = rh.compare(f"{case.id}@{route}", dict(out=res["out"], **res["grads"][0]), dict(out=out64, **g64), e32, kinds, report=_report)
    a, b = res["grads"]
    fails += [f"g{k}: two backward passes differ" for k in a if not torch.equal(a[k].view(torch.int32), b[k].view(torch.int32))]
    # inference: the same route without kept tensors
    inp = lh.inputs(case)
    plan, _ = lh.plan_of(case.graph, gpu_device)
    mv = lambda k: None if inp[k] is None else inp[k].to(gpu_device)
    out, st = engine.forward(plan, mv("V"), mv("E"), mv("W_i"), mv("W_h"), mv("W_o"), mv("b_o"), mv("b_i"), mv("b_h"), depth=case.depth, act="selu",
                             route=route)
    assert st.route.startswith(route), st.route
    fails += [f"inference: {f}" for f in rh.compare(f"{case.id}@{route}/inference", dict(out=out.cpu()), dict(out=out64), e32, "fwd", report=_report)]
    assert not fails, f"{case.id}: " + "; ".join(fails)


# ---- 4. the per-step general route: directed, undirected, W_d, the input gradients ---------------------------------------------------
# (graph, d_v, d_e, d_h, d_vd, depth, undirected, bias, mfma): the ELU cases of tests/test_input_grad_gpu.py and their twins on the other pipe
GENERAL = {
    "general16-directed-h300": (lambda: rh.chain_graph(4, 13, seed=8), 72, 1, 300, 0, 2, False, False, "split16"),
    "general-directed-h30-depth1-W_d": (lambda: rh.degree_graph([0, 1, 2, 4, 12, 3], seed=4), 72, 14, 30, 5, 1, False, False, "f32"),
    "general16-undirected-depth4": (lambda: rh.degree_graph([3, 3, 2, 1], seed=10), 17, 15, 16, 0, 4, True, True, "split16"),
    "general-undirected-W_d": (lambda: rh.chain_graph(1, 17, seed=14), 15, 1, 4, 5, 3, True, False, "f32"),
    "general16-directed-W_d-h66": (lambda: rh.degree_graph([0, 1, 2, 4, 12, 5, 6], seed=5), 16, 14, 66, 5, 3, False, True, "split16"),
    "general-directed-h31": (lambda: rh.chain_graph(5, 10, seed=6), 16, 15, 31, 0, 3, False, True, "f32"),
}


def _general_ref(bmg, t, depth, undirected, dtype):
    del PRE[:]
    g = ig._oracle_grads(bmg, t, depth, "selu", undirected, dtype)
    return g, list(PRE)


@pytest.mark.parametrize("name", list(GENERAL))
def test_selu_general_routes(name, gpu_device):
    make, d_v, d_e, d_h, d_vd, depth, undirected, bias, mfma = GENERAL[name]
    bmg = make()
    t = ig._case_tensors(bmg, d_v, d_e, d_h, d_vd, bias, seed=len(name))
    t.update(_shape_inputs({k: t[k] for k in ("V", "E", "W_i", "b_i")}))
    ref, pre64 = _general_ref(bmg, t, depth, undirected, torch.float64)
    condition(pre64, name)
    e32 = rh.yardstick(ref, _general_ref(bmg, t, depth, undirected, torch.float32)[0])
    plan, d, out, st = ig._kept_forward(gpu_device, bmg, t, depth, "selu", undirected, mfma)
    present = [k for k in ig._PARAMS if t[k] is not None]
    want = ["V", "E"] + (["V_d"] if d_vd else [])
    rc, msg, grads, outs = ig._run_inputs(gpu_device, st, d["G"], {k: True for k in present}, want)
    assert rc == 0, msg
    got = {k: outs[k].read("g" + k) for k in want}
    got.update({k: grads[k].cpu() for k in present})
    got["out"] = out.cpu()
    kinds = {k: "grad" for k in got}
    kinds["out"] = "fwd"
    fails = rh.compare(f"selu-{name}", got, ref, e32, kinds, report=_report)
    assert not fails, fails


# ---- 5. ... with p = 0.25 in the row kernels, given the masks ------------------------------------------------------------------------
DROP = [(Case("h68-rows-dropout-selu", "chains30x6", 68, depth=3, act="selu", p=0.25, bias=True), False),
        (Case("h36-rows-dropout-selu-undirected", "qm9x12", 36, depth=3, act="selu", p=0.25), True)]


def _drop_ref(case, undirected, keeps, dtype):
    """base.py:196-212 in ``dtype`` with the masks replayed at the kernels' float scale."""
    bmg, inp = lh.graph(case.graph), lh.inputs(case)
    nV = int(bmg.V.shape[0])
    src, dst = bmg.edge_index
    rev = bmg.rev_edge_index
    L = {k: (None if inp[k] is None else inp[k].to(dtype).requires_grad_()) for k in lh.GRADS}
    w = ot.MPWeights(L["W_i"], L["W_h"], L["W_o"], L["b_o"], L["b_i"], L["b_h"])
    V, E = inp["V"].to(dtype), inp["E"].to(dtype)
    s = ah.scale32(case.p)
    pre = []

    def tau(z):
        pre.append(z.detach())
        return F.selu(z)

    H0 = ot.initialize(V, E, src, w)
    H = tau(H0)
    for t in range(1, case.depth):
        if undirected:
            H = (H + H[rev]) / 2
        H = ot.update(ot.message(H, src, dst, rev, nV), H0, w, tau) * (keeps[t - 1].to(dtype) * s)
    out = ot.finalize(ot.segment_sum_dst(H, dst, nV), V, None, w, tau) * (keeps[-1].to(dtype) * s)
    (out * inp["G"].to(dtype)).sum().backward()
    return dict(out=out.detach(), **{k: p.grad for k, p in L.items() if p is not None}), pre


@pytest.mark.parametrize("run", DROP, ids=lambda r: r[0].id)
def test_selu_general16_with_dropout_given_its_masks(run, gpu_device):
    from chemprop_amd import engine

    case, undirected = run
    bmg, inp = lh.graph(case.graph), lh.inputs(case)
    nV, nE = int(bmg.V.shape[0]), int(bmg.edge_index.shape[1])
    keeps = lh.keep_masks(case, nE, nV)
    assert 0.6 < float(keeps[0].float().mean()) < 0.9
    ref, pre64 = _drop_ref(case, undirected, keeps, torch.float64)
    condition(pre64, case.id)
    e32 = rh.yardstick(ref, _drop_ref(case, undirected, keeps, torch.float32)[0])
    plan, _ = lh.plan_of(case.graph, gpu_device)
    mv = lambda k: None if inp[k] is None else inp[k].to(gpu_device)
    out, st = engine.forward(plan, mv("V"), mv("E"), mv("W_i"), mv("W_h"), mv("W_o"), mv("b_o"), mv("b_i"), mv("b_h"), depth=case.depth, act="selu",
                             keep=True, route="general", mfma="split16", dropout=(case.p, lh.DROP_SEED), undirected=undirected,
                             undirected_dropout=undirected)
    assert st.route == "general16" and float(st.args.dropout_p) == pytest.approx(case.p), st.route
    got = engine.backward(st, mv("G"), {k: True for k in lh.GRADS})
    torch.cuda.synchronize()
    got = dict(out=out.cpu(), **{k: v.cpu() for k, v in got.items() if v is not None})
    assert bool((got["out"][~keeps[-1]] == 0).all()), "an entry the finalize's mask drops is exactly zero"
    kinds = dict(out="fwd", **{k: "grad" for k in lh.GRADS})
    fails = rh.compare(case.id, got, ref, e32, kinds, report=_report)
    assert not fails, f"{case.id}: " + "; ".join(fails)


# ---- 6. the mol-atom-bond blocks on the tile route, both read-outs -------------------------------------------------------------------
@pytest.mark.parametrize("atom", [False, True], ids=["bond-messages", "atom-messages"])
def test_selu_mol_atom_bond_on_the_tile_route(atom, gpu_device, monkeypatch):
    from chemprop_amd import synth
    from chemprop_amd.mab import MABAtomMessagePassing, MABBondMessagePassing

    monkeypatch.setenv("DMPNN_VALIDATE", "never")
    cls = MABAtomMessagePassing if atom else MABBondMessagePassing
    kw = dict(activation="selu", bias=True, depth=3, d_h=64)
    bmg = synth.random_batch(24, "qm9", seed=14)
    bmg.V, bmg.E = bmg.V * SCALE, bmg.E * SCALE
    torch.manual_seed(9)
    ref_mp = cls(**kw)
    with torch.no_grad():
        ref_mp.W_i.weight[C0] = 0.0
        ref_mp.W_i.bias[C0] = 0.0
    assert ref_mp.return_vertex_embeddings and ref_mp.return_edge_embeddings
    gen = torch.Generator().manual_seed(3)
    Gs = None

    def reference(dtype):
        nonlocal Gs
        mp = cls(**kw).to(dtype)
        mp.load_state_dict({k: v.to(dtype) for k, v in ref_mp.state_dict().items()})
        w = ot.MABWeights.from_state_dict(dict(mp.named_parameters()))
        del PRE[:]
        ref = ot.mab_forward(bmg.V.to(dtype), bmg.E.to(dtype), bmg.edge_index, bmg.rev_edge_index, w, atom_messages=atom, depth=mp.depth, activation="selu")
        pre = list(PRE)
        if Gs is None:
            Gs = [torch.randn(r.shape, generator=gen) for r in ref]
        sum((r * g.to(dtype)).sum() for r, g in zip(ref, Gs)).backward()
        t = dict(H_v=ref[0].detach(), H_e=ref[1].detach(), **{k: p.grad for k, p in mp.named_parameters()})
        return t, pre

    ref, pre64 = reference(torch.float64)
    condition(pre64, f"mab-{atom}")
    e32 = rh.yardstick(ref, reference(torch.float32)[0])
    dev_bmg = synth.random_batch(24, "qm9", seed=14)
    dev_bmg.V, dev_bmg.E = dev_bmg.V * SCALE, dev_bmg.E * SCALE
    dev_bmg.to(gpu_device)
    for plan_kind in ("tiles", "full"):
        monkeypatch.setenv("DMPNN_TRAIN_PLAN", plan_kind)
        mp = cls(**kw)
        mp.load_state_dict(ref_mp.state_dict())
        mp = mp.to(gpu_device).train()
        out = mp(dev_bmg)
        assert mp.__dict__.get("_dmpnn_route") == ("mega16/atom" if atom else "mega16"), (plan_kind, mp.__dict__.get("_dmpnn_route"))
        sum((o * g.to(gpu_device)).sum() for o, g in zip(out, Gs)).backward()
        got = dict(H_v=out[0].detach().cpu(), H_e=out[1].detach().cpu(), **{k: p.grad.cpu() for k, p in mp.named_parameters()})
        kinds = {k: "grad" for k in got}
        kinds["H_v"] = kinds["H_e"] = "fwd"
        fails = rh.compare(f"selu-mab-{'atom' if atom else 'bond'}@{plan_kind}", got, ref, e32, kinds, report=_report)
        assert not fails, f"{plan_kind}: " + "; ".join(fails)
        # inference on the tile route: both read-outs again
        with torch.no_grad():
            mp.eval()
            inf = mp(dev_bmg)
        fails = rh.compare(f"selu-mab-{'atom' if atom else 'bond'}@{plan_kind}/inference", dict(H_v=inf[0].cpu(), H_e=inf[1].cpu()),
                           dict(H_v=ref["H_v"], H_e=ref["H_e"]), e32, "fwd", report=_report)
        assert not fails, f"{plan_kind} inference: " + "; ".join(fails)


# ---- 7. one block, two routes -------------------------------------------------------------------------------------------------------
def test_selu_tile_route_and_general16_agree(gpu_device):
    from chemprop_amd import engine

    case = TILE[0][0]
    inp = lh.inputs(case)
    tile = th.run_tile(gpu_device, case, "full", bits=False, backward=0)
    plan, _ = lh.plan_of(case.graph, gpu_device)
    mv = lambda k: None if inp[k] is None else inp[k].to(gpu_device)
    out, st = engine.forward(plan, mv("V"), mv("E"), mv("W_i"), mv("W_h"), mv("W_o"), mv("b_o"), mv("b_i"), mv("b_h"), depth=case.depth, act="selu",
                             keep=True, route="general", mfma="split16")
    assert st.route == "general16", st.route
    err = parity_err(out.cpu().numpy(), tile["out"].numpy())
    print(f"SELUROUTES out tile-vs-general16 err={err:.3e} bar={TOL:.1e}")
    assert err <= TOL
