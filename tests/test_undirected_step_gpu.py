"""Undirected bond blocks on the GPU: the undirected hot builds of the message kernel (``k_segment<4, 0, 1, none | relu>``) against the
generic build bit for bit and against float64; the training forward / backward of the per-step general route on the f16 pipe with
block dropout and undirected messages (``DMPNN_F_UNDIRECTED_MASK``: ``engine.forward(..., undirected=True, route="general",
mfma="split16", keep=True, dropout=(p, seed), undirected_dropout=True)`` and ``engine.backward``) given the hash masks; the one-call
step (``FusedTrainer(model, undirected=True)``) and ``HipMPNN``.

Every reference is float64 with the hash masks of ``oracle/dropout_hash.py`` replayed at the kernels' ``float`` scale, as in
tests/test_rows_dropout_gpu.py, whose helpers and bars this file uses: output <= TOL = 1e-5, every parameter gradient (unfloored)
<= 2e-5, at most 8 ReLU-class decisions away from float64's, each within 1e-5 of the kink; the message kernel at
``rows_harness.MARGIN`` times the float32 restatement's own error.

Figures of this file's cases on one MI355X (they are printed before every assertion):
  message kernel  err / max(e32, 2**-23) at most 1.00 over the 16 cases (bar 16); the hot and the generic build differ in 0 entries in
                  every case, and both are the float32 restatement bit for bit
  engine          output error 2.7e-07 .. 7.0e-07 (bar 1e-5), every gradient given the masks (unfloored) at most 6.6e-07 (bar 2e-5), no
                  ReLU-class decision differs from float64's in the three ReLU-class cases (at most 8 may, each at the kink)
  one-call step   p = 0: loss 0.95950800 against float64's 0.95950796 (zinc), 0.95554590 against 0.95554589 (qm9); every gradient of
                  the model against float64 autograd at most 9.2e-09 of max(1, max|ref|) (bar 2e-5)
  W_d + dropout   three steps against the module path given the masks: losses agree to 1.4e-06 of max(1, |loss|) (bar 1e-4), parameters after
                  them to 2.5e-07 (bar 1e-4)
"""
import copy
import functools
import types

import numpy as np
import pytest
import torch

import rows_harness as rh
from chemprop_amd import _lib
from conftest import TOL, parity_err, parity_err_unfloored
from test_dropout_gpu import ReplayDropout, _restated_forward
from test_lean_dropout_gpu import NAMES, RecordingTau, ReplayTau
from test_multicomponent_integration import stub_chemprop  # noqa: F401  (the fixture)
from test_rows_dropout_gpu import ROWS, SEED, SEED2, _batch, _engine_forward, _masks, _reference, _slope

pytestmark = pytest.mark.gpu

UROWS = dict(ROWS, undirected=True, undirected_dropout=True)


def bits(t):
    return t.contiguous().view(torch.int32)


# ---- 1. the message kernel: the undirected hot builds -----------------------------------------------------------------------------------
DEGREES = (0, 1, 2, 3, 4, 5, 6, 7)     # every straight-line body (1 .. 6) and the any-degree body (7)
SEG_H = (4, 256, 300, 516)             # under one column group, exactly 64 lanes, 75 float4 (a partial second group), a third pass
SEG_CASES = [(g, h, act) for g in ("degrees", "zinc") for h in SEG_H for act in ("none", "relu")]


@functools.lru_cache(maxsize=None)
def _seg_graph(name):
    from chemprop_amd import synth

    return rh.degree_graph(DEGREES, seed=3) if name == "degrees" else synth.random_batch(24, "zinc", seed=17)


@functools.lru_cache(maxsize=None)
def _seg_input(name, h):
    nE = int(_seg_graph(name).edge_index.shape[1])
    return torch.randn(nE, h, generator=torch.Generator().manual_seed(300 + h)) * (1 + torch.arange(h).float() / h)


@functools.lru_cache(maxsize=None)
def _seg_ref(name, h, act):
    bmg, Hin = _seg_graph(name), _seg_input(name, h)
    r64, r32 = rh.segment_fwd_ref(bmg, Hin, "message", act, True), rh.segment_fwd_ref(bmg, Hin, "message", act, True, torch.float32)
    return r64, r32, rh.yardstick(dict(out=r64), dict(out=r32))


def test_the_degree_graph_reaches_every_body():
    assert set(rh.in_degrees(_seg_graph("degrees")).tolist()) == set(DEGREES)
    assert int(rh.in_degrees(_seg_graph("zinc")).max()) <= 4


@pytest.mark.parametrize("graph,h,act", SEG_CASES, ids=[f"{g}-h{h}-{a}" for g, h, a in SEG_CASES])
def test_undirected_message_hot_build_equals_the_generic_build(graph, h, act, gpu_device):
    """The aligned layout runs ``k_segment<4, 0, 1, act>``; the same input at ``ld_in = h + 1`` the scalar generic build: bit for bit.
    Both against float64 at the row kernels' bar; padding columns and guard words untouched."""
    bmg, Hin = _seg_graph(graph), _seg_input(graph, h)
    plan, _ = rh.make_plan(bmg, gpu_device)
    r64, r32, e32 = _seg_ref(graph, h, act)
    case = f"undirected-message {graph} h{h} {act}"
    rc, msg, hot = rh.run_segment_fwd(gpu_device, plan, "message", Hin, act, undirected=True, ld_out=h + 4)
    assert rc == 0, msg
    rc, msg, gen = rh.run_segment_fwd(gpu_device, plan, "message", Hin, act, undirected=True, ld_in=h + 1)
    assert rc == 0, msg
    got_hot, got_gen = hot.read(case + " hot"), gen.read(case + " generic")
    differ = int((bits(got_hot) != bits(got_gen)).sum())
    print(f"UNDIR {case}: {differ} entries differ between the hot and the generic build")
    assert differ == 0, case
    fails = rh.compare(case, dict(out=got_hot), dict(out=r64), e32, "fwd")
    assert not fails, (case, fails)
    assert torch.equal(bits(got_hot), bits(r32)), f"{case}: not the float32 run of the same sums"


# ---- 2. forward and every parameter gradient through the engine, given the masks -------------------------------------------------------
CASES = [
    (12, "zinc", dict(d_h=400, depth=3), 0.25),
    (8, "synth40", dict(d_h=324, depth=2, activation="leakyrelu", bias=True), 0.4),
    (16, "qm9", dict(d_h=302, depth=4, activation="tanh"), 0.2),                   # N % 4 != 0: the scalar epilogue, ldh = 304
    (4, "synth40", dict(d_h=1024, depth=2, activation="elu", bias=True), 0.5),
    (10, "zinc", dict(d_h=64, depth=1), 0.3),                                      # no averaging happens: the directed run, bit for bit
]


@pytest.mark.parametrize("n_mols,kind,kw,p", CASES, ids=[f"{c[1]}-{c[0]}-h{c[2]['d_h']}" for c in CASES])
def test_undirected_general16_dropout_given_its_masks(n_mols, kind, kw, p, gpu_device):
    from chemprop_amd import engine, synth
    from chemprop_amd.nn import BondMessagePassing

    dev = gpu_device
    kw = dict(kw, undirected=True)
    cpu_bmg = synth.random_batch(n_mols, kind, seed=11)
    torch.manual_seed(5)
    mp = BondMessagePassing(dropout=p, **kw)
    state = {k: v.clone() for k, v in mp.state_dict().items()}
    nV, nE, d_h, depth = int(cpu_bmg.V.shape[0]), int(cpu_bmg.E.shape[0]), kw["d_h"], mp.depth
    act_name = type(mp.tau).__name__
    relu_class = act_name in ("ReLU", "LeakyReLU")
    G = torch.randn(nV, d_h, generator=torch.Generator().manual_seed(6))
    mp = mp.to(dev).train()
    bmg = synth.random_batch(n_mols, kind, seed=11)
    bmg.to(dev)
    plan = engine.GraphPlan.from_bmg(bmg)
    assert nE > 48 and nV > 48
    tag = f"undirected rows-dropout {kind}-{n_mols}-h{d_h}"

    with pytest.raises(engine.RouteUnavailable):                                   # (without the keyword: as before)
        _engine_forward(mp, plan, bmg, (p, SEED), undirected=True, **ROWS)
    out, st = _engine_forward(mp, plan, bmg, (p, SEED), **UROWS)
    assert st.route == "general16", st.route
    assert int(st.args.flags) & _lib.F_UNDIRECTED_MASK and int(st.args.flags) & _lib.F_UNDIRECTED
    assert abs(float(st.args.dropout_p) - p) < 1e-7 and int(st.args.dropout_seed) == SEED
    need = {k: True for k, _, _ in NAMES}
    g1 = engine.backward(st, G.to(dev), need)
    g1 = {k: (None if v is None else v.clone()) for k, v in g1.items()}
    g2 = engine.backward(st, G.to(dev), need)
    torch.cuda.synchronize()
    for k in g1:                                                                   # two backward passes on one forward: bit-identical
        assert (g1[k] is None) == (g2[k] is None) and (g1[k] is None or torch.equal(g1[k], g2[k])), k
    again, _ = _engine_forward(mp, plan, bmg, (p, SEED), **UROWS)
    other, _ = _engine_forward(mp, plan, bmg, (p, SEED2), **UROWS)
    assert torch.equal(again, out)
    assert not torch.equal(other == 0, out == 0)

    keeps = _masks(SEED, p, depth, nE, nV, d_h)
    out_c = out.detach().cpu()
    fin = keeps[-1]
    # what the hash drops is exactly zero in H^(t) and in the output; a smooth activation is zero nowhere else
    assert bool((out_c[~fin] == 0).all())
    if not relu_class:
        assert torch.equal(out_c == 0, ~fin)
    Hs = st.Hs[:, :, :d_h].detach().cpu() if depth > 1 else None
    for t in range(depth - 1):
        assert bool((Hs[t][~keeps[t]] == 0).all()), f"update site {t}"
        if not relu_class:
            assert torch.equal(Hs[t] == 0, ~keeps[t]), f"update site {t}"

    # the directed forward under the same seed: the same zero patterns (the mask does not care about direction) ...
    if act_name == "Tanh" or depth == 1:
        d_out, d_st = _engine_forward(mp, plan, bmg, (p, SEED), **ROWS)
        assert not int(d_st.args.flags) & (_lib.F_UNDIRECTED | _lib.F_UNDIRECTED_MASK)
        assert torch.equal(d_out == 0, out == 0)
        for t in range(depth - 1):
            assert torch.equal(d_st.Hs[t][:, :d_h] == 0, st.Hs[t][:, :d_h] == 0), f"update site {t}"
        if depth == 1:
            # ... and with no message step nothing is averaged: output and every gradient bit-equal to the directed run
            assert torch.equal(bits(d_out), bits(out))
            gd = engine.backward(d_st, G.to(dev), need)
            torch.cuda.synchronize()
            for k in g1:
                assert (g1[k] is None) == (gd[k] is None) and (g1[k] is None or torch.equal(bits(g1[k]), bits(gd[k]))), k
        else:
            assert not torch.equal(d_out, out)                                     # (the average does change the numbers)

    # the output against float64 given the masks
    ref, ref_out = _reference(cpu_bmg, kw, state, p, keeps, RecordingTau)
    assert ref.undirected
    pre = ref.tau.pre
    assert len(pre) == depth + 1
    err_out = parity_err(out_c.numpy(), ref_out.detach().numpy())
    print(f"{tag}: output error {err_out:.3e}")
    assert err_out <= TOL, err_out

    if relu_class:
        H0 = st.H0[:, :d_h].detach().cpu()
        cond = [H0 > 0] + [torch.where(keeps[t], Hs[t] > 0, pre[t + 1] > 0) for t in range(depth - 1)] + [torch.where(fin, out_c > 0, pre[depth] > 0)]
        flips = 0
        for t in range(depth + 1):
            diff = cond[t] != (pre[t] > 0)
            flips += int(diff.sum())
            if diff.any():
                assert float(pre[t][diff].abs().max()) <= 1e-5 * float(pre[t].abs().max()), f"site {t}: a decision differs away from the kink"
        print(f"{tag}: {flips} activation decisions differ from float64's")
        assert flips <= 8, flips
        ref, ref_out = _reference(cpu_bmg, kw, state, p, keeps, lambda inner: ReplayTau(cond, _slope(mp)))
        assert parity_err(out_c.numpy(), ref_out.detach().numpy()) <= TOL
    else:
        ref, ref_out = _reference(cpu_bmg, kw, state, p, keeps, lambda inner: inner)
    (ref_out * G.double()).sum().backward()
    errs = {}
    for k, lin, n in NAMES:
        prm = getattr(getattr(ref, lin), n)
        if prm is None:
            assert g1[k] is None
            continue
        if prm.grad is None:                                                       # (depth 1: W_h takes no part; the engine answers zeros)
            assert depth == 1 and lin == "W_h" and not bool(g1[k].any()), k
            continue
        errs[k] = parity_err_unfloored(g1[k].cpu().numpy(), prm.grad.numpy())
    print(f"{tag}: gradient errors given the masks {errs}")
    assert max(errs.values()) <= 2e-5, errs


# ---- 3. the one-call step -------------------------------------------------------------------------------------------------------------
def _model(dev, p, **mp_kw):
    from chemprop_amd import agg as cagg
    from chemprop_amd.model import MPNN, RegressionFFN
    from chemprop_amd.nn import BondMessagePassing

    mp = BondMessagePassing(dropout=p, undirected=True, **mp_kw)
    return MPNN(mp, cagg.MeanAggregation(), RegressionFFN(input_dim=mp_kw["d_h"])).to(dev).train()


STEP_MODELS = [("zinc", dict(d_h=400)), ("qm9", dict(d_h=64, activation="tanh"))]
STEP_IDS = ["zinc-relu-h400", "qm9-tanh-h64"]


def _hand_step(before, tr, model, bmg, y, drop, **fwd_kw):
    """The step by hand on the parameters before it: engine.forward, the head on its output, engine.backward on gH_v — its loss within
    1e-6 relative and its block gradients bit-equal to the flat buffer's.  -> the forward's state."""
    from chemprop_amd import engine
    from head_harness import run_head

    dev = bmg.V.device
    step_grads = {id(p): tr._views[id(p)].detach().clone() for p in model.message_passing.parameters()}
    plan = engine.GraphPlan.from_bmg(bmg)
    out, st = _engine_forward(before.message_passing, plan, bmg, drop, undirected=True, **fwd_kw)
    head_loss, _, _, gH = run_head(before, out, bmg.batch, len(bmg), y, None, None, None)
    grads = engine.backward(st, gH.to(dev), {k: True for k, _, _ in NAMES})
    torch.cuda.synchronize()
    named = dict(model.message_passing.named_parameters())
    assert len(named) == len(step_grads)
    for k, lin, n in NAMES:
        p_new = named.get(f"{lin}.{n}")
        if p_new is None:
            assert grads[k] is None
            continue
        assert torch.equal(grads[k], step_grads[id(p_new)]), f"{k}: the step's gradient is not engine.backward's, bit for bit"
    return st, head_loss


@pytest.mark.parametrize("kind,kw", STEP_MODELS, ids=STEP_IDS)
def test_fused_trainer_takes_an_undirected_block_on_request(kind, kw, gpu_device):
    from chemprop_amd import synth
    from chemprop_amd.model import FusedTrainer, criterion_loss
    from oracle import agg_torch, ffn_torch

    dev = gpu_device
    torch.manual_seed(21)
    model = _model(dev, 0.0, **kw)
    bmg, y = _batch(dev, kind)
    before = copy.deepcopy(model)
    with pytest.raises(NotImplementedError):                                       # (the test that fails without the feature's keyword)
        FusedTrainer(copy.deepcopy(model), lr=1e-3)
    tr = FusedTrainer(model, lr=1e-3, undirected=True)
    rng = torch.get_rng_state()
    loss = tr.step(bmg, y)
    torch.cuda.synchronize()
    assert torch.equal(torch.get_rng_state(), rng)                                 # (p = 0: no seed)
    all_grads = {k: tr._views[id(p)].detach().cpu().clone() for k, p in model.named_parameters()}
    st, head_loss = _hand_step(before, tr, model, bmg, y, None)
    assert tr.last_route == st.route and st.route in ("general", "general16"), (tr.last_route, st.route)
    assert int(st.args.flags) & _lib.F_UNDIRECTED and not int(st.args.flags) & _lib.F_UNDIRECTED_MASK
    assert abs(float(loss[0]) - head_loss) <= 1e-6 * abs(head_loss), (float(loss[0]), head_loss)

    # every gradient against float64 autograd on the restated model
    ref = copy.deepcopy(before).cpu().double()
    cpu = synth.random_batch(24, kind, seed=13)
    g = types.SimpleNamespace(V=cpu.V.double(), E=cpu.E.double(), edge_index=cpu.edge_index, rev_edge_index=cpu.rev_edge_index)
    Hv = _restated_forward(g, ref.message_passing, lambda x: x)
    lin = [m for m in ref.predictor.ffn.modules() if isinstance(m, torch.nn.Linear)]                # (MeanAggregation, no batch norm, a ReLU MLP)
    preds = ffn_torch.mlp_forward(agg_torch.mean(Hv, cpu.batch), [m.weight for m in lin], [m.bias for m in lin], "relu")
    l64 = criterion_loss(ref.criterion, preds, y.cpu().double())
    l64.backward()
    assert abs(float(loss[0]) - float(l64)) <= 1e-5 * max(1.0, abs(float(l64))), (float(loss[0]), float(l64))
    errs = {k: parity_err(all_grads[k].numpy(), p.grad.numpy()) for k, p in ref.named_parameters()}
    print(f"undirected step {kind}: loss {float(loss[0]):.8f} float64 {float(l64):.8f}, gradient errors {errs}")
    assert len(errs) == len(all_grads) and max(errs.values()) <= 2e-5, errs


@pytest.mark.parametrize("kind,kw", STEP_MODELS, ids=STEP_IDS)
def test_fused_trainer_takes_an_undirected_block_with_dropout_in_the_row_kernels(kind, kw, gpu_device):
    from chemprop_amd.model import FusedTrainer

    dev = gpu_device
    torch.manual_seed(21)
    model = _model(dev, 0.2, **kw)
    bmg, y = _batch(dev, kind)
    before = copy.deepcopy(model)
    for kws in (dict(), dict(rows_dropout=True), dict(undirected=True)):           # (both keywords are needed)
        with pytest.raises(NotImplementedError):
            FusedTrainer(copy.deepcopy(model), lr=1e-3, **kws)
    tr = FusedTrainer(model, lr=1e-3, rows_dropout=True, undirected=True)
    torch.manual_seed(99)
    first = int(torch.randint(0, 2 ** 62, (1,), dtype=torch.int64).item())
    torch.manual_seed(99)
    loss = tr.step(bmg, y)
    torch.cuda.synchronize()
    assert tr.last_route == "general16", tr.last_route
    assert tr.last_dropout_seed == first
    st, head_loss = _hand_step(before, tr, model, bmg, y, (0.2, first), undirected_dropout=True, **ROWS)
    assert st.route == "general16" and int(st.args.flags) & _lib.F_UNDIRECTED_MASK
    assert abs(float(loss[0]) - head_loss) <= 1e-6 * abs(head_loss), (float(loss[0]), head_loss)


def test_fused_trainer_refuses_undirected_dropout_before_a_seed_is_drawn(gpu_device):
    """A trainer built for ``p = 0`` without ``rows_dropout`` whose module's ``p`` was raised since: the step refuses, torch's generator
    untouched, nothing updated.  The same with ``rows_dropout`` for a shape the row kernels refuse (odd ``d_v``)."""
    from chemprop_amd import synth
    from chemprop_amd.model import FusedTrainer

    dev = gpu_device
    torch.manual_seed(24)
    model = _model(dev, 0.0, d_h=64, activation="tanh")
    bmg, y = _batch(dev, "qm9")
    tr = FusedTrainer(model, lr=1e-3, undirected=True)
    model.message_passing.dropout.p = 0.2
    before = [p.detach().clone() for p in model.parameters()]
    rng = torch.get_rng_state()
    with pytest.raises(NotImplementedError, match="rows_dropout"):
        tr.step(bmg, y)
    assert torch.equal(torch.get_rng_state(), rng) and tr.opt.steps == 0
    assert all(torch.equal(p, q) for p, q in zip(model.parameters(), before))

    odd = _model(dev, 0.2, d_h=64, activation="tanh", d_v=71)
    b71 = synth.random_batch(16, "qm9", seed=2, d_v=71)
    b71.to(dev)
    tr = FusedTrainer(odd, lr=1e-3, rows_dropout=True, undirected=True)
    rng = torch.get_rng_state()
    with pytest.raises(NotImplementedError, match="odd d_v"):
        tr.step(b71, torch.randn(16, 1, device=dev))
    assert torch.equal(torch.get_rng_state(), rng) and tr.opt.steps == 0


def test_fused_trainer_eval_draws_no_seed_for_an_undirected_block(gpu_device):
    from chemprop_amd.model import FusedTrainer

    dev = gpu_device
    torch.manual_seed(23)
    model = _model(dev, 0.2, d_h=64, activation="tanh")
    bmg, y = _batch(dev, "qm9")
    tr = FusedTrainer(model, lr=1e-3, rows_dropout=True, undirected=True)
    model.eval()
    rng = torch.get_rng_state()
    part = tr._block_args(tr.mp, bmg, len(bmg), tr.acts[0], False, None, None)
    assert float(part.st.args.dropout_p) == 0.0 and torch.equal(torch.get_rng_state(), rng)
    assert int(part.st.args.flags) & _lib.F_UNDIRECTED and not int(part.st.args.flags) & _lib.F_UNDIRECTED_MASK
    assert not hasattr(tr, "last_dropout_seed") or tr.last_dropout_seed is None
    with pytest.raises(RuntimeError, match="eval mode"):
        tr.step(bmg, y)


LEARN = [("zinc", dict(d_h=400), 0.2), ("qm9", dict(d_h=64, activation="tanh"), 0.2), ("qm9", dict(d_h=64, activation="tanh"), 0.0)]


@pytest.mark.parametrize("kind,kw,p", LEARN, ids=["zinc-relu-h400-p0.2", "qm9-tanh-h64-p0.2", "qm9-tanh-h64-p0"])
def test_fused_trainer_learns_with_an_undirected_block(kind, kw, p, gpu_device):
    from chemprop_amd.model import FusedTrainer

    dev = gpu_device
    torch.manual_seed(22)
    model = _model(dev, p, **kw)
    bmg, y = _batch(dev, kind)
    tr = FusedTrainer(model, lr=3e-3, rows_dropout=True, undirected=True)
    losses = [float(tr.step(bmg, y)[0]) for _ in range(60)]
    assert tr.last_route == "general16" if p > 0 else tr.last_route in ("general", "general16"), tr.last_route
    print(f"undirected trainer {kind} p={p}: first five losses {losses[:5]}, last five {losses[-5:]}")
    assert np.mean(losses[-5:]) < 0.7 * np.mean(losses[:5]), (losses[:5], losses[-5:])


def test_undirected_step_with_atom_descriptors_and_dropout_equals_module_path_given_the_masks(gpu_device, monkeypatch):
    """``FusedTrainer(rows_dropout=True, vd_dropout=True, undirected=True).step(bmg, y, w, V_d=V)`` three times against the module path
    run op by op on a copy whose dropout replays the hash masks of the seed each step drew — the step comparison of
    tests/test_vd_dropout_gpu.py (its ``rows`` home), with an undirected block."""
    from chemprop_amd import agg as cagg
    from chemprop_amd import synth
    from chemprop_amd.model import MPNN, MSE, FusedTrainer, RegressionFFN, masked_loss
    from chemprop_amd.nn import BondMessagePassing
    from test_vd_dropout_gpu import P, _masks as vd_masks, _spy

    monkeypatch.setenv("DMPNN_VALIDATE", "never")
    dev, d_h, d_vd, n_mols, depth = gpu_device, 64, 5, 32, 3
    torch.manual_seed(11)
    mp = BondMessagePassing(d_h=d_h, depth=depth, activation="elu", d_vd=d_vd, dropout=P, undirected=True)
    pred = RegressionFFN(n_tasks=1, input_dim=mp.output_dim, hidden_dim=300, n_layers=1, activation="elu", criterion=MSE(1.0))
    a = MPNN(mp, cagg.NormAggregation(), pred, batch_norm=True)
    b = copy.deepcopy(a)
    a, b = a.to(dev).train(), b.to(dev).train()
    bmg = synth.random_batch(n_mols, "zinc", seed=12)
    bmg.to(dev)
    gen = torch.Generator().manual_seed(13)
    y = torch.randn(n_mols, 1, generator=gen).to(dev)
    w = (0.5 + torch.rand(n_mols, 1, generator=gen)).to(dev)
    V = torch.randn(int(bmg.V.shape[0]), d_vd, generator=gen).to(dev)
    for kws in (dict(rows_dropout=True, vd_dropout=True), dict(rows_dropout=True, undirected=True), dict(vd_dropout=True, undirected=True)):
        with pytest.raises(NotImplementedError):                                   # (all three keywords are needed)
            FusedTrainer(copy.deepcopy(a), lr=1e-3, eps=1e-4, **kws)
    tr = FusedTrainer(a, lr=1e-3, eps=1e-4, rows_dropout=True, vd_dropout=True, undirected=True)
    seen = _spy(tr)
    mp_b = b.message_passing
    nV, nE = int(bmg.V.shape[0]), int(bmg.E.shape[0])
    opt = torch.optim.Adam([p for p in b.parameters() if p.requires_grad], lr=1e-3, eps=1e-4)
    seeds = []
    for s in range(3):
        la = float(tr.step(bmg, y, w, V_d=V)[0])
        assert tr.last_route == "general16", tr.last_route
        seed = int(tr.last_dropout_seed)
        seeds.append(seed)
        vd = seen["vd"]
        assert abs(float(vd.dropout_p) - P) < 1e-7 and int(vd.dropout_seed) == seed
        args = seen["part"].st.args
        assert float(args.dropout_p) == float(vd.dropout_p) and int(args.dropout_seed) == seed and int(args.flags) & _lib.F_UNDIRECTED_MASK
        _, masks = vd_masks(seed, P, depth, nE, nV, d_h, d_vd, dev)
        mp_b.dropout = ReplayDropout(P, masks)
        opt.zero_grad()
        lb = masked_loss(b.predictor.train_step(b.fingerprint(bmg, V, None)), y, w, None, None, None, "mse")
        lb.backward()
        opt.step()
        assert mp_b.dropout.i == depth + 1   # (every site was visited, the one behind W_d last)
        lb = float(lb.detach())
        print(f"undirected VDDROP step {s}: fused {la:.8f} module {lb:.8f}")
        assert abs(la - lb) <= (1e-5 if s == 0 else 1e-4) * max(1.0, abs(lb)), (s, la, lb)
    torch.cuda.synchronize()
    assert len(set(seeds)) == 3 and tr.opt.steps == 3
    for (k, pa), (kb, pb) in zip(a.named_parameters(), b.named_parameters()):
        assert k == kb
        e = parity_err(pa.detach().cpu().numpy(), pb.detach().cpu().numpy())
        print(f"undirected VDDROP {k}: {e:.2e}")
        assert e <= 1e-4, f"{k}: {e:.2e}"


# ---- 4. HipMPNN -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [0.0, 0.2])
def test_hip_mpnn_takes_an_undirected_block_on_the_fused_step(p, stub_chemprop, gpu_device):  # noqa: F811
    """``HipMPNN`` with an undirected ``BondMessagePassing`` under the Trainer stand-in reports a ``fused:`` route, not the module path,
    and moves the parameters."""
    from chemprop_amd.model import RegressionFFN

    S = stub_chemprop
    integ = S.integration
    integ.enable()
    HipM = integ.hip_mpnn_class()[1]
    torch.manual_seed(3)
    mp = S.mods["chemprop.nn"].BondMessagePassing(d_h=64, undirected=True, dropout=p)
    model = HipM(mp, S.mods["chemprop.nn"].NormAggregation(), RegressionFFN(input_dim=64), batch_norm=True, init_lr=1e-3).to(gpu_device).train()
    assert model.message_passing.undirected
    opt = model.configure_optimizers()["optimizer"]
    model._trainer = types.SimpleNamespace(optimizers=[opt], accumulate_grad_batches=1, gradient_clip_val=None, gradient_clip_algorithm=None,
                                           strategy=None)
    bmg, y = _batch(gpu_device, "qm9")
    before = model.message_passing.W_h.weight.detach().clone()
    for i in range(3):
        opt.step(lambda i=i: model.training_step((bmg, None, None, y, None, None, None), i))
        route = model.__dict__["_hip"]["route"]
        assert route == "fused:general16" if p > 0 else route in ("fused:general", "fused:general16"), model.__dict__["_hip"]
    torch.cuda.synchronize()
    assert not torch.equal(model.message_passing.W_h.weight.detach(), before)
