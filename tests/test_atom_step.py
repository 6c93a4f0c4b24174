"""Atom-message models on the one-call step: ``fused_block(..., atom_messages=True)`` / ``FusedTrainer(..., atom_messages=True)`` and
``HipMPNN``.

CPU: the defaults still refuse an atom block; with the flag the block is taken with the bond block's ``(activation, slope)``; what
the kernels do not implement is refused (undirected, PReLU, ``W_d``, ``d_e > 16``, dropout without ``rows_dropout`` or with a module
that is not ``nn.Dropout``, a multicomponent model).

GPU: ``MPNN(AtomMessagePassing, NormAggregation, RegressionFFN, batch_norm=True)`` and its deep copy — three ``FusedTrainer.step``
against three steps of ``loss().backward()`` + ``FlatAdam`` on the copy: on the tile home (64 QM9-shaped molecules, ReLU: the module
path runs the same tile kernels, so no decision can differ), on the general home (8 forty-atom molecules mixed with QM9-shaped ones,
tanh) and with ``p = 0.2`` (tanh; the module path's ``nn.Dropout`` replays the hash masks of the step's seed, as
``tests/test_rows_dropout_gpu.py`` does).  Then: validated against tile-plan batches, the staged step against the one-call step,
``HipMPNN`` under the Trainer stand-in.

The bar: ``err = max|a - b| / max|b|`` per tensor (every loss, every parameter after the last step) within
``min(MARGIN max(e32, 2**-23), cap)``, caps 1e-5 (loss) and 2e-5 (parameters).  The yardstick ``e32`` is what float32 itself does to
the same quantity: the same training steps restated on the CPU (``atom_harness.train_ref``: the block, the aggregation, the batch
norm, the predictor, MSE, ``torch.optim.Adam``) from the same parameters, in float32 against float64 — a parameter that starts at
zero and moves by a few ``lr`` (``bn.bias``), or a gradient that is a sum of cancelling terms, is as uncertain in float32 as the
yardstick says, whatever kernel computes it.  Adam runs with ``lr = 0.05``, ``eps = 1`` on every side: its update
``lr m / (sqrt(v) + eps)`` turns a gradient error of ``d max|g|`` into an update error of up to ``d max|g| / eps`` of the largest
update — for an entry with ``|g|`` below ``eps`` the normalisation divides the error by ``eps``, not by ``|g|`` — so with the
default 1e-8 (or 1e-4: the gradients here reach 0.2) the comparison measures rounding noise through an amplifier of 10^3 .. 10^7, not
kernels; with ``eps = 1`` the amplification is at most 1 and every parameter still moves by ``0.05 g``, far above the bar.  The
CPU test asserts that float32 meets the caps.

MARGIN: the worst ``err / max(e32, 2**-23)`` over this module's comparisons on the MI355X is 1.45 (``message_passing.W_h.weight`` of
``general-qm9x64-tanh-p0.2``; 1.42 and 1.41 on ``general-40atoms-tanh`` follow; the tile home 0.98, validated against tile plan 0.75,
the staged general step is the one-call step bit for bit); doubled and rounded up to a power of two: 4.
"""
import copy

import numpy as np
import pytest
import torch

import atom_harness as ah
from conftest import parity_err_unfloored
from test_multicomponent_integration import stub_chemprop  # noqa: F401  (the fixture)

MARGIN = 4.0
EPS32 = 2.0 ** -23
CAP = dict(loss=1e-5, param=2e-5)
ADAM = dict(lr=0.05, eps=1.0)
gpu = pytest.mark.gpu


def _atom(**kw):
    from chemprop_amd.nn import AtomMessagePassing

    return AtomMessagePassing(**kw)


# ---- CPU -----------------------------------------------------------------------------------------------------------------------------
def test_defaults_still_refuse_an_atom_block():
    from chemprop_amd import agg as cagg
    from chemprop_amd.model import MPNN, FusedTrainer, RegressionFFN, fused_block, is_atom_block

    mp = _atom(d_h=64)
    assert is_atom_block(mp)
    with pytest.raises(NotImplementedError, match="BondMessagePassing"):
        fused_block(mp)
    with pytest.raises(NotImplementedError, match="BondMessagePassing"):
        fused_block(mp, rows_dropout=True, vd_dropout=True)
    with pytest.raises(NotImplementedError, match="BondMessagePassing"):
        FusedTrainer(MPNN(mp, cagg.NormAggregation(), RegressionFFN(input_dim=64)))


def test_atom_messages_takes_the_block_with_the_bond_blocks_activation():
    from chemprop_amd.model import fused_block, is_atom_block
    from chemprop_amd.nn import BondMessagePassing

    for kw in (dict(), dict(activation="tanh"), dict(activation="leakyrelu", bias=True), dict(activation="elu", d_h=324, depth=1), dict(d_e=1), dict(d_e=16)):
        bond_kw = {k: v for k, v in kw.items() if k != "d_e"}
        assert fused_block(_atom(**kw), atom_messages=True) == fused_block(BondMessagePassing(**bond_kw)), kw
    assert fused_block(_atom(), atom_messages=True)[0] == "relu"
    assert fused_block(_atom(dropout=0.2, activation="tanh"), rows_dropout=True, atom_messages=True)[0] == "tanh"
    assert not is_atom_block(BondMessagePassing())
    assert fused_block(BondMessagePassing(), atom_messages=True) == fused_block(BondMessagePassing())   # (a bond block: as before)


def test_atom_messages_refusals():
    from chemprop_amd import agg as cagg
    from chemprop_amd.model import MPNN, FusedTrainer, MulticomponentMPNN, RegressionFFN, fused_block
    from chemprop_amd.nn import MulticomponentMessagePassing

    class OtherDropout(torch.nn.Dropout):
        pass

    odd = _atom(dropout=0.2)
    odd.dropout = OtherDropout(0.2)
    for mp, why in ((_atom(undirected=True), "directed"), (_atom(activation="prelu"), "PReLU"), (_atom(d_vd=3), "W_d"), (_atom(d_e=17), "d_e"),
                    (_atom(d_e=28), "d_e"), (_atom(dropout=0.2), "rows_dropout"), (odd, "nn.Dropout")):
        with pytest.raises(NotImplementedError, match=why):
            fused_block(mp, atom_messages=True, rows_dropout=mp is odd)
    for flag in (False, True):
        blocks = [_atom(d_h=32), _atom(d_h=32)]
        model = MulticomponentMPNN(MulticomponentMessagePassing(blocks, 2), cagg.NormAggregation(), RegressionFFN(input_dim=64))
        with pytest.raises(NotImplementedError):
            FusedTrainer(model, atom_messages=flag)


def test_float32_meets_the_caps_on_every_step_comparison():
    """The yardstick of every comparison below (the CPU restatement of the training steps, float32 against float64) is under the
    caps: the bar is one a correct kernel can meet.  (Dropout: one fixed seed per step.)"""
    todo = [(cid, kind, kw, p, 3) for cid, kind, kw, p, _, _ in STEP_CASES]
    todo += [("validated-vs-tile-plan", "qm9x64", dict(d_h=64, activation="tanh"), 0.0, 1), ("staged-general", "mixed40", dict(d_h=64, activation="tanh"), 0.0, 3)]
    for cid, kind, kw, p, steps in todo:
        e32 = _yardstick(_model("cpu", **kw), kind, steps, p, seeds=[101, 202, 303])
        for k, e in e32.items():
            assert e < CAP["loss" if k.startswith("loss") else "param"], (cid, k, e)


# ---- GPU: the step against the module path -------------------------------------------------------------------------------------------
def _model(dev, seed=3, **kw):
    from chemprop_amd import agg as cagg
    from chemprop_amd.model import MPNN, RegressionFFN

    torch.manual_seed(seed)
    mp = _atom(**kw)
    d_h = mp.W_o.out_features
    return MPNN(mp, cagg.NormAggregation(), RegressionFFN(n_tasks=2, input_dim=d_h, hidden_dim=64, activation=kw.get("activation", "relu")),
                batch_norm=True).to(dev).train()


def _cpu_batch(kind, seed=21):
    from chemprop_amd import synth
    from chemprop_amd.data import BatchMolGraph

    if kind == "qm9x64":
        bmg = synth.random_batch(64, "qm9", seed=seed)
    else:   # 8 forty-atom molecules among 16 QM9-shaped ones
        big, small = synth.random_molgraphs(8, "synth40", seed=seed), synth.random_molgraphs(16, "qm9", seed=seed + 1)
        bmg = BatchMolGraph([m for i in range(8) for m in (small[2 * i], big[i], small[2 * i + 1])])
    return bmg, torch.randn(len(bmg), 2, generator=torch.Generator().manual_seed(seed + 2))


def _batch(kind, dev, seed=21):
    bmg, y = _cpu_batch(kind, seed)
    return ah.on_device(bmg, dev), y.to(dev)


def _yardstick(model, kind, steps, p=0.0, seeds=None):
    """``e32`` of every loss and every parameter after ``steps`` steps from ``model``'s CURRENT parameters: the CPU restatement in
    float32 against float64 (``seeds``: the dropout seeds of the steps)."""
    from oracle import dropout_hash as dh

    bmg, y = _cpu_batch(kind)
    nV, nE, d_h, depth = int(bmg.V.shape[0]), int(bmg.E.shape[0]), model.message_passing.W_o.out_features, model.message_passing.depth
    keeps_of = None
    if p > 0:
        keeps_of = lambda i: ([torch.from_numpy(dh.keep_mask(seeds[i], t, nE, d_h, p)) for t in range(depth - 1)]
                              + [torch.from_numpy(dh.keep_mask(seeds[i], depth - 1, nV, d_h, p))])
    runs = [ah.train_ref(model, bmg, y, steps, dt, keeps_of=keeps_of, p=p, **ADAM) for dt in (torch.float64, torch.float32)]
    e32 = {f"loss[{i}]": abs(runs[1][0][i] - runs[0][0][i]) / abs(runs[0][0][i]) for i in range(steps)}
    for k, v in runs[0][1].items():
        e32[k] = parity_err_unfloored(runs[1][1][k].double().numpy(), v.numpy())
    return e32


def _bar(name, a, b, kind, e32, worst):
    err = parity_err_unfloored(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64))
    bar = min(MARGIN * max(e32, EPS32), CAP[kind])
    ratio = err / max(e32, EPS32)
    worst[0] = max(worst[0], ratio)
    print(f"ATOMBAR step {name} err={err:.3e} e32={e32:.3e} ratio={ratio:.2f} bar={bar:.3e}")
    return [] if err <= bar else [f"{name}: err {err:.3e} > bar {bar:.3e} (fp32 yardstick {e32:.3e}, ratio {ratio:.1f})"]


def _compare_models(tag, a, b, losses_a, losses_b, e32):
    worst, fails = [0.0], []
    for i, (x, z) in enumerate(zip(losses_a, losses_b)):
        fails += _bar(f"{tag} loss[{i}]", [x], [z], "loss", e32[f"loss[{i}]"], worst)
    for (k, pa), (_, pb) in zip(a.named_parameters(), b.named_parameters()):
        fails += _bar(f"{tag} {k}", pa.detach().cpu().numpy(), pb.detach().cpu().numpy(), "param", e32[k], worst)
    print(f"ATOMBAR step {tag} worst-ratio={worst[0]:.2f}")
    assert not fails, "; ".join(fails)


def _module_steps(b, bmg, y, n, before_step=None):
    from chemprop_amd import distributed as ddp
    from chemprop_amd.optim import FlatAdam

    sync = ddp.GradSync(list(b.parameters()), modules=[b])
    opt = FlatAdam(sync, **ADAM)
    losses = []
    for i in range(n):
        if before_step is not None:
            before_step(i)
        l = b.loss(bmg, y)
        l.backward()
        sync.allreduce()
        opt.step()
        sync.zero_grad()
        losses.append(float(l))
    return losses


STEP_CASES = [("tile-qm9x64-relu", "qm9x64", dict(d_h=64), 0.0, "mega16", "mega16/atom"),
              ("general-40atoms-tanh", "mixed40", dict(d_h=64, activation="tanh", bias=True), 0.0, "general16", "rows/atom"),
              ("general-40atoms-tanh-h300-depth2", "mixed40", dict(d_h=300, depth=2, activation="tanh"), 0.0, "general16", "rows/atom"),
              ("general-qm9x64-tanh-p0.2", "qm9x64", dict(d_h=64, activation="tanh", dropout=0.2), 0.2, "general16", "rows/atom")]


@gpu
@pytest.mark.parametrize("cid,kind,kw,p,route,module_route", STEP_CASES, ids=[c[0] for c in STEP_CASES])
def test_atom_step_equals_the_module_path(cid, kind, kw, p, route, module_route, gpu_device):
    from chemprop_amd import _lib
    from chemprop_amd.model import FusedTrainer
    from oracle import dropout_hash as dh
    from test_dropout_gpu import ReplayDropout

    dev = gpu_device
    a = _model(dev, **kw)
    b, start = copy.deepcopy(a), copy.deepcopy(a)
    bmg, y = _batch(kind, dev)
    nV, nE, d_h, depth = int(bmg.V.shape[0]), int(bmg.E.shape[0]), a.message_passing.W_o.out_features, a.message_passing.depth
    with pytest.raises(NotImplementedError):
        FusedTrainer(copy.deepcopy(a), rows_dropout=True)
    tr = FusedTrainer(a, rows_dropout=True, atom_messages=True, **ADAM)
    la, seeds = [], []
    for i in range(3):
        la.append(float(tr.step(bmg, y)[0]))
        assert tr.last_route == route, (i, tr.last_route)
        seeds.append(getattr(tr, "last_dropout_seed", None))
        if route == "mega16":
            assert tr._last_plan_tiles == (i >= 2), i   # (the first, validated batches on the full plan, then the tile plan)
    part = tr._block_args(tr.mp, bmg, len(bmg), tr.acts[0], False, None, None) if p == 0 else None
    assert part is None or (part.st.args.flags & _lib.F_ATOM and part.route == route)

    def replay(i):   # the module path's nn.Dropout replays the hash masks of the step's seed, at the kernels' float scale
        keeps = [dh.keep_mask(seeds[i], t, nE, d_h, p) for t in range(depth - 1)] + [dh.keep_mask(seeds[i], depth - 1, nV, d_h, p)]
        b.message_passing.dropout = ReplayDropout(p, [torch.from_numpy(k).to(dev).float() * ah.scale32(p) for k in keeps])

    lb = _module_steps(b, bmg, y, 3, replay if p > 0 else None)
    assert b.message_passing.__dict__.get("_dmpnn_route") == module_route
    torch.cuda.synchronize()
    _compare_models(cid, a, b, la, lb, _yardstick(start, kind, 3, p, seeds))
    assert int(a.bn.num_batches_tracked) == int(b.bn.num_batches_tracked) == 3


@gpu
def test_atom_step_validated_and_tile_plan_batches_agree(gpu_device, monkeypatch):
    """One step from the same state on a launched, validated full plan and on the tile plan built inside the call: the same step."""
    from chemprop_amd.model import FusedTrainer

    a = _model(gpu_device, d_h=64, activation="tanh")
    b = copy.deepcopy(a)
    e32 = _yardstick(a, "qm9x64", 1)
    bmg, y = _batch("qm9x64", gpu_device)
    ta = FusedTrainer(a, atom_messages=True, **ADAM)
    la = float(ta.step(bmg, y)[0])
    assert ta.last_route == "mega16" and not ta._last_plan_tiles and ta._checked == 1
    monkeypatch.setenv("DMPNN_VALIDATE", "never")
    tb = FusedTrainer(b, atom_messages=True, **ADAM)
    lb = float(tb.step(bmg, y)[0])
    assert tb.last_route == "mega16" and tb._last_plan_tiles and tb._checked == 0
    torch.cuda.synchronize()
    _compare_models("validated-vs-tile-plan", a, b, [la], [lb], e32)


@gpu
@pytest.mark.parametrize("kind,kw", [("qm9x64", dict(d_h=64)), ("mixed40", dict(d_h=64, activation="tanh"))], ids=["tile", "general"])
def test_atom_staged_step_equals_the_one_call_step(kind, kw, gpu_device, monkeypatch):
    from chemprop_amd.model import FusedTrainer

    a = _model(gpu_device, **kw)
    b = copy.deepcopy(a)
    e32 = _yardstick(a, kind, 3)
    bmg, y = _batch(kind, gpu_device)
    ta = FusedTrainer(a, atom_messages=True, **ADAM)
    la = [float(ta.step(bmg, y)[0]) for _ in range(3)]
    monkeypatch.setenv("DMPNN_FORCE_COLLECTIVE", "1")
    tb = FusedTrainer(b, atom_messages=True, **ADAM)
    lb = [float(tb.step(bmg, y)[0]) for _ in range(3)]
    assert ta.last_route == tb.last_route == ("mega16" if kind == "qm9x64" else "general16")
    torch.cuda.synchronize()
    _compare_models(f"staged-{kind}", b, a, lb, la, e32)


@gpu
def test_atom_step_refuses_before_a_seed_is_drawn(gpu_device):
    """Dropout with an odd ``d_v`` (the finalize would leave the f16 pipe): ``NotImplementedError`` from the step, torch's generator
    untouched, nothing updated."""
    from chemprop_amd import synth
    from chemprop_amd.model import FusedTrainer

    a = _model(gpu_device, d_v=71, d_h=64, activation="tanh", dropout=0.2)
    bmg = synth.random_batch(16, "qm9", seed=2, d_v=71)
    bmg.to(gpu_device)
    y = torch.randn(16, 2, device=gpu_device)
    tr = FusedTrainer(a, rows_dropout=True, atom_messages=True)
    before = [p.detach().clone() for p in a.parameters()]
    rng = torch.get_rng_state()
    with pytest.raises(NotImplementedError, match="odd d_v"):
        tr.step(bmg, y)
    assert torch.equal(torch.get_rng_state(), rng) and tr.opt.steps == 0
    assert all(torch.equal(p, q) for p, q in zip(a.parameters(), before))


@gpu
def test_hip_mpnn_takes_an_atom_block_on_the_fused_step(stub_chemprop, gpu_device):  # noqa: F811
    """``HipMPNN`` with the reference's ``AtomMessagePassing`` under the Trainer stand-in reports a ``fused:`` route, not the module
    path, and moves the parameters."""
    import types

    from chemprop_amd.model import RegressionFFN

    S = stub_chemprop
    integ = S.integration
    integ.enable()
    HipM = integ.hip_mpnn_class()[1] if isinstance(integ.hip_mpnn_class(), tuple) else integ.hip_mpnn_class()
    torch.manual_seed(3)
    mp = S.mods["chemprop.nn"].AtomMessagePassing(d_h=64)
    model = HipM(mp, S.mods["chemprop.nn"].NormAggregation(), RegressionFFN(input_dim=64), batch_norm=True, init_lr=1e-3).to(gpu_device).train()
    opt = model.configure_optimizers()["optimizer"]
    model._trainer = types.SimpleNamespace(optimizers=[opt], accumulate_grad_batches=1, gradient_clip_val=None, gradient_clip_algorithm=None,
                                           strategy=None)
    bmg, y = _batch("qm9x64", gpu_device)
    before = model.message_passing.W_h.weight.detach().clone()
    for i in range(3):
        opt.step(lambda i=i: model.training_step((bmg, None, None, y[:, :1].contiguous(), None, None, None), i))
        assert model.__dict__["_hip"]["route"] == "fused:mega16", model.__dict__["_hip"]
    torch.cuda.synchronize()
    assert not torch.equal(model.message_passing.W_h.weight.detach(), before)
