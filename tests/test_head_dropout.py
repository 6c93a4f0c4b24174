"""The predictor's dropout (``chemprop train --dropout p``: ``MLP.build``'s shared ``nn.Dropout`` between ``tau`` and every Linear
layer after the first) on the head kernels and the one-call training step: ``dmpnn_head_args.ffn_dropout_p / ffn_dropout_seed``, a
hash mask regenerated in the backward pass (``include/dmpnn.h``); the four-launch row form and the chain form of
``csrc/dmpnn_head.hip`` (kernels: ``csrc/dmpnn_head_kernels.hpp``); ``HeadSpec`` / ``FusedTrainer(ffn_dropout=True)``; ``integration.HipMPNN``'s step.

Parity of a stochastic op is parity given its mask: the tests rebuild the head's masks from the seed with the oracle's restatement
of the hash and replay them in a float64 restatement."""
import copy
import ctypes as C

import numpy as np
import pytest
import torch
from torch import nn

from chemprop_amd import _lib
from conftest import parity_err, parity_err_unfloored
from oracle import dropout_hash as dh
from test_multicomponent_integration import _fake_trainer, stub_chemprop  # noqa: F401  (the stand-in chemprop and its fixture)


# ---- the mask, restated -------------------------------------------------------------------------------------------------------------
def ffn_keep(seed, layer, n_rows, N, p):
    """Boolean ``[n_rows, N]``: True where element (r, c) of layer ``layer``'s input is kept — site DROP_SITE_FFN + layer, hash row
    r ceil(N / 1024) + c // 1024, hash column c % 1024 (dmpnn.h, ``ffn_dropout_p``)."""
    nblk = -(-N // 1024)
    keep = np.empty((n_rows, N), dtype=bool)
    rows, thr = np.arange(n_rows), np.uint32(dh.threshold(p))
    for b in range(nblk):
        c0, c1 = 1024 * b, min(N, 1024 * (b + 1))
        keep[:, c0:c1] = dh.drop_hash(seed, _lib.DROP_SITE_FFN + layer, rows * nblk + b, np.arange(c1 - c0)) >= thr
    return keep


# ---- helpers ---------------------------------------------------------------------------------------------------------------------
def make_model(d_h, hidden, tasks, p, kind="mse", act="relu", n_layers=1, bn=True, agg="norm", n_comp=1):
    from chemprop_amd import agg as cagg
    from chemprop_amd.model import (BCE, CE, MPNN, MSE, MVE, BinaryClassificationFFN, MulticlassClassificationFFN, MulticomponentMPNN,
                                    MveFFN, RegressionFFN)
    from chemprop_amd.nn import BondMessagePassing, MulticomponentMessagePassing

    if n_comp > 1:
        mp = MulticomponentMessagePassing([BondMessagePassing(d_h=d_h, activation=act) for _ in range(n_comp)], n_comp)
    else:
        mp = BondMessagePassing(d_h=d_h, activation=act)
    ag = dict(norm=cagg.NormAggregation, mean=cagg.MeanAggregation, sum=cagg.SumAggregation)[agg]()
    ffn = dict(n_tasks=tasks, input_dim=mp.output_dim, hidden_dim=hidden, n_layers=n_layers, dropout=p, activation=act)
    if kind == "bce":
        pred = BinaryClassificationFFN(criterion=BCE(1.0), **ffn)
    elif kind == "ce":
        pred = MulticlassClassificationFFN(3, criterion=CE(1.0), **ffn)
    elif kind == "mve":
        pred = MveFFN(criterion=MVE(1.0), **ffn)
    else:
        pred = RegressionFFN(criterion=MSE(1.0), **ffn)
    return (MulticomponentMPNN if n_comp > 1 else MPNN)(mp, ag, pred, batch_norm=bn)


def run_head(model, Hvs, batches, n, T, w, seed):
    """ONE ``dmpnn_head`` call (forward + backward, ``bn_training``) with the predictor's dropout at ``seed``; ``Hvs`` / ``batches``:
    one per component (merged into one H_v and the batch vector ``c n + i``).  Returns (loss, preds, {param id: grad}, gH_v)."""
    from chemprop_amd import engine
    from chemprop_amd.model import HeadSpec

    lib = _lib.load()
    spec = HeadSpec(model, ffn_dropout=True)
    dev = Hvs[0].device
    Hv = torch.cat(Hvs).contiguous()
    batch = torch.cat([b + c * n for c, b in enumerate(batches)]).contiguous()
    grads = {id(p): torch.zeros_like(p) for p in spec.params()}
    h = _lib.HeadArgs()
    nV, d = int(Hv.shape[0]), int(Hv.shape[1])
    keep = spec.fill(h, nV, n, d, batch, T, w, None, None, lambda p: None if p is None else grads[id(p)].data_ptr(),
                     ffn_dropout=(spec.drop.p, seed))
    preds = torch.full((n, spec.n_out), float("nan"), device=dev)
    loss = torch.empty(2, device=dev)
    gH = torch.full((nV, d), float("nan"), device=dev)
    h.preds, h.loss_out, h.gHv, h.ldg = preds.data_ptr(), loss.data_ptr(), gH.data_ptr(), d
    nb = int(lib.dmpnn_head_ws_bytes(C.byref(h)))
    ws = torch.empty(nb, dtype=torch.uint8, device=dev)
    h.ws, h.ws_bytes = ws.data_ptr(), nb
    with engine._OnDevice(dev):
        _lib.check(lib.dmpnn_head(C.byref(h), Hv.data_ptr(), Hv.stride(0), engine._stream_ptr(dev)), "dmpnn_head")
    torch.cuda.synchronize()
    del keep
    return float(loss[0]), preds.cpu(), {k: g.cpu() for k, g in grads.items()}, gH.cpu()


def restate(model, Hvs, batches, n, T, w, seed, p, zs=None):
    """The head in float64 on the CPU, op by op, with the predictor's masks replayed: agg, BatchNorm1d (training), the MLP
    ``(tau, mask / (1 - p), Linear)``, the criterion.  Returns (loss, raw outputs, {param id: grad}, gH_v); ``zs`` (a list) receives
    the pre-activations of the hidden layers."""
    from chemprop_amd.model import MODES, HeadSpec, masked_loss

    spec = HeadSpec(model, ffn_dropout=True)
    f = lambda t: t.detach().cpu().double()
    mode = {v: k for k, v in MODES.items()}[spec.agg_mode]
    Hv64 = f(torch.cat(Hvs)).requires_grad_()
    Hs, row = [], 0
    for b in batches:
        b = b.cpu()
        H = torch.zeros(n, Hv64.shape[1], dtype=torch.float64).index_add(0, b, Hv64[row:row + b.numel()])
        row += b.numel()
        if mode == "mean":
            H = H / torch.bincount(b, minlength=n).clamp(min=1).double().view(-1, 1)
        elif mode == "norm":
            H = H / spec.agg_norm
        Hs.append(H)
    H = torch.cat(Hs, 1)
    leaves = {}
    if spec.bn is not None:
        bw, bb = f(spec.bn.weight).requires_grad_(), f(spec.bn.bias).requires_grad_()
        rm, rv = f(spec.bn.running_mean).clone(), f(spec.bn.running_var).clone()
        H = torch.nn.functional.batch_norm(H, rm, rv, bw, bb, training=True, momentum=spec.bn.momentum, eps=spec.bn.eps)
        leaves[id(spec.bn.weight)], leaves[id(spec.bn.bias)] = bw, bb
    Z = H
    for i, blk in enumerate(model.predictor.ffn):
        lin = blk[-1]
        if i > 0:
            m = torch.from_numpy(ffn_keep(seed, i, n, Z.shape[1], p)).double() / (1.0 - p)
            Z = blk[0](Z) * m
        W = f(lin.weight).requires_grad_()
        leaves[id(lin.weight)] = W
        bias = None
        if lin.bias is not None:
            bias = f(lin.bias).requires_grad_()
            leaves[id(lin.bias)] = bias
        Z = torch.nn.functional.linear(Z, W, bias)
        if zs is not None and i + 1 < len(model.predictor.ffn):
            zs.append(Z.detach())
    Y = Z
    if spec.kind == "ce":
        P = Y.reshape(n, -1, spec.n_classes)
    elif spec.kind == "mve":
        mean, var = torch.chunk(Y, 2, 1)
        P = torch.stack((mean, torch.nn.functional.softplus(var)), 2)
    else:
        P = Y
    l = masked_loss(P, f(T), None if w is None else f(w), None, None, None, spec.kind)
    l.backward()
    return float(l.detach()), Y.detach(), {k: v.grad for k, v in leaves.items()}, Hv64.grad


def unkink(model, Hvs, batches, n, T, w, seed, p):
    """ReLU / LeakyReLU: a float64 reference cannot vouch for an entry whose pre-activation lies within fp32 rounding of 0 (the
    kernel's mask may differ there, and one flipped unit moves a batch-mean gradient by ~1e-4 of its largest entry).  Layer by layer
    the hidden biases are shifted per unit by the smallest amount that leaves ``min |z| >= 1e-4 max|z|`` in the float64
    pre-activations (``head_harness._unkink_bias``); asserted for the final parameters.  Nothing is excluded from the comparison."""
    from head_harness import _unkink_bias

    hidden = [blk[-1] for blk in model.predictor.ffn][:-1]
    for l, lin in enumerate(hidden):
        zs = []
        restate(model, Hvs, batches, n, T, w, seed, p, zs)
        s = _unkink_bias(zs[l], 2e-4 * float(zs[l].abs().max()))
        with torch.no_grad():
            lin.bias.copy_((lin.bias.detach().cpu().double() + s).float())
    zs = []
    restate(model, Hvs, batches, n, T, w, seed, p, zs)
    for z in zs:
        assert float(z.abs().min()) >= 1e-4 * float(z.abs().max())


CASES = {
    # (DMPNN_HEAD, n_components, molecules, d_h, hidden, tasks, ffn n_layers, criterion, activation, p)
    "rows-512-mse-relu-0.1": ("rows", 1, 512, 300, 300, 1, 1, "mse", "relu", 0.1),
    "rows-512-mse-tanh-0.5": ("rows", 1, 512, 300, 300, 1, 1, "mse", "tanh", 0.5),
    "rows-512-bce-relu-0.5": ("rows", 1, 512, 300, 300, 2, 1, "bce", "relu", 0.5),
    "rows-512-bce-tanh-0.1": ("rows", 1, 512, 300, 300, 2, 1, "bce", "tanh", 0.1),
    "chain-2048-ce-leakyrelu-0.1": ("chain", 1, 2048, 300, 2048, 1, 2, "ce", "leakyrelu", 0.1),
    "chain-2048-mve-leakyrelu-0.5": ("chain", 1, 2048, 300, 2048, 1, 2, "mve", "leakyrelu", 0.5),
    "2-components-256-mse-relu-0.1": (None, 2, 256, 64, 96, 2, 1, "mse", "relu", 0.1),
    "2-components-256-bce-elu-0.5": ("chain", 2, 256, 64, 96, 2, 2, "bce", "elu", 0.5),
}


def case_inputs(case, dev, seed=0):
    from chemprop_amd import synth

    _, n_comp, n, d_h, hidden, tasks, n_layers, kind, act, p = case
    torch.manual_seed(seed + 5)
    model = make_model(d_h, hidden, tasks, p, kind, act, n_layers, n_comp=n_comp).to(dev).train()
    with torch.no_grad():   # (non-trivial batch-norm parameters)
        model.bn.weight.uniform_(0.5, 1.5), model.bn.bias.uniform_(-0.5, 0.5)
    gen = torch.Generator().manual_seed(seed + 2)
    bmgs = [synth.random_batch(n, "qm9", seed=seed + 9 + c) for c in range(n_comp)]
    Hvs = [torch.randn(int(b.V.shape[0]), d_h, generator=gen).to(dev) for b in bmgs]
    batches = [b.batch.to(dev) for b in bmgs]
    if kind == "bce":
        T = torch.rand(n, tasks, generator=gen).round()
    elif kind == "ce":
        T = torch.randint(0, 3, (n, tasks), generator=gen).float()
    else:
        T = torch.randn(n, tasks, generator=gen)
    if tasks > 1:
        T[torch.rand(n, tasks, generator=gen) < 0.2] = float("nan")
    w = 0.5 + torch.rand(n, 1, generator=gen)
    return model, Hvs, batches, n, T.to(dev), w.to(dev)


# ---- GPU: the head ------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_head_with_ffn_dropout_matches_float64_restatement(name, gpu_device, monkeypatch):
    """``dmpnn_head`` with ``ffn_dropout_p``: loss, raw predictions, every ``gW`` / ``gb`` / batch-norm gradient and ``gH_v`` against
    the float64 restatement with the hash masks replayed.  Row cases under ``DMPNN_HEAD=rows`` (a shape that would take the chain is
    an error there), chain cases under ``=chain``."""
    case = CASES[name]
    if case[0]:
        monkeypatch.setenv("DMPNN_HEAD", case[0])
    model, Hvs, batches, n, T, w = case_inputs(case, gpu_device)
    p, seed = case[-1], 0x5EED0000 + 77 * len(name)
    if case[-2] in ("relu", "leakyrelu"):
        unkink(model, Hvs, batches, n, T, w, seed, p)
    ref_loss, ref_P, ref_g, ref_gH = restate(model, Hvs, batches, n, T, w, seed, p)
    loss, P, g, gH = run_head(model, Hvs, batches, n, T, w, seed)
    assert abs(loss - ref_loss) <= 1e-5 * max(1.0, abs(ref_loss)), (loss, ref_loss)
    assert parity_err(P.numpy(), ref_P.numpy()) <= 2e-5
    from chemprop_amd.model import HeadSpec

    spec = HeadSpec(model, ffn_dropout=True)
    names = {id(q): k for k, q in model.named_parameters()}
    assert len(ref_g) == len(spec.params())
    for q in spec.params():
        assert torch.isfinite(g[id(q)]).all(), names[id(q)]
        e = parity_err(g[id(q)].numpy(), ref_g[id(q)].numpy())
        assert e <= 2e-5, f"{names[id(q)]}: {e:.2e}"
        # (gradients of a loss that is a batch mean: max|ref| << 1, the floored bar is an absolute one — hold the relative one beside it)
        eu = parity_err_unfloored(g[id(q)].numpy(), ref_g[id(q)].numpy())
        print(f"{name} {names[id(q)]}: floored {e:.2e}, un-floored {eu:.2e}")
        assert eu <= 2e-5, f"{names[id(q)]}: un-floored {eu:.2e}"
    assert parity_err(gH.numpy(), ref_gH.numpy()) <= 2e-5
    eu = parity_err_unfloored(gH.numpy(), ref_gH.numpy())
    print(f"{name} gH_v: un-floored {eu:.2e}")
    assert eu <= 2e-5, f"gH_v: un-floored {eu:.2e}"
    # the mask is live: a different seed gives a different result
    _, P2, _, _ = run_head(model, Hvs, batches, n, T, w, seed + 1)
    assert not torch.equal(P, P2)


@pytest.mark.gpu
@pytest.mark.parametrize("name", [k for k, v in CASES.items() if v[0] == "rows"])
def test_head_rows_form_equals_chain_with_ffn_dropout(name, gpu_device, monkeypatch):
    """The four-launch row form and the chain form under one seed: the same masks, the same function."""
    case = CASES[name]
    seed = 12345
    a = case_inputs(case, gpu_device)
    b = case_inputs(case, gpu_device)
    monkeypatch.setenv("DMPNN_HEAD", "rows")
    la, Pa, ga, gHa = run_head(*a, seed)
    monkeypatch.setenv("DMPNN_HEAD", "chain")
    lb, Pb, gb, gHb = run_head(*b, seed)
    assert abs(la - lb) <= 2e-6 * max(1.0, abs(lb)), (la, lb)
    assert parity_err(Pa.numpy(), Pb.numpy()) <= 1e-5
    for x, y in zip(a[0].parameters(), b[0].parameters()):
        if id(x) in ga:
            assert parity_err(ga[id(x)].numpy(), gb[id(y)].numpy()) <= 1e-5
            assert parity_err_unfloored(ga[id(x)].numpy(), gb[id(y)].numpy()) <= 1e-5
    assert parity_err(gHa.numpy(), gHb.numpy()) <= 1e-5
    assert parity_err_unfloored(gHa.numpy(), gHb.numpy()) <= 1e-5


# ---- GPU: the one-call step ---------------------------------------------------------------------------------------------------------
def _qm9(n, dev, seed=1):
    from chemprop_amd import synth

    bmg = synth.random_batch(n, "qm9", seed=seed)
    bmg.to(dev)
    gen = torch.Generator().manual_seed(seed + 1)
    return bmg, torch.randn(n, 1, generator=gen).to(dev), (0.5 + torch.rand(n, 1, generator=gen)).to(dev)


def _step_model(p_block, p_ffn, dev, seed=11, act="relu"):
    from chemprop_amd import agg as cagg
    from chemprop_amd.model import MPNN, RegressionFFN
    from chemprop_amd.nn import BondMessagePassing

    torch.manual_seed(seed)
    mp = BondMessagePassing(dropout=p_block, activation=act)
    return MPNN(mp, cagg.NormAggregation(), RegressionFFN(input_dim=mp.output_dim, dropout=p_ffn, activation=act), batch_norm=True).to(dev).train()


@pytest.mark.gpu
def test_fused_step_with_block_and_predictor_dropout_given_the_masks(gpu_device):
    """``FusedTrainer(model, ffn_dropout=True)``, p = 0.1 in the block and in the predictor, one step at 512 QM9 molecules.  The block
    under the step's block seed (``last_dropout_seed``) is the module path's tile-kernel forward under the same seed (the block's own
    dropout parity given its masks: tests/test_dropout_gpu.py); behind it the head is restated in float64 with the head masks of
    ``last_head_dropout_seed`` replayed.  The step's loss and the gradient of every head parameter match that restatement; the block's
    gradients match the module path's backward from the restatement's dl/dH_v."""
    from chemprop_amd.model import FusedTrainer

    bmg, y, w = _qm9(512, gpu_device)
    a = _step_model(0.1, 0.1, gpu_device)
    b = copy.deepcopy(a)
    tr = FusedTrainer(a, lr=1e-3, ffn_dropout=True)
    torch.manual_seed(77)
    loss = tr.step(bmg, y, w)
    torch.cuda.synchronize()
    grads = {k: tr._views[id(q)].detach().cpu().clone() for k, q in a.named_parameters()}
    bseed, hseed = int(tr.last_dropout_seed), int(tr.last_head_dropout_seed)
    assert bseed != hseed and str(tr.last_route).startswith("mega16"), tr.last_route
    # the block's output under the step's block seed: the module path draws its seed the same way
    torch.manual_seed(77)
    out = b.message_passing(bmg)
    assert int(out.grad_fn.st.args.dropout_seed) == bseed
    ref_loss, _, ref_g, ref_gH = restate(b, [out.detach()], [bmg.batch], 512, y, w, hseed, 0.1)
    assert abs(float(loss[0]) - ref_loss) <= 1e-5 * max(1.0, abs(ref_loss)), (float(loss[0]), ref_loss)
    names = {id(q): k for k, q in b.named_parameters()}
    for pid, rg in ref_g.items():
        e = parity_err(grads[names[pid]].numpy(), rg.numpy())
        assert e <= 2e-5, f"{names[pid]}: {e:.2e}"
    out.backward(ref_gH.float().to(gpu_device))
    for k, q in b.message_passing.named_parameters():
        e = parity_err(grads["message_passing." + k].numpy(), q.grad.cpu().numpy())
        assert e <= 2e-5, f"{k}: {e:.2e}"


@pytest.mark.gpu
def test_fused_step_with_predictor_dropout_is_seeded_and_learns(gpu_device):
    """Three steps under one ``torch.manual_seed`` are bit-identical across two runs and differ under another seed; on a fittable
    target the loss falls over 60 steps."""
    from chemprop_amd.model import FusedTrainer

    bmg, y, w = _qm9(512, gpu_device)

    def run(seed):
        m = _step_model(0.1, 0.1, gpu_device)
        tr = FusedTrainer(m, lr=1e-3, ffn_dropout=True)
        torch.manual_seed(seed)
        losses = [float(tr.step(bmg, y, w)[0]) for _ in range(3)]
        torch.cuda.synchronize()
        return losses, torch.cat([q.detach().reshape(-1) for q in m.parameters()]).cpu()

    la, pa = run(5)
    lb, pb = run(5)
    lc, pc = run(6)
    assert la == lb and torch.equal(pa, pb)
    assert la != lc and not torch.equal(pa, pc)
    # a fittable target: a fixed function of the aggregated atom features
    m = _step_model(0.0, 0.1, gpu_device, seed=3)
    tr = FusedTrainer(m, lr=3e-3, ffn_dropout=True)
    target = torch.zeros(512, 1, device=gpu_device).index_add_(0, bmg.batch, bmg.V[:, :8].sum(1, keepdim=True))
    target = (target - target.mean()) / target.std()
    torch.manual_seed(0)
    losses = [float(tr.step(bmg, target)[0]) for _ in range(60)]
    assert np.mean(losses[-5:]) < 0.5 * np.mean(losses[:5]), (losses[:5], losses[-5:])


@pytest.mark.gpu
def test_predictor_dropout_in_eval_mode_passes_p0(gpu_device):
    """A predictor with p > 0 whose dropout is in eval mode (``model.predictor.eval()``) steps exactly like the same model built with
    p = 0: the head gets ``ffn_dropout_p = 0`` and no head seed is drawn."""
    from chemprop_amd.model import FusedTrainer

    bmg, y, w = _qm9(512, gpu_device)
    a, b = _step_model(0.0, 0.3, gpu_device), _step_model(0.0, 0.0, gpu_device)
    a.predictor.eval()
    ta, tb = FusedTrainer(a, lr=1e-3, ffn_dropout=True), FusedTrainer(b, lr=1e-3, ffn_dropout=True)
    for _ in range(2):
        la, lb = ta.step(bmg, y, w), tb.step(bmg, y, w)
        assert torch.equal(la, lb)
    torch.cuda.synchronize()
    assert not hasattr(ta, "last_head_dropout_seed")
    for (k, qa), (_, qb) in zip(a.named_parameters(), b.named_parameters()):
        assert torch.equal(qa, qb), k


@pytest.mark.gpu
def test_hip_mpnn_takes_the_one_call_step_with_predictor_dropout(stub_chemprop, gpu_device):
    """Through the stand-in ``chemprop``: a ``HipMPNN`` whose predictor has dropout 0.1 trains on the fused step (route ``fused:...``)
    and computes what ``FusedTrainer(ffn_dropout=True)`` computes on a copy of the model under the same seeds, over three steps."""
    from chemprop_amd.model import FusedTrainer, RegressionFFN

    S = stub_chemprop
    integ = S.integration
    integ.enable()
    HipM = integ.hip_mpnn_class()[1]
    torch.manual_seed(3)
    mp = S.cli.BondMessagePassing()
    a = HipM(mp, S.mods["chemprop.nn"].NormAggregation(), RegressionFFN(input_dim=mp.output_dim, dropout=0.1), batch_norm=True, init_lr=1e-3)
    a = a.to(gpu_device).train()
    b = copy.deepcopy(a)
    bmg, y, w = _qm9(256, gpu_device, seed=4)
    opt = _fake_trainer(a)
    tr = FusedTrainer(b, lr=1e-3, ffn_dropout=True)
    for i in range(3):
        out = {}

        def closure(i=i):
            out["loss"] = a.training_step((bmg, None, None, y, w, None, None), i)
            return out["loss"]

        torch.manual_seed(100 + i)
        opt.step(closure)
        assert a.__dict__["_hip"]["route"].startswith("fused:"), a.__dict__["_hip"]
        torch.manual_seed(100 + i)
        lb = float(tr.step(bmg, y, w)[0])
        assert a.__dict__["_hip"]["fused"].last_head_dropout_seed == tr.last_head_dropout_seed
        assert abs(float(out["loss"]) - lb) <= 1e-6 * max(1.0, abs(lb)), (i, float(out["loss"]), lb)
    torch.cuda.synchronize()
    for (k, pa), (_, pb) in zip(a.named_parameters(), b.named_parameters()):
        assert parity_err(pa.detach().cpu().numpy(), pb.detach().cpu().numpy()) <= 1e-6, k


# ---- no GPU -------------------------------------------------------------------------------------------------------------------------
def test_headspec_takes_predictor_dropout_only_when_asked():
    """``HeadSpec(model)`` still refuses a predictor with dropout; ``ffn_dropout=True`` takes the shared ``nn.Dropout`` and refuses a
    dropout module that is not ``nn.Dropout``."""
    from chemprop_amd.model import HeadSpec

    torch.manual_seed(0)
    model = make_model(64, 32, 1, 0.2, n_layers=2)
    with pytest.raises(NotImplementedError, match="dropout 0"):
        HeadSpec(model)
    spec = HeadSpec(model, ffn_dropout=True)
    assert type(spec.drop) is nn.Dropout and spec.drop.p == 0.2
    assert all(blk[1] is spec.drop for blk in list(model.predictor.ffn)[1:])
    assert HeadSpec(make_model(64, 32, 1, 0.0), ffn_dropout=True).drop.p == 0.0

    class OtherDropout(nn.Dropout):
        pass

    other = OtherDropout(0.2)
    for blk in list(model.predictor.ffn)[1:]:
        blk[1] = other
    with pytest.raises(NotImplementedError, match="nn.Dropout"):
        HeadSpec(model, ffn_dropout=True)


def test_head_refuses_ffn_dropout_outside_0_1_before_touching_the_device():
    """``ffn_dropout_p`` outside [0, 1) is ``DMPNN_EINVAL`` before anything reaches the device (no GPU here)."""
    lib = _lib.load()

    def call(p):
        h = _lib.HeadArgs()
        h.n_atoms, h.n_mols, h.d_h, h.n_layers = 9 * 64, 64, 300, 2
        for i, v in enumerate((300, 300, 1)):
            h.dims[i] = v
        h.ffn_dropout_p, h.ffn_dropout_seed = p, 7
        return int(lib.dmpnn_head(C.byref(h), 4096, 300, None)), lib.dmpnn_last_error_string().decode()

    for p in (1.0, 1.5, -0.1, float("nan")):
        rc, msg = call(p)
        assert rc == -1 and "ffn_dropout_p" in msg, (p, rc, msg)
    for p in (0.0, 0.5):   # (a valid p gets past that check and stops at the next one: no weights)
        rc, msg = call(p)
        assert rc == -1 and "no weight" in msg, (p, rc, msg)


@pytest.mark.parametrize("N", [300, 2048])
def test_mask_restatement_matches_the_library_hash(N):
    """The test's restatement of the head's mask equals ``dmpnn_dropout_keep`` at the mapped (site, row, col) element for element,
    and no two (molecule, column) pairs of a batch share a hash key (row * 1024 + col)."""
    lib = _lib.load()
    seed, p, layer = (0x0123456789ABCDEF, 0.3, 1)
    rows = [0, 1, 2, 511, 2047]
    keep = ffn_keep(seed, layer, max(rows) + 1, N, p)
    nblk = -(-N // 1024)
    for r in rows:
        lib_row = [lib.dmpnn_dropout_keep(C.c_uint64(seed), _lib.DROP_SITE_FFN + layer, r * nblk + c // 1024, c % 1024, C.c_float(p))
                   for c in range(N)]
        assert np.array_equal(keep[r], np.array(lib_row, dtype=bool)), r
    r = np.arange(2048, dtype=np.int64).reshape(-1, 1)
    c = np.arange(N, dtype=np.int64).reshape(1, -1)
    key = (r * nblk + c // 1024) * 1024 + c % 1024
    assert key.max() < 2 ** 32 and np.unique(key).size == key.size


@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("shape", [(512, 300), (2048, 2048)])
def test_dropped_fraction_is_p_within_5_sigma(p, shape):
    """The fraction of dropped elements of a layer's mask is p within binomial 5-sigma bounds."""
    n = shape[0] * shape[1]
    for seed, layer in ((1, 1), (2 ** 40 + 3, 2)):
        dropped = 1.0 - float(ffn_keep(seed, layer, *shape, p).mean())
        assert abs(dropped - p) <= 5 * np.sqrt(p * (1 - p) / n), (seed, layer, dropped)
