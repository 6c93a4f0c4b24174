"""Multicomponent models (``chemprop.models.MulticomponentMPNN``, ``nn/message_passing/multi.py``) on the head kernels and the
one-call step: the fingerprint ``cat([agg(H_v^c, bmg^c.batch) for c], 1)`` through batch norm, ``dmpnn_head_args.n_components``
(molecule ``i`` of component ``c`` is ``c B + i`` of the batch vector) and ``dmpnn_step_args.n_extra / extra`` (one block per
component) or the merged batch of a shared block (``data.merge_components``)."""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

from chemprop_amd import _lib
from conftest import parity_err, parity_err_unfloored


# ---- helpers ---------------------------------------------------------------------------------------------------------------------
def solvent_batch(n, d_v=72, d_e=14, seed=0):
    """``n`` single-atom molecules without bonds (water, a metal ion): every molecule's aggregate is its one atom's row."""
    from chemprop_amd.data import BatchMolGraph, MolGraph

    rng = np.random.default_rng(seed)
    return BatchMolGraph([MolGraph(rng.standard_normal((1, d_v)).astype(np.float32), np.zeros((0, d_e), np.float32),
                                   np.zeros((2, 0), np.int64), np.zeros(0, np.int64)) for _ in range(n)])


def make_multi(kinds, shared, d_h=300, hidden=300, tasks=1, bn=True, agg="norm", kind="mse", act="elu", d_xd=0, n_layers=1):
    from chemprop_amd import agg as cagg
    from chemprop_amd.model import BCE, CE, MSE, BinaryClassificationFFN, MulticlassClassificationFFN, MulticomponentMPNN, RegressionFFN
    from chemprop_amd.nn import BondMessagePassing, MulticomponentMessagePassing

    dims = dict(qm9=(72, 14), cgr=(106, 28), solvent=(72, 14))
    blocks = [BondMessagePassing(*dims[k], d_h=d_h, depth=3, activation=act) for k in (kinds[:1] if shared else kinds)]
    mp = MulticomponentMessagePassing(blocks, len(kinds), shared=shared)
    ag = dict(norm=cagg.NormAggregation, mean=cagg.MeanAggregation, sum=cagg.SumAggregation)[agg]()
    ffn = dict(n_tasks=tasks, input_dim=mp.output_dim + d_xd, hidden_dim=hidden, n_layers=n_layers, activation=act)
    if kind == "bce":
        pred = BinaryClassificationFFN(criterion=BCE(1.0), **ffn)
    elif kind == "ce":
        pred = MulticlassClassificationFFN(3, criterion=CE(1.0), **ffn)
    else:
        pred = RegressionFFN(criterion=MSE(1.0), **ffn)
    return MulticomponentMPNN(mp, ag, pred, batch_norm=bn)


def batches(kinds, n, dev=None, seed=0):
    from chemprop_amd import synth

    out = []
    for c, k in enumerate(kinds):
        b = solvent_batch(n, seed=seed + c) if k == "solvent" else synth.random_batch(n, k, seed=seed + 7 * c + 1)
        if dev is not None:
            b.to(dev)
        out.append(b)
    return out


def restate(model, Hvs, batches_, n, T, w, X=None):
    """The head of a multicomponent model in float64 on the CPU, op by op; returns (loss, raw outputs, {param id: grad}, [gH_v^c],
    {running_mean, running_var})."""
    from chemprop_amd.model import MODES, HeadSpec, masked_loss

    spec = HeadSpec(model)
    f = lambda t: t.detach().cpu().double()
    mode = {v: k for k, v in MODES.items()}[spec.agg_mode]
    leaves64, Hs = [], []
    for Hv, b in zip(Hvs, batches_):
        Hv64 = f(Hv).requires_grad_()
        leaves64.append(Hv64)
        b = b.cpu()
        H = torch.zeros(n, Hv64.shape[1], dtype=torch.float64).index_add(0, b, Hv64)
        if mode == "mean":
            H = H / torch.bincount(b, minlength=n).clamp(min=1).double().view(-1, 1)
        elif mode == "norm":
            H = H / spec.agg_norm
        Hs.append(H)
    H = torch.cat(Hs, 1)
    leaves, bufs = {}, {}
    if spec.bn is not None:
        bw, bb = f(spec.bn.weight).requires_grad_(), f(spec.bn.bias).requires_grad_()
        rm, rv = f(spec.bn.running_mean).clone(), f(spec.bn.running_var).clone()
        H = torch.nn.functional.batch_norm(H, rm, rv, bw, bb, training=True, momentum=spec.bn.momentum, eps=spec.bn.eps)
        leaves[id(spec.bn.weight)], leaves[id(spec.bn.bias)] = bw, bb
        bufs = dict(running_mean=rm, running_var=rv)
    Z = H if X is None else torch.cat((H, f(X)), 1)
    for i, blk in enumerate(model.predictor.ffn):
        lin = blk[-1]
        if i > 0:
            Z = blk[0](Z)
        W = f(lin.weight).requires_grad_()
        leaves[id(lin.weight)] = W
        bias = None
        if lin.bias is not None:
            bias = f(lin.bias).requires_grad_()
            leaves[id(lin.bias)] = bias
        Z = torch.nn.functional.linear(Z, W, bias)
    Y = Z
    P = Y.reshape(n, -1, spec.n_classes) if spec.kind == "ce" else Y
    l = masked_loss(P, f(T), None if w is None else f(w), None, None, None, spec.kind)
    l.backward()
    return float(l.detach()), Y.detach(), {k: v.grad for k, v in leaves.items()}, [x.grad for x in leaves64], bufs


def run_head(model, Hvs, batches_, n, T, w, X=None):
    """ONE ``dmpnn_head`` call on the components' H_v rows (one matrix) and the merged batch vector ``c n + i``."""
    from chemprop_amd import engine
    from chemprop_amd.model import HeadSpec

    lib = _lib.load()
    spec = HeadSpec(model)
    dev = Hvs[0].device
    Hv = torch.cat(Hvs).contiguous()
    batch = torch.cat([b + c * n for c, b in enumerate(batches_)]).contiguous()
    grads = {id(p): torch.zeros_like(p) for p in spec.params()}
    h = _lib.HeadArgs()
    nV, d = int(Hv.shape[0]), int(Hv.shape[1])
    keep = spec.fill(h, nV, n, d, batch, T, w, None, None, lambda p: None if p is None else grads[id(p)].data_ptr(), X_d=X)
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
    sizes = [int(x.shape[0]) for x in Hvs]
    return float(loss[0]), preds.cpu(), {k: g.cpu() for k, g in grads.items()}, list(gH.cpu().split(sizes))


def head_inputs(n_comp, n, d_h, kind, dev, seed=0, d_xd=0, **kw):
    torch.manual_seed(seed + 3)
    model = make_multi(["qm9"] * n_comp, False, d_h=d_h, hidden=96 if d_h < 300 else 300, tasks=2, kind=kind, d_xd=d_xd, **kw)
    model = model.to(dev).train()
    if model.bn.__class__ is torch.nn.BatchNorm1d:
        with torch.no_grad():
            model.bn.weight.uniform_(0.5, 1.5), model.bn.bias.uniform_(-0.5, 0.5)
            model.bn.running_mean.uniform_(-0.1, 0.1), model.bn.running_var.uniform_(0.5, 2.0)
    bs = batches(["qm9"] * n_comp, n, seed=seed)
    gen = torch.Generator().manual_seed(seed + 2)
    Hvs = [torch.randn(int(b.V.shape[0]), d_h, generator=gen).to(dev) for b in bs]
    bts = [b.batch.to(dev) for b in bs]
    if kind == "bce":
        T = torch.rand(n, 2, generator=gen).round()
    elif kind == "ce":
        T = torch.randint(0, 3, (n, 2), generator=gen).float()
    else:
        T = torch.randn(n, 2, generator=gen)
    T[torch.rand(n, 2, generator=gen) < 0.2] = float("nan")
    w = 0.5 + torch.rand(n, 1, generator=gen)
    X = torch.randn(n, d_xd, generator=gen).to(dev) if d_xd else None
    return model, Hvs, bts, T.to(dev), w.to(dev), X


# ---- GPU: the head ------------------------------------------------------------------------------------------------------------------
HEAD_CASES = {
    # (n_components, B, d_h, criterion, aggregation, batch norm, d_xd, DMPNN_HEAD)
    "2x64-rows-norm-bn": (2, 64, 64, "mse", "norm", True, 0, None),
    "3x64-rows-sum": (3, 64, 32, "bce", "sum", False, 0, None),
    "2x512-rows-mean-xd": (2, 512, 64, "mse", "mean", True, 40, None),
    "2x700-cols-norm": (2, 700, 300, "mse", "norm", True, 0, None),
    "3x700-cols-mean-xd": (3, 700, 64, "bce", "mean", True, 24, None),
    "2x1100-chain-sum": (2, 1100, 64, "mse", "sum", True, 0, None),
    "2x512-300-ce": (2, 512, 300, "ce", "norm", True, 0, None),
    "3x64-chain-mean-xd": (3, 64, 64, "mse", "mean", True, 13, "chain"),
    "2x512-chain-norm-nobn": (2, 512, 300, "ce", "norm", False, 0, "chain"),
    # a component width that is not a multiple of 4: the column kernels refuse it (a quad would straddle two components) and the
    # chain's scalar aggregation folds the components (molagg_fwd_rows / molagg_bwd_rows)
    "2x100-d30-mean": (2, 100, 30, "mse", "mean", True, 0, None),
    "3x600-d30-norm-xd": (3, 600, 30, "bce", "norm", True, 10, None),
}


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(HEAD_CASES))
def test_multicomponent_head_matches_float64_restatement(name, gpu_device, monkeypatch):
    """``dmpnn_head`` with ``n_components`` 2 / 3: loss, raw outputs, every head gradient, every component's ``gH_v`` and the running
    statistics against the float64 restatement — every aggregation regime (fused at B <= 512, in front beyond, the chain beyond 1 024
    and on demand), with and without batch norm and descriptors, MSE / BCE / cross entropy."""
    nc, n, d_h, kind, agg, bn, d_xd, form = HEAD_CASES[name]
    if form:
        monkeypatch.setenv("DMPNN_HEAD", form)
    model, Hvs, bts, T, w, X = head_inputs(nc, n, d_h, kind, gpu_device, d_xd=d_xd, agg=agg, bn=bn)
    ref_loss, ref_P, ref_g, ref_gH, ref_bufs = restate(model, Hvs, bts, n, T, w, X)
    loss, P, g, gH = run_head(model, Hvs, bts, n, T, w, X)
    assert abs(loss - ref_loss) <= 1e-5 * max(1.0, abs(ref_loss)), (loss, ref_loss)
    assert parity_err(P.numpy(), ref_P.numpy()) <= 2e-5
    from chemprop_amd.model import HeadSpec

    names = {id(p): k for k, p in model.named_parameters()}
    for p in HeadSpec(model).params():
        e = parity_err(g[id(p)].numpy(), ref_g[id(p)].numpy())
        assert e <= 2e-5, f"{names[id(p)]}: {e:.2e}"
        # (gradients of a loss that is a batch mean: max|ref| << 1, the floored bar is an absolute one — hold the relative one beside it)
        eu = parity_err_unfloored(g[id(p)].numpy(), ref_g[id(p)].numpy())
        print(f"{name} {names[id(p)]}: floored {e:.2e}, un-floored {eu:.2e}")
        assert eu <= 2e-5, f"{names[id(p)]}: un-floored {eu:.2e}"
    for c in range(nc):
        assert parity_err(gH[c].numpy(), ref_gH[c].numpy()) <= 2e-5, c
        eu = parity_err_unfloored(gH[c].numpy(), ref_gH[c].numpy())
        print(f"{name} gH_v[{c}]: un-floored {eu:.2e}")
        assert eu <= 2e-5, f"gH_v[{c}]: un-floored {eu:.2e}"
    for k, v in ref_bufs.items():
        assert parity_err(getattr(model.bn, k).cpu().numpy(), v.numpy()) <= 1e-6, k


@pytest.mark.gpu
@pytest.mark.parametrize("n,form", [(64, None), (700, None), (300, "chain")])
def test_head_n_components_one_is_bit_identical_to_zero(n, form, gpu_device, monkeypatch):
    """``n_components = 1`` is today's head, bit for bit: loss, predictions, every gradient."""
    from chemprop_amd import agg as cagg
    from chemprop_amd import synth
    from chemprop_amd.model import MPNN, MSE, RegressionFFN
    from chemprop_amd.nn import BondMessagePassing

    if form:
        monkeypatch.setenv("DMPNN_HEAD", form)
    torch.manual_seed(1)
    model = MPNN(BondMessagePassing(d_h=300), cagg.NormAggregation(), RegressionFFN(2, 300, 300, criterion=MSE(1.0)), batch_norm=True)
    model = model.to(gpu_device).train()
    bmg = synth.random_batch(n, "qm9", seed=2)
    gen = torch.Generator().manual_seed(3)
    Hv = torch.randn(int(bmg.V.shape[0]), 300, generator=gen).to(gpu_device)
    T, w = torch.randn(n, 2, generator=gen).to(gpu_device), (0.5 + torch.rand(n, 1, generator=gen)).to(gpu_device)
    batch = bmg.batch.to(gpu_device)
    a = copy.deepcopy(model)
    r0 = _single_head(model, Hv, batch, n, T, w, 0)
    r1 = _single_head(a, Hv, batch, n, T, w, 1)
    assert torch.equal(r0[0], r1[0]) and torch.equal(r0[1], r1[1]) and torch.equal(r0[3], r1[3])
    for x, y in zip(r0[2], r1[2]):
        assert torch.equal(x, y)
    assert torch.equal(model.bn.running_var, a.bn.running_var)


def _single_head(model, Hv, batch, n, T, w, ncomp_field):
    from chemprop_amd import engine
    from chemprop_amd.model import HeadSpec

    lib = _lib.load()
    spec = HeadSpec(model)
    dev = Hv.device
    grads = {id(p): torch.zeros_like(p) for p in spec.params()}
    h = _lib.HeadArgs()
    nV, d = int(Hv.shape[0]), int(Hv.shape[1])
    keep = spec.fill(h, nV, n, d, batch, T, w, None, None, lambda p: None if p is None else grads[id(p)].data_ptr())
    h.n_components = ncomp_field
    preds = torch.empty(n, spec.n_out, device=dev)
    loss = torch.empty(2, device=dev)
    gH = torch.empty(nV, d, device=dev)
    h.preds, h.loss_out, h.gHv, h.ldg = preds.data_ptr(), loss.data_ptr(), gH.data_ptr(), d
    nb = int(lib.dmpnn_head_ws_bytes(C.byref(h)))
    ws = torch.empty(nb, dtype=torch.uint8, device=dev)
    h.ws, h.ws_bytes = ws.data_ptr(), nb
    with engine._OnDevice(dev):
        _lib.check(lib.dmpnn_head(C.byref(h), Hv.data_ptr(), Hv.stride(0), engine._stream_ptr(dev)), "dmpnn_head")
    torch.cuda.synchronize()
    del keep
    return loss.cpu(), preds.cpu(), [grads[id(p)].cpu() for p in spec.params()], gH.cpu()


# ---- GPU: the one-call step ---------------------------------------------------------------------------------------------------------
STEP_CASES = {
    # (components, shared, B)
    "shared-qm9-qm9": (["qm9", "qm9"], True, 64),
    "separate-qm9-qm9": (["qm9", "qm9"], False, 64),
    "separate-cgr-qm9": (["cgr", "qm9"], False, 512),
    "separate-qm9-solvent": (["qm9", "solvent"], False, 64),
    "shared-qm9-qm9-512": (["qm9", "qm9"], True, 512),
}


def _step_pair(kinds, shared, n, dev, seed=11):
    torch.manual_seed(seed)
    a = make_multi(kinds, shared).to(dev).train()
    b = copy.deepcopy(a)
    bs = batches(kinds, n, dev, seed=seed)
    gen = torch.Generator().manual_seed(seed + 2)
    y = torch.randn(n, 1, generator=gen).to(dev)
    w = (0.5 + torch.rand(n, 1, generator=gen)).to(dev)
    return a, b, bs, y, w


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(STEP_CASES))
def test_fused_multicomponent_step_equals_module_path_over_three_steps(name, gpu_device):
    """``FusedTrainer.step`` on a ``MulticomponentMPNN`` three times against the module path run op by op on a copy —
    ``predictor.train_step(fingerprint(bmgs))`` + ``masked_loss`` + backward + ``torch.optim.Adam`` — and its first loss against the
    float64 restatement of the head on the module path's block outputs."""
    from chemprop_amd.model import FusedTrainer, masked_loss

    kinds, shared, n = STEP_CASES[name]
    a, b, bs, y, w = _step_pair(kinds, shared, n, gpu_device)
    tr = FusedTrainer(a, lr=1e-3, eps=1e-4)
    opt = torch.optim.Adam(b.parameters(), lr=1e-3, eps=1e-4)
    for s in range(3):
        if s == 0:
            with torch.no_grad():
                Hvs = b.message_passing(bs, None)
            ref = restate(b, Hvs, [x.batch for x in bs], n, y, w)[0]
        la = float(tr.step(bs, y, w)[0])
        opt.zero_grad()
        lb = masked_loss(b.predictor.train_step(b.fingerprint(bs)), y, w, None, None, None, "mse")
        lb.backward()
        opt.step()
        lb = float(lb.detach())
        if s == 0:
            assert abs(la - ref) <= 1e-5 * max(1.0, abs(ref)), (la, ref)
        assert abs(la - lb) <= (1e-5 if s == 0 else 1e-4) * max(1.0, abs(lb)), (s, la, lb)
    torch.cuda.synchronize()
    assert tr.opt.steps == 3
    if kinds[0] == "cgr":   # (one call, two routes: the CGR block on the per-step routes, the QM9 block on the tile kernel)
        assert isinstance(tr.last_route, tuple) and tr.last_route[0] != tr.last_route[1], tr.last_route
    assert len(list(a.parameters())) == len(list(b.parameters()))
    for (k, pa), (_, pb) in zip(a.named_parameters(), b.named_parameters()):
        e = parity_err(pa.detach().cpu().numpy(), pb.detach().cpu().numpy())
        assert e <= 1e-4, f"{k}: {e:.2e}"
    for k in ("running_mean", "running_var"):
        assert parity_err(getattr(a.bn, k).cpu().numpy(), getattr(b.bn, k).cpu().numpy()) <= 1e-5, k


@pytest.mark.gpu
@pytest.mark.parametrize("shared", [True, False])
def test_staged_multicomponent_step_equals_the_fused_one(shared, gpu_device, monkeypatch):
    """The data-parallel form (``DMPNN_FORCE_COLLECTIVE=1`` at world 1: forward stage, backward stage, update on the host side)
    computes what the one-call step computes."""
    from chemprop_amd.model import FusedTrainer

    kinds = ["cgr", "qm9"] if not shared else ["qm9", "qm9"]
    a, b, bs, y, w = _step_pair(kinds, shared, 96, gpu_device)
    ta, tb = FusedTrainer(a, lr=1e-3, eps=1e-4), None
    # (four steps: the first two on launched, validated plans; from the third on K0 and every component's plan inside the FORWARD stage)
    la = [float(ta.step(bs, y, w)[0]) for _ in range(4)]
    monkeypatch.setenv("DMPNN_FORCE_COLLECTIVE", "1")
    tb = FusedTrainer(b, lr=1e-3, eps=1e-4)
    lb = [float(tb.step(bs, y, w)[0]) for _ in range(4)]
    assert tb._checked == 2
    torch.cuda.synchronize()
    for x, z in zip(la, lb):
        assert abs(x - z) <= 1e-5 * max(1.0, abs(z)), (la, lb)
    for (k, pa), (_, pb) in zip(a.named_parameters(), b.named_parameters()):
        assert parity_err(pa.detach().cpu().numpy(), pb.detach().cpu().numpy()) <= 1e-5, k


@pytest.mark.gpu
def test_fused_multicomponent_step_refusals(gpu_device):
    """``ValueError`` for components of different ``B`` and for ``V_ds``; ``NotImplementedError`` for blocks of different ``d_h``,
    active dropout in a block, and a block the single-component step refuses (an atom block)."""
    from chemprop_amd import agg as cagg
    from chemprop_amd.model import FusedTrainer, MulticomponentMPNN, RegressionFFN
    from chemprop_amd.nn import AtomMessagePassing, BondMessagePassing, MulticomponentMessagePassing

    a, _, bs, y, w = _step_pair(["qm9", "qm9"], False, 32, gpu_device)
    tr = FusedTrainer(a)
    short = batches(["qm9"], 31, gpu_device, seed=5)[0]
    with pytest.raises(ValueError):
        tr.step([bs[0], short], y, w)
    with pytest.raises(ValueError):
        tr.step(bs, y, w, V_ds=[torch.zeros(int(bs[0].V.shape[0]), 4, device=gpu_device), None])

    def model(blocks):
        mp = MulticomponentMessagePassing(blocks, len(blocks))
        return MulticomponentMPNN(mp, cagg.NormAggregation(), RegressionFFN(1, mp.output_dim, 64), batch_norm=True).to(gpu_device)

    with pytest.raises(NotImplementedError):
        FusedTrainer(model([BondMessagePassing(d_h=64), BondMessagePassing(d_h=128)]))
    with pytest.raises(NotImplementedError):
        FusedTrainer(model([BondMessagePassing(d_h=64, dropout=0.1), BondMessagePassing(d_h=64)]))
    with pytest.raises(NotImplementedError):
        FusedTrainer(model([BondMessagePassing(d_h=64), AtomMessagePassing(d_h=64)]))


@pytest.mark.gpu
def test_module_path_multicomponent_loss_matches_torch_ops(gpu_device):
    """``MulticomponentMPNN.loss`` (the module path: ONE head node behind the blocks) gives the loss and the gradients of the op-by-op
    torch form."""
    from chemprop_amd.model import masked_loss

    a, b, bs, y, w = _step_pair(["cgr", "qm9"], False, 80, gpu_device)
    la = a.loss(bs, y, w)
    la.backward()
    lb = masked_loss(b.predictor.train_step(b.fingerprint(bs)), y, w, None, None, None, "mse")
    lb.backward()
    assert abs(float(la) - float(lb)) <= 1e-5 * max(1.0, abs(float(lb)))
    for (k, pa), (_, pb) in zip(a.named_parameters(), b.named_parameters()):
        assert parity_err(pa.grad.cpu().numpy(), pb.grad.cpu().numpy()) <= 2e-5, k
        eu = parity_err_unfloored(pa.grad.cpu().numpy(), pb.grad.cpu().numpy())
        print(f"multicomponent module path {k}: un-floored {eu:.2e}")
        assert eu <= 2e-5, f"{k}: un-floored {eu:.2e}"


# ---- CPU ------------------------------------------------------------------------------------------------------------------------------
def test_mirror_output_dim_shared_parameters_and_state_dict_keys():
    from chemprop_amd.nn import BondMessagePassing, MulticomponentMessagePassing

    blk = BondMessagePassing(d_h=64)
    sh = MulticomponentMessagePassing([blk], 3, shared=True)
    assert sh.output_dim == 192 and len(sh) == 3 and sh.hparams["shared"] and sh.hparams["n_components"] == 3
    assert all(b is blk for b in sh.blocks)
    assert len(list(sh.parameters())) == len(list(blk.parameters()))   # (one block's parameters, listed once)
    sep = MulticomponentMessagePassing([BondMessagePassing(d_h=64), BondMessagePassing(106, 28, d_h=32)], 2)
    assert sep.output_dim == 96
    keys = set(sep.state_dict())
    assert {"blocks.0.W_i.weight", "blocks.0.W_h.weight", "blocks.0.W_o.weight", "blocks.0.W_o.bias", "blocks.1.W_i.weight"} <= keys
    with pytest.raises(ValueError):
        MulticomponentMessagePassing([BondMessagePassing(d_h=64)], 2, shared=False)
    with pytest.raises(ValueError):
        MulticomponentMessagePassing([], 2, shared=True)
    m = make_multi(["qm9", "qm9"], True, d_h=64, hidden=32)
    assert m.bn.num_features == 128 and "message_passing.blocks.0.W_h.weight" in m.state_dict()


def test_merge_components_offsets_and_batch_vector():
    from chemprop_amd.data import merge_components

    bs = batches(["qm9", "solvent", "qm9"], 5, seed=3)
    m = merge_components(bs)
    assert len(m) == 15
    nV = [int(b.V.shape[0]) for b in bs]
    nE = [int(b.E.shape[0]) for b in bs]
    assert torch.equal(m.V, torch.cat([b.V for b in bs])) and torch.equal(m.E, torch.cat([b.E for b in bs]))
    assert torch.equal(m.edge_index, torch.cat([bs[0].edge_index, bs[1].edge_index + nV[0], bs[2].edge_index + nV[0] + nV[1]], 1))
    assert torch.equal(m.rev_edge_index, torch.cat([bs[0].rev_edge_index, bs[1].rev_edge_index + nE[0], bs[2].rev_edge_index + nE[0] + nE[1]]))
    assert torch.equal(m.batch, torch.cat([bs[0].batch, bs[1].batch + 5, bs[2].batch + 10]))
    assert bool((m.batch[1:] >= m.batch[:-1]).all())
    with pytest.raises(ValueError):
        merge_components([bs[0], batches(["qm9"], 4)[0]])


def test_grown_structs_match_the_c_layout(tmp_path):
    """``dmpnn_head_args.n_components`` and ``dmpnn_step_args.n_extra / extra`` (+ ``dmpnn_step_component``) at the offsets the C
    compiler gives them (include/dmpnn.h), and the size of every struct."""
    import os
    import shutil
    import subprocess

    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if cc is None:
        cc = "/opt/rocm/llvm/bin/clang"
    src = tmp_path / "off.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "dmpnn.h"\nint main(void){printf("%zu %zu %zu %zu %zu %zu %zu %zu\\n",'
                   'offsetof(dmpnn_head_args, n_components), sizeof(dmpnn_head_args), offsetof(dmpnn_step_args, n_extra),'
                   'offsetof(dmpnn_step_args, extra), sizeof(dmpnn_step_args), offsetof(dmpnn_step_component, bwd),'
                   'sizeof(dmpnn_step_component), offsetof(dmpnn_step_args, clip_ws));return 0;}\n')
    exe = tmp_path / "off"
    inc = os.path.join(os.path.dirname(_lib.__file__), "..", "include")
    subprocess.run([cc, "-I", inc, str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    want = [_lib.HeadArgs.n_components.offset, C.sizeof(_lib.HeadArgs), _lib.StepArgs.n_extra.offset, _lib.StepArgs.extra.offset,
            C.sizeof(_lib.StepArgs), _lib.StepComponent.bwd.offset, C.sizeof(_lib.StepComponent), _lib.StepArgs.clip_ws.offset]
    assert got == want


def _head_args(n_mols=64, d_h=300, dims=(600, 300, 1), ncomp=2):
    h = _lib.HeadArgs()
    h.n_atoms, h.n_mols, h.d_h = 9 * n_mols, n_mols, d_h
    h.n_layers = len(dims) - 1
    for i, v in enumerate(dims):
        h.dims[i] = v
    h.n_components = ncomp
    return h


def test_head_refuses_inconsistent_components_before_touching_the_device():
    """``dims[0]`` against ``n_components d_h``, and ``n_components`` in range: ``DMPNN_EINVAL`` before anything reaches the device
    (no GPU here)."""
    lib = _lib.load()

    def call(h):
        return int(lib.dmpnn_head(C.byref(h), 4096, h.d_h, None)), lib.dmpnn_last_error_string().decode()

    for dims0, nc in ((300, 2), (900, 2), (600, 3)):
        rc, msg = call(_head_args(dims=(dims0, 300, 1), ncomp=nc))
        assert rc == -1 and "dims[0]" in msg, (rc, msg)
    for nc in (-1, _lib.MAX_COMPONENTS + 1):
        rc, msg = call(_head_args(dims=(300 * max(nc, 1), 300, 1), ncomp=nc))
        assert rc == -1 and "n_components" in msg, (rc, msg)
    rc, msg = call(_head_args(dims=(600, 300, 1), ncomp=2))   # consistent: past those checks, stopped at the next one (no weights)
    assert rc == -1 and "no weight" in msg, (rc, msg)
    # the workspace grows with the components' fingerprint
    assert int(lib.dmpnn_head_ws_bytes(C.byref(_head_args(dims=(600, 300, 1), ncomp=2)))) > \
        int(lib.dmpnn_head_ws_bytes(C.byref(_head_args(dims=(300, 300, 1), ncomp=0))))
