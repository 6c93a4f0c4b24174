"""Molecule descriptors ``X_d`` (``--molecule-featurizers`` / ``--descriptors-path``) on the head kernels and the one-call training
step: ``fingerprint = cat(bn(agg(H_v)), X_d_transform(X_d))`` (``models/model.py``, ``fingerprint``), the predictor's first layer
``d_h + d_xd`` wide.  ``dmpnn_head_args.X_d / ld_xd``; the chain form and the four-launch row form (``csrc/dmpnn_head.hip``)."""
import copy
import ctypes as C

import numpy as np
import pytest
import torch
from torch import nn

from chemprop_amd import _lib
from conftest import parity_err, parity_err_unfloored
from head_harness import case_inputs, descriptors, make_model, restate, run_head


CASES = {
    # (form, n_mols, d_h, d_xd, hidden, tasks, n_layers, bn, agg, kind, act, X_d kind, strided view)
    "rows-512-300+200": ("rows", 512, 300, 200, 300, 1, 1, True, "norm", "mse", "relu", "mixed", False),
    "rows-77-64+36": ("rows", 77, 64, 36, 128, 3, 1, True, "sum", "bounded-mse", "elu", "mixed", False),
    "rows-1000-300+212": ("rows", 1000, 300, 212, 200, 4, 1, False, "mean", "bce", "leakyrelu", "normal", False),
    "chain-64-300+2048-binary": ("chain", 64, 300, 2048, 300, 1, 1, True, "norm", "mse", "relu", "binary", False),
    "chain-odd-13": ("chain", 100, 64, 13, 96, 2, 1, True, "mean", "mse", "tanh", "mixed", False),
    "chain-strided-view": ("chain", 100, 64, 40, 96, 2, 1, True, "sum", "mae", "tanh", "mixed", True),
    "chain-two-hidden": ("chain", 120, 64, 24, 80, 1, 2, True, "norm", "mse", "elu", "normal", False),
    "chain-no-hidden": ("chain", 60, 64, 13, 64, 2, 0, False, "norm", "mse", "relu", "mixed", False),
    "chain-multiclass": ("chain", 90, 64, 20, 64, 2, 1, True, "norm", "ce", "elu", "normal", False),
    "chain-mve": ("chain", 90, 64, 20, 64, 2, 1, False, "mean", "mve", "elu", "normal", False),
}


# ---- GPU ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_head_with_descriptors_matches_float64_restatement(name, gpu_device, monkeypatch):
    """``dmpnn_head`` with ``X_d``: loss, raw predictions, every gradient (``gW[0]`` with its descriptor columns, ``gb``, batch-norm
    weight and bias, ``gH_v``) and the running statistics against the float64 restatement on the CPU.  The row cases run under
    ``DMPNN_HEAD=rows`` (a shape that would fall back to the chain is an error there), the others under ``DMPNN_HEAD=chain``."""
    case = CASES[name]
    model, Hv, batch, n, T, w, lt, gt, X = case_inputs(case, gpu_device)
    ref_loss, ref_P, ref_g, ref_gH, ref_bufs = restate(model, Hv, batch, n, T, w, lt, gt, X)
    monkeypatch.setenv("DMPNN_HEAD", case[0])
    loss, P, g, gH = run_head(model, Hv, batch, n, T, w, lt, gt, X)
    assert abs(loss - ref_loss) <= 1e-5 * max(1.0, abs(ref_loss)), (loss, ref_loss)
    assert parity_err(P.numpy(), ref_P.numpy()) <= 2e-5
    assert parity_err_unfloored(P.numpy(), ref_P.numpy()) <= 2e-5
    from chemprop_amd.model import HeadSpec

    spec = HeadSpec(model)
    names = {id(p): k for k, p in model.named_parameters()}
    assert len(ref_g) == len(spec.params())
    for p in spec.params():
        assert torch.isfinite(g[id(p)]).all(), names[id(p)]
        e = parity_err(g[id(p)].numpy(), ref_g[id(p)].numpy())
        assert e <= 2e-5, f"{names[id(p)]}: {e:.2e}"
        # (the loss is a mean over the batch: max|ref| << 1, the floored metric above is an absolute bar there — hold the relative one too)
        eu = parity_err_unfloored(g[id(p)].numpy(), ref_g[id(p)].numpy())
        print(f"{name} {names[id(p)]}: floored {e:.2e}, un-floored {eu:.2e}")
        assert eu <= 2e-5, f"{names[id(p)]}: un-floored {eu:.2e}"
    assert parity_err(gH.numpy(), ref_gH.numpy()) <= 2e-5
    eu = parity_err_unfloored(gH.numpy(), ref_gH.numpy())
    print(f"{name} gH_v: un-floored {eu:.2e}")
    assert eu <= 2e-5, f"gH_v: un-floored {eu:.2e}"
    W0 = spec.layers[0].weight
    assert float(ref_g[id(W0)][:, case[2]:].abs().max()) > 0   # (the descriptor columns of gW[0] carry a gradient)
    for k, v in ref_bufs.items():
        assert parity_err(getattr(model.bn, k).cpu().numpy(), v.numpy()) <= 1e-6, k


@pytest.mark.gpu
@pytest.mark.parametrize("name", [k for k, v in CASES.items() if v[0] == "rows"])
def test_head_rows_form_equals_chain_with_descriptors(name, gpu_device, monkeypatch):
    """The four-launch row form against the chain on the row form's descriptor shapes (``DMPNN_HEAD=rows`` / ``=chain``)."""
    case = CASES[name]
    a = case_inputs(case, gpu_device)
    b = case_inputs(case, gpu_device)
    monkeypatch.setenv("DMPNN_HEAD", "rows")
    la, Pa, ga, gHa = run_head(*a)
    monkeypatch.setenv("DMPNN_HEAD", "chain")
    lb, Pb, gb, gHb = run_head(*b)
    assert abs(la - lb) <= 2e-6 * max(1.0, abs(lb)), (la, lb)
    assert parity_err(Pa.numpy(), Pb.numpy()) <= 1e-5
    pa = [p for p in a[0].parameters()]
    pb = [p for p in b[0].parameters()]
    for x, y in zip(pa, pb):
        if id(x) in ga:
            assert parity_err(ga[id(x)].numpy(), gb[id(y)].numpy()) <= 1e-5
            assert parity_err_unfloored(ga[id(x)].numpy(), gb[id(y)].numpy()) <= 1e-5
    assert parity_err(gHa.numpy(), gHb.numpy()) <= 1e-5
    assert parity_err_unfloored(gHa.numpy(), gHb.numpy()) <= 1e-5


@pytest.mark.gpu
def test_rows_form_refuses_a_descriptor_shape_beyond_its_limits(gpu_device, monkeypatch):
    """``DMPNN_HEAD=rows`` reports an error for a descriptor model whose first layer is wider than 512 (it would take the chain)."""
    case = ("rows", 64, 300, 2048, 300, 1, 1, True, "norm", "mse", "relu", "binary", False)
    args = case_inputs(case, gpu_device)
    monkeypatch.setenv("DMPNN_HEAD", "rows")
    with pytest.raises(RuntimeError, match="DMPNN_HEAD=rows"):
        run_head(*args)


def _step_models(n_mols, d_xd, xk, gpu_device, seed=11):
    from chemprop_amd import synth

    torch.manual_seed(seed)
    a = make_model(300, d_xd, 300, 1, True, "norm", "mse", "elu", depth=3)
    b = copy.deepcopy(a)
    a, b = a.to(gpu_device).train(), b.to(gpu_device).train()
    bmg = synth.random_batch(n_mols, "qm9", seed=seed + 1)
    bmg.to(gpu_device)
    gen = torch.Generator().manual_seed(seed + 2)
    y = torch.randn(n_mols, 1, generator=gen).to(gpu_device)
    w = (0.5 + torch.rand(n_mols, 1, generator=gen)).to(gpu_device)
    X = descriptors(n_mols, d_xd, seed + 3, xk).to(gpu_device)
    return a, b, bmg, y, w, X


@pytest.mark.gpu
@pytest.mark.parametrize("n_mols,d_xd,xk", [(512, 200, "mixed"), (64, 2048, "binary")])
def test_fused_step_with_descriptors_equals_module_path_over_three_steps(n_mols, d_xd, xk, gpu_device):
    """``FusedTrainer.step(..., X_d=...)`` three times against the module path run op by op on a copy of the model —
    ``predictor.train_step(fingerprint(bmg, X_d=X_d))`` + ``masked_loss`` + backward + ``torch.optim.Adam``: the losses, the
    parameters and the batch-norm buffers after the three steps.  (Adam's eps at 1e-4: an entry whose gradient is fp32 noise around
    zero must not move by a full learning rate in the direction of the noise's sign.)"""
    from chemprop_amd.model import FusedTrainer, masked_loss

    a, b, bmg, y, w, X = _step_models(n_mols, d_xd, xk, gpu_device)
    tr = FusedTrainer(a, lr=1e-3, eps=1e-4)
    opt = torch.optim.Adam(b.parameters(), lr=1e-3, eps=1e-4)
    for s in range(3):
        la = float(tr.step(bmg, y, w, X_d=X)[0])
        opt.zero_grad()
        lb = masked_loss(b.predictor.train_step(b.fingerprint(bmg, X_d=X)), y, w, None, None, None, "mse")
        lb.backward()
        opt.step()
        # (the first step from the same parameters to the fp32 bar; the later ones from parameters that two Adam updates have moved
        #  apart by their fp32 differences)
        lb = float(lb.detach())
        assert abs(la - lb) <= (1e-5 if s == 0 else 1e-4) * max(1.0, abs(lb)), (s, la, lb)
    torch.cuda.synchronize()
    assert tr.opt.steps == 3
    for (k, pa), (_, pb) in zip(a.named_parameters(), b.named_parameters()):
        e = parity_err(pa.detach().cpu().numpy(), pb.detach().cpu().numpy())
        assert e <= 1e-4, f"{k}: {e:.2e}"
    for k in ("running_mean", "running_var"):
        assert parity_err(getattr(a.bn, k).cpu().numpy(), getattr(b.bn, k).cpu().numpy()) <= 1e-5, k
    assert int(a.bn.num_batches_tracked) == int(b.bn.num_batches_tracked) == 3


@pytest.mark.gpu
def test_fused_step_learns_from_the_descriptors(gpu_device):
    """Targets that are a fixed linear function of ``X_d`` alone: the fused step's loss falls below a quarter of its start in 60 steps
    (the descriptors reach the predictor's first layer)."""
    from chemprop_amd import synth
    from chemprop_amd.model import FusedTrainer

    torch.manual_seed(0)
    model = make_model(64, 16, 64, 1, True, "mean", "mse", "relu").to(gpu_device).train()
    bmg = synth.random_batch(64, "qm9", seed=2)
    bmg.to(gpu_device)
    X = descriptors(64, 16, 3).to(gpu_device)
    coef = torch.randn(16, 1, generator=torch.Generator().manual_seed(4)).to(gpu_device)
    y = X @ coef
    tr = FusedTrainer(model, lr=3e-3)
    losses = [float(tr.step(bmg, y, X_d=X)[0]) for _ in range(60)]
    assert np.mean(losses[-5:]) < 0.25 * np.mean(losses[:5]), (losses[:5], losses[-5:])


@pytest.mark.gpu
def test_module_path_loss_with_descriptors_is_one_autograd_node(gpu_device):
    """``MPNN.loss(..., X_d=...)``: ONE ``_HeadLoss`` node whose gradients match the torch modules op by op (through
    ``X_d_transform``); descriptors that need a gradient themselves take the module path (and get it)."""
    from chemprop_amd import synth
    from chemprop_amd.model import masked_loss

    class Scale(nn.Module):   # (the reference's ScaleTransform in its evaluated form: (X - mean) / scale)
        def __init__(self, d):
            super().__init__()
            self.register_buffer("mean", torch.linspace(-1.0, 1.0, d))
            self.register_buffer("scale", torch.linspace(0.5, 2.0, d))

        def forward(self, X):
            return (X - self.mean) / self.scale

    torch.manual_seed(3)
    a = make_model(64, 24, 48, 2, True, "sum", "mse", "elu", n_layers=2, X_d_transform=Scale(24)).to(gpu_device).train()
    b = copy.deepcopy(a)
    bmg = synth.random_batch(40, "qm9", seed=6)
    bmg.to(gpu_device)
    gen = torch.Generator().manual_seed(1)
    y = torch.randn(40, 2, generator=gen)
    y[torch.rand(40, 2, generator=gen) < 0.2] = float("nan")
    y = y.to(gpu_device)
    w = (0.5 + torch.rand(40, 1, generator=gen)).to(gpu_device)
    X = descriptors(40, 24, 7, "mixed").to(gpu_device)
    la = a.loss(bmg, y, w, X_d=X)
    assert type(la.grad_fn).__name__ == "_HeadLossBackward", type(la.grad_fn).__name__
    (2.5 * la).backward()
    lb = masked_loss(b.predictor.train_step(b.fingerprint(bmg, X_d=X)), y, w, None, None, None, "mse")
    (2.5 * lb).backward()
    torch.cuda.synchronize()
    assert abs(float(la) - float(lb)) <= 1e-5 * max(1.0, abs(float(lb))), (float(la), float(lb))
    for (k, pa), (_, pb) in zip(a.named_parameters(), b.named_parameters()):
        assert (pa.grad is None) == (pb.grad is None), k
        if pa.grad is not None:
            assert parity_err(pa.grad.cpu().numpy(), pb.grad.cpu().numpy()) <= 2e-5, k
            eu = parity_err_unfloored(pa.grad.cpu().numpy(), pb.grad.cpu().numpy())
            print(f"module path with descriptors {k}: un-floored {eu:.2e}")
            assert eu <= 2e-5, f"{k}: un-floored {eu:.2e}"
    for k in ("running_mean", "running_var"):
        assert parity_err(getattr(a.bn, k).cpu().numpy(), getattr(b.bn, k).cpu().numpy()) <= 1e-6, k
    Xg = X.clone().requires_grad_()
    lc = a.loss(bmg, y, w, X_d=Xg)
    assert type(lc.grad_fn).__name__ != "_HeadLossBackward"
    lc.backward()
    assert Xg.grad is not None and torch.isfinite(Xg.grad).all()


@pytest.mark.gpu
def test_fused_step_refuses_missing_unexpected_or_misshapen_descriptors(gpu_device):
    from chemprop_amd import synth
    from chemprop_amd.model import FusedTrainer

    torch.manual_seed(0)
    with_xd = make_model(64, 16, 64, 1).to(gpu_device).train()
    without = make_model(64, 0, 64, 1).to(gpu_device).train()
    bmg = synth.random_batch(32, "qm9", seed=2)
    bmg.to(gpu_device)
    y = torch.randn(32, 1, device=gpu_device)
    X = torch.randn(32, 16, device=gpu_device)
    ta, tb = FusedTrainer(with_xd), FusedTrainer(without)
    with pytest.raises(ValueError, match="expects 16"):
        ta.step(bmg, y)
    with pytest.raises(ValueError, match="no molecule descriptors"):
        tb.step(bmg, y, X_d=X)
    for bad in (X[:, :15], X[:31], X.reshape(-1)):
        with pytest.raises(ValueError, match="X_d must be"):
            ta.step(bmg, y, X_d=bad)
    assert ta.opt.steps == 0 and tb.opt.steps == 0
    ta.step(bmg, y, X_d=X.double())   # (converted to fp32 rows)
    assert ta.opt.steps == 1


# ---- no GPU -------------------------------------------------------------------------------------------------------------------------
def _head_args(n_mols=64, d_h=300, dims=(300, 300, 1), X_d=None, ld_xd=0):
    h = _lib.HeadArgs()
    h.n_atoms, h.n_mols, h.d_h = 9 * n_mols, n_mols, d_h
    h.n_layers = len(dims) - 1
    for i, v in enumerate(dims):
        h.dims[i] = v
    h.X_d, h.ld_xd = X_d, ld_xd
    return h


def test_head_refuses_inconsistent_descriptor_widths_before_touching_the_device():
    """``dmpnn_head`` checks ``X_d`` / ``ld_xd`` / ``dims[0]`` before anything reaches the device (no GPU here): ``DMPNN_EINVAL``."""
    lib = _lib.load()

    def call(h):
        return int(lib.dmpnn_head(C.byref(h), 4096, h.d_h, None)), lib.dmpnn_last_error_string().decode()

    fake = 4096   # (never dereferenced: every case fails its argument checks)
    for dims0 in (300, 200):   # X_d given, dims[0] <= d_h
        rc, msg = call(_head_args(dims=(dims0, 300, 1), X_d=fake, ld_xd=64))
        assert rc == -1 and "X_d" in msg, (rc, msg)
    rc, msg = call(_head_args(dims=(500, 300, 1), X_d=fake, ld_xd=199))   # ld_xd < d_xd
    assert rc == -1 and "ld_xd" in msg, (rc, msg)
    rc, msg = call(_head_args(dims=(500, 300, 1)))                         # no X_d, dims[0] != d_h
    assert rc == -1 and "dims[0] == d_h" in msg, (rc, msg)
    # a consistent descriptor shape gets past those checks (and stops at the next one: no weights)
    rc, msg = call(_head_args(dims=(500, 300, 1), X_d=fake, ld_xd=200))
    assert rc == -1 and "no weight" in msg, (rc, msg)


# dmpnn_head_ws_bytes of the shapes tests/test_abi.py lists (and a few more), as the library before descriptors computed them:
# (n_mols, d_h, hidden, n_tasks, loss) -> bytes
WS_PINNED = {
    (512, 300, 300, 8, 0): 10698496, (512, 300, 300, 1, 0): 11503872, (77, 64, 128, 3, 0): 482560, (1024, 300, 200, 4, 0): 17019392,
    (512, 300, 300, 1, 3): 10684160, (77, 64, 128, 3, 3): 408320, (1024, 300, 200, 4, 3): 16272128, (1025, 300, 300, 1, 0): 21384448,
    (512, 300, 384, 1, 0): 13216768, (512, 300, 384, 1, 3): 13216768, (64, 300, 300, 1, 0): 2439168, (1000, 300, 200, 4, 0): 16828928,
    (16, 128, 36, 2, 0): 213248,
}


def _ws(n_mols, d, hidden, tasks, loss=0, d_xd=0, X_d=None):
    lib = _lib.load()
    h = _head_args(n_mols, d, (d + d_xd, hidden, tasks), X_d=X_d, ld_xd=d_xd)
    h.loss = loss
    h.n_classes = 2 if loss == _lib.LOSS["ce"] else 0
    return int(lib.dmpnn_head_ws_bytes(C.byref(h)))


def test_head_workspace_grows_for_descriptors_only():
    """``dmpnn_head_ws_bytes``: the shapes without descriptors keep their sizes (pinned from the library before ``X_d``); a descriptor
    shape adds the fingerprint ``[n_mols, Kp]`` (and, on the row form, the wider forward split of W0)."""
    for (n, d, hid, t, loss), want in WS_PINNED.items():
        assert _ws(n, d, hid, t, loss) == want, (n, d, hid, t, loss)
        assert _ws(n, d, hid, t, loss, X_d=None) == want
    base = _ws(512, 300, 300, 1)
    with_xd = _ws(512, 300, 300, 1, d_xd=200, X_d=4096)
    assert with_xd >= base + 512 * 500 * 4
    # the chain's descriptor shape (2048 columns): at least the fingerprint and layer 0's [N, K] scratch
    assert _ws(64, 300, 300, 1, d_xd=2048, X_d=4096) >= _ws(64, 300, 300, 1) + 64 * 2348 * 4 + 300 * 2348 * 4


def test_mirror_mpnn_builds_a_descriptor_model_with_the_reference_names():
    """The mirror ``MPNN`` takes a predictor wider than the block (``X_d_transform`` under the reference's attribute name; its
    buffers in the state dict); without a transform the state-dict keys are exactly those of the four sub-modules; a narrower
    predictor is refused.  ``HeadSpec.d_xd`` and the checks of what the kernels would be handed (no GPU needed)."""
    from chemprop_amd import agg as cagg
    from chemprop_amd.model import MPNN, HeadSpec, RegressionFFN
    from chemprop_amd.nn import BondMessagePassing

    class Scale(nn.Module):
        def __init__(self, d):
            super().__init__()
            self.register_buffer("mean", torch.zeros(d))
            self.register_buffer("scale", torch.ones(d))

        def forward(self, X):
            return (X - self.mean) / self.scale

    mp, ag = BondMessagePassing(d_h=64), cagg.MeanAggregation()
    pred = RegressionFFN(input_dim=64 + 10, hidden_dim=32)
    m = MPNN(mp, ag, pred, batch_norm=True, X_d_transform=Scale(10))
    keys = set(m.state_dict())
    assert {"X_d_transform.mean", "X_d_transform.scale"} <= keys
    plain = MPNN(BondMessagePassing(d_h=64), cagg.MeanAggregation(), RegressionFFN(input_dim=74, hidden_dim=32), batch_norm=True)
    subs = {f"{n}.{k}" for n in ("message_passing", "agg", "bn", "predictor") for k in getattr(plain, n).state_dict()}
    assert set(plain.state_dict()) == subs
    assert isinstance(plain.X_d_transform, nn.Identity)
    with pytest.raises(ValueError):
        MPNN(BondMessagePassing(d_h=64), cagg.MeanAggregation(), RegressionFFN(input_dim=60))
    spec = HeadSpec(m)
    assert spec.d_xd == 10
    assert HeadSpec(MPNN(BondMessagePassing(d_h=64), cagg.MeanAggregation(), RegressionFFN(input_dim=64))).d_xd == 0
    dev = torch.device("cpu")
    with pytest.raises(ValueError, match="expects 10"):
        spec.descriptors(None, 8, dev)
    with pytest.raises(ValueError, match="X_d must be"):
        spec.descriptors(torch.zeros(8, 9), 8, dev)
    wide = torch.zeros(8, 16, dtype=torch.float64)[:, 2:12]
    X = spec.descriptors(wide, 8, dev)
    assert X.dtype == torch.float32 and X.stride(1) == 1 and tuple(X.shape) == (8, 10)
    view = torch.zeros(8, 16)[:, 3:13]
    assert spec.descriptors(view, 8, dev).data_ptr() == view.data_ptr()   # (a row-strided fp32 view goes through as it is)
