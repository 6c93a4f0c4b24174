"""Spectral heads on the one-call step (``FusedTrainer.step`` -> ``dmpnn_train_step``) and on the module path's one-node head
(``MPNN.loss`` -> ``head_loss`` -> ``_HeadLoss``), against a float64 restatement of the whole model on the CPU: the block through
``oracle.dmpnn_torch.forward``, the head (aggregation, batch norm on batch statistics, the MLP) through
``tests/test_dirichlet_step_gpu.py``'s ops, the criterion through ``tests/test_spectral_head.py``'s restatement of ``include/dmpnn.h``,
Adam through ``torch.optim.Adam`` in float64.

The model: ``d_h`` 64, depth 3, one hidden layer of 32, batch norm, tanh, a ``SpectralFFN`` of ``t = 65``; SID and Wasserstein,
softplus and exp, one run with a threshold.  Batches: 24 QM9-shaped and 12 ZINC-shaped molecules, 15 % missing targets.

Bars: those of ``tests/test_dirichlet_step_gpu.py`` — the loss within ``1e-5 max(1, |ref|)``, every gradient within ``parity_err <=
2e-5``, the parameters after two Adam steps within ``2e-6`` of Adam on the CPU fed with the kernels' gradients and within ``2e-4`` of
the float64 restatement's own two steps on the entries ``conftest.adam_comparable`` keeps."""
import copy
import math

import pytest
import torch

from conftest import adam_comparable, parity_err, parity_err_where
from test_dirichlet_step_gpu import LR, _adam_reference, fingerprint64
from test_spectral_head import spectral_criterion, spectral_targets

F = torch.nn.functional
pytestmark = pytest.mark.gpu
T_SPEC = 65


def _model(kind, crit, sact, thr=None, dropout=0.0, seed=7, act="tanh", mp_dropout=0.0):
    from chemprop_amd import agg as cagg
    from chemprop_amd.model import MPNN, SID, SpectralFFN, Wasserstein

    torch.manual_seed(seed)
    d_h = 64
    mp = BondMessagePassing_(d_h, act, mp_dropout)
    tw = 0.5 + torch.rand(T_SPEC, generator=torch.Generator().manual_seed(seed + 1))
    pred = SpectralFFN(n_tasks=T_SPEC, input_dim=d_h, hidden_dim=32, n_layers=1, dropout=dropout, activation=act,
                       criterion=(SID if crit == "sid" else Wasserstein)(tw, threshold=thr), spectral_activation=sact)
    agg = cagg.MeanAggregation() if kind == "qm9" else cagg.NormAggregation()
    return MPNN(mp, agg, pred, batch_norm=True).train()


def BondMessagePassing_(d_h, act, dropout):
    from chemprop_amd.nn import BondMessagePassing

    return BondMessagePassing(d_h=d_h, depth=3, activation=act, dropout=dropout)


def _batch(n, kind, seed=41):
    from chemprop_amd import synth

    gen = torch.Generator().manual_seed(seed)
    T = spectral_targets(n, T_SPEC, "none", seed).double()
    gone = torch.rand(n, T_SPEC, generator=gen) < 0.15
    gone[:, 0] = False
    T = T / torch.where(gone, torch.zeros_like(T), T).sum(1, keepdim=True)
    T[gone] = float("nan")
    return synth.random_batch(n, kind, seed=seed), synth.random_batch(n, kind, seed=seed), T.float(), 0.5 + torch.rand(n, 1, generator=gen)


def raw64(m, Z):
    from chemprop_amd.ffn import mlp_blocks

    for l, blk in enumerate(mlp_blocks(m.predictor.ffn)):
        Z = F.linear(torch.tanh(Z) if l else Z, blk[-1].weight, blk[-1].bias)
    return Z


def float64_steps(model, bmg, T, w, crit, sact, thr, steps=2):
    m = copy.deepcopy(model).cpu().double().train()
    opt = torch.optim.Adam([p for p in m.parameters()], LR)
    losses, grads = [], []
    for _ in range(steps):
        opt.zero_grad()
        H = fingerprint64(m, bmg)
        Z = F.batch_norm(H, m.bn.running_mean, m.bn.running_var, m.bn.weight, m.bn.bias, training=True, momentum=m.bn.momentum, eps=m.bn.eps)
        loss = spectral_criterion(crit, raw64(m, Z), T.double(), w.double().reshape(-1), m.predictor.criterion.task_weights.reshape(-1), sact, thr)
        loss.backward()
        losses.append(float(loss.detach()))
        grads.append({k: p.grad.clone() for k, p in m.named_parameters()})
        opt.step()
    return losses, grads, {k: p.detach() for k, p in m.named_parameters()}


CASES = [("qm9x24-sid-softplus", 24, "qm9", "sid", "softplus", None), ("qm9x24-wasserstein-exp", 24, "qm9", "wasserstein", "exp", None),
         ("zincx12-wasserstein-softplus", 12, "zinc", "wasserstein", "softplus", None), ("zincx12-sid-exp", 12, "zinc", "sid", "exp", None),
         ("qm9x24-sid-softplus-thr", 24, "qm9", "sid", "softplus", 0.5 / T_SPEC)]


@pytest.mark.parametrize("cid,n,kind,crit,sact,thr", CASES, ids=[c[0] for c in CASES])
def test_one_call_step_and_module_path_against_float64(cid, n, kind, crit, sact, thr, gpu_device):
    """Two ``FusedTrainer.step`` calls — ``FusedTrainer(model)`` takes these models — losses, every gradient of the first step and the
    parameters after the second against the float64 restatement; the module path's loss is ONE ``_HeadLoss`` node."""
    from chemprop_amd.model import FusedTrainer, HeadSpec

    cpu_model = _model(kind, crit, sact, thr)
    cpu_bmg, bmg, T, w = _batch(n, kind)
    ref_losses, ref_grads, ref_params = float64_steps(cpu_model, cpu_bmg, T, w, crit, sact, thr)

    model = copy.deepcopy(cpu_model).to(gpu_device).train()
    bmg.to(gpu_device)
    Tg, wg = T.to(gpu_device), w.to(gpu_device)
    state = copy.deepcopy(model.state_dict())
    loss_mod = model.loss(bmg, Tg, wg)
    assert type(loss_mod.grad_fn).__name__ == "_HeadLossBackward", type(loss_mod.grad_fn).__name__
    spec = model.__dict__["_dmpnn_head_spec"][1]
    assert isinstance(spec, HeadSpec) and (spec.kind, spec.n_tasks, spec.spectral_act, spec.spectral_threshold) == (crit, T_SPEC, sact, thr or 0.0)
    loss_mod.backward()
    mod_grads = {k: p.grad.detach().cpu().clone() for k, p in model.named_parameters()}
    model.load_state_dict(state)
    model.zero_grad(set_to_none=True)

    tr = FusedTrainer(model, lr=LR)
    names = [k for k, p in model.named_parameters() if p.requires_grad]
    p0 = [p.detach().cpu().clone() for _, p in model.named_parameters() if p.requires_grad]
    my_grads = []
    for s in range(2):
        out = tr.step(bmg, Tg, wg)
        torch.cuda.synchronize()
        print(f"SPECSTEP {cid} step {s} route {tr.last_route} loss {float(out[0]):.8f} float64 {ref_losses[s]:.8f}")
        assert float(out[1]) == float(T.isfinite().sum())
        if s == 0:
            assert abs(float(out[0]) - ref_losses[0]) <= 1e-5 * max(1.0, abs(ref_losses[0]))
            assert abs(float(loss_mod) - ref_losses[0]) <= 1e-5 * max(1.0, abs(ref_losses[0]))
        else:
            assert abs(float(out[0]) - ref_losses[1]) <= 5e-4 * max(1.0, abs(ref_losses[1]))
        if kind == "qm9":
            assert str(tr.last_route).startswith("mega16"), tr.last_route
        else:
            assert not str(tr.last_route).startswith("mega"), tr.last_route
        grads = [tr.sync.views[i].detach().cpu().clone() for i in range(len(names))]
        my_grads.append(grads)
        if s == 0:
            for k, gf in zip(names, grads):
                e_ref, e_mod = parity_err(gf.numpy(), ref_grads[0][k].numpy()), parity_err(gf.numpy(), mod_grads[k].numpy())
                print(f"SPECSTEP {cid} d{k}: vs float64 {e_ref:.2e}, vs module path {e_mod:.2e}, max|ref| {float(ref_grads[0][k].abs().max()):.2e}")
                assert e_ref <= 2e-5 and e_mod <= 2e-5, (k, e_ref, e_mod)
                assert parity_err(mod_grads[k].numpy(), ref_grads[0][k].numpy()) <= 2e-5, k
    want = _adam_reference(p0, my_grads)
    arrs = {f"g{s}.{k}": ref_grads[s][k].numpy() for s in range(2) for k in names}
    for k, p, wnt in zip(names, [p for _, p in model.named_parameters() if p.requires_grad], want):
        got = p.detach().cpu().numpy()
        assert parity_err(got, wnt.numpy()) <= 2e-6, k
        assert parity_err_where(got, ref_params[k].numpy(), adam_comparable(arrs, k, 2)) <= 2e-4, k
    assert int(model.bn.num_batches_tracked) == 2


def test_the_module_path_on_torch_ops_agrees(gpu_device, monkeypatch):
    """What such a model ran on before: ``head_loss`` switched off, the mirrors' ``train_step`` and ``masked_loss`` on torch ops — the
    same loss as the one node within the suite's 1e-5."""
    import chemprop_amd.model as cm

    model = _model("qm9", "wasserstein", "exp", 0.5 / T_SPEC).to(gpu_device).train()
    _, bmg, T, w = _batch(24, "qm9")
    bmg.to(gpu_device)
    Tg, wg = T.to(gpu_device), w.to(gpu_device)
    state = copy.deepcopy(model.state_dict())
    one_node = float(model.loss(bmg, Tg, wg))
    model.load_state_dict(state)
    monkeypatch.setattr(cm, "head_loss", lambda *a, **k: None)
    ops = model.loss(bmg, Tg, wg)
    assert type(ops.grad_fn).__name__ != "_HeadLossBackward"
    assert abs(float(ops) - one_node) <= 1e-5 * max(1.0, abs(one_node))


@pytest.mark.parametrize("what", ["ffn-dropout", "block-dropout-lean"])
def test_the_step_composes_with_dropout(what, gpu_device):
    """A spectral model with predictor dropout (p = 0.2), and one with dropout inside a ReLU block on 12 ZINC-shaped molecules (beyond
    the tile: the lean step kernels): the step runs and its loss is finite (the masks have their own tests)."""
    from chemprop_amd.model import FusedTrainer

    lean = what == "block-dropout-lean"
    kind, n = ("zinc", 12) if lean else ("qm9", 24)
    model = _model(kind, "sid" if lean else "wasserstein", "softplus", dropout=0.0 if lean else 0.2, act="relu" if lean else "tanh",
                   mp_dropout=0.1 if lean else 0.0).to(gpu_device).train()
    _, bmg, T, w = _batch(n, kind)
    bmg.to(gpu_device)
    tr = FusedTrainer(model, lr=LR, ffn_dropout=True)
    assert tr.head.kind == ("sid" if lean else "wasserstein") and tr.head.drop.p == (0.0 if lean else 0.2)
    out = tr.step(bmg, T.to(gpu_device), w.to(gpu_device), clip=(1.0, "norm"))
    torch.cuda.synchronize()
    assert math.isfinite(float(out[0])) and float(out[1]) == float(T.isfinite().sum())
    assert str(tr.last_route).startswith("fused16/lean" if lean else "mega16"), tr.last_route
    assert all(bool(torch.isfinite(p).all()) for p in model.parameters())
