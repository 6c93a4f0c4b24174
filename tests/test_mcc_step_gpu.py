"""Binary MCC heads on the one-call step (``FusedTrainer.step`` -> ``dmpnn_train_step``), on the module path's one-node head
(``MPNN.loss`` -> ``head_loss`` -> ``_HeadLoss``) and under ``HipMPNN``, against (a) a float64 restatement of the whole model on the CPU
— the block through ``oracle.dmpnn_torch.forward``, the head through ``tests/test_dirichlet_step_gpu.py``'s ops, the criterion through
``tests/test_mcc_head.py``'s restatement of ``include/dmpnn.h``, Adam through ``torch.optim.Adam`` in float64 — and (b) the module path on
torch ops (``head_loss`` switched off: what such a model trained on before ``DMPNN_LOSS_MCC``) with ``torch.optim.Adam`` on the device.

The model: ``d_h`` 64, depth 3, one hidden layer of 32, batch norm, tanh, a ``BinaryClassificationFFN`` of 12 tasks with ``BinaryMCC``
and task weights.  Batches: 64 QM9-shaped molecules (the tile kernels) and 8 ZINC-shaped ones (molecules beyond the tile: the per-step
route), about 30 % positives, 15 % missing targets.

Bars: those of ``tests/test_dirichlet_step_gpu.py`` / ``tests/test_spectral_step_gpu.py`` — the loss within ``1e-5 max(1, |ref|)``
(``5e-4`` once the parameters have moved), predictions and every gradient within ``parity_err <= 2e-5``, the parameters after one and
after three Adam steps within ``2e-6`` of Adam on the CPU fed with the kernels' gradients and within ``2e-4`` of the float64
restatement's and of the module path's own steps on the entries ``conftest.adam_comparable`` keeps."""
import copy
import types

import pytest
import torch

from conftest import adam_comparable, parity_err, parity_err_where
from test_dirichlet_step_gpu import LR, _adam_reference, fingerprint64, raw64
from test_mcc_head import mcc_criterion
from test_multicomponent_integration import stub_chemprop  # noqa: F401  (the fixture)

F = torch.nn.functional
pytestmark = pytest.mark.gpu
TASKS, STEPS = 12, 3


def _model(kind, seed=7):
    from chemprop_amd import agg as cagg
    from chemprop_amd.model import MPNN, BinaryClassificationFFN, BinaryMCC
    from chemprop_amd.nn import BondMessagePassing

    torch.manual_seed(seed)
    d_h = 64
    mp = BondMessagePassing(d_h=d_h, depth=3, activation="tanh")
    tw = 0.5 + torch.rand(TASKS, generator=torch.Generator().manual_seed(seed + 1))
    pred = BinaryClassificationFFN(n_tasks=TASKS, input_dim=d_h, hidden_dim=32, n_layers=1, activation="tanh", criterion=BinaryMCC(tw))
    agg = cagg.MeanAggregation() if kind == "qm9" else cagg.NormAggregation()
    return MPNN(mp, agg, pred, batch_norm=True).train()


def _batch(n, kind, seed=41):
    from chemprop_amd import synth

    gen = torch.Generator().manual_seed(seed)
    T = (torch.rand(n, TASKS, generator=gen) < 0.3).float()
    T[torch.rand(n, TASKS, generator=gen) < 0.15] = float("nan")
    return synth.random_batch(n, kind, seed=seed), synth.random_batch(n, kind, seed=seed), T, 0.5 + torch.rand(n, 1, generator=gen)


def float64_steps(model, bmg, T, w, steps=STEPS):
    m = copy.deepcopy(model).cpu().double().train()
    opt = torch.optim.Adam([p for p in m.parameters()], LR)
    losses, grads, raws, params = [], [], [], []
    for _ in range(steps):
        opt.zero_grad()
        H = fingerprint64(m, bmg)
        Z = F.batch_norm(H, m.bn.running_mean, m.bn.running_var, m.bn.weight, m.bn.bias, training=True, momentum=m.bn.momentum, eps=m.bn.eps)
        raw = raw64(m, Z)
        loss = mcc_criterion(raw, T.double(), w.double().reshape(-1), m.predictor.criterion.task_weights.reshape(-1))
        loss.backward()
        losses.append(float(loss.detach()))
        raws.append(raw.detach())
        grads.append({k: p.grad.clone() for k, p in m.named_parameters()})
        opt.step()
        params.append({k: p.detach().clone() for k, p in m.named_parameters()})
    return losses, grads, raws, params


def module_path_steps(model, bmg, T, w, monkeypatch, steps=STEPS):
    """``steps`` of ``MPNN.loss(...).backward()`` on TORCH OPS behind the block (``head_loss`` off) with ``torch.optim.Adam`` on a copy."""
    import chemprop_amd.model as cm

    m = copy.deepcopy(model).train()
    opt = torch.optim.Adam([p for p in m.parameters()], LR)
    raws = []
    hook = m.predictor.ffn.register_forward_hook(lambda mod, inp, out: raws.append(out.detach().cpu()))
    losses, grads, params = [], [], []
    with monkeypatch.context() as mk:
        mk.setattr(cm, "head_loss", lambda *a, **k: None)
        for _ in range(steps):
            opt.zero_grad()
            loss = m.loss(bmg, T, w)
            assert type(loss.grad_fn).__name__ != "_HeadLossBackward"
            loss.backward()
            losses.append(float(loss.detach()))
            grads.append({k: p.grad.detach().cpu().clone() for k, p in m.named_parameters()})
            opt.step()
            params.append({k: p.detach().cpu().clone() for k, p in m.named_parameters()})
    hook.remove()
    return losses, grads, raws, params


CASES = [("qm9x64", 64, "qm9"), ("zincx8", 8, "zinc")]


@pytest.mark.parametrize("cid,n,kind", CASES, ids=[c[0] for c in CASES])
def test_one_call_step_against_float64_and_the_module_path(cid, n, kind, gpu_device, monkeypatch):
    from chemprop_amd.model import FusedTrainer, HeadSpec

    cpu_model = _model(kind)
    cpu_bmg, bmg, T, w = _batch(n, kind)
    ref_losses, ref_grads, ref_raws, ref_params = float64_steps(cpu_model, cpu_bmg, T, w)

    model = copy.deepcopy(cpu_model).to(gpu_device).train()
    bmg.to(gpu_device)
    Tg, wg = T.to(gpu_device), w.to(gpu_device)
    mod_losses, mod_grads, mod_raws, mod_params = module_path_steps(model, bmg, Tg, wg, monkeypatch)

    # the module path's ONE node for everything behind the block (it leaves the parameters alone)
    state = copy.deepcopy(model.state_dict())
    loss_node = model.loss(bmg, Tg, wg)
    assert type(loss_node.grad_fn).__name__ == "_HeadLossBackward", type(loss_node.grad_fn).__name__
    spec = model.__dict__["_dmpnn_head_spec"][1]
    assert isinstance(spec, HeadSpec) and (spec.kind, spec.n_classes, spec.n_tasks) == ("mcc", 0, TASKS)
    loss_node.backward()
    node_grads = {k: p.grad.detach().cpu().clone() for k, p in model.named_parameters()}
    model.load_state_dict(state)
    model.zero_grad(set_to_none=True)

    tr = FusedTrainer(model, lr=LR)
    assert tr.head.kind == "mcc"
    names = [k for k, p in model.named_parameters() if p.requires_grad]
    p0 = [p.detach().cpu().clone() for _, p in model.named_parameters() if p.requires_grad]
    arrs = {f"g{s}.{k}": ref_grads[s][k].numpy() for s in range(STEPS) for k in names}
    my_grads = []
    for s in range(STEPS):
        out = tr.step(bmg, Tg, wg)
        torch.cuda.synchronize()
        print(f"MCCSTEP {cid} step {s} route {tr.last_route} loss {float(out[0]):.8f} float64 {ref_losses[s]:.8f} torch ops {mod_losses[s]:.8f}")
        assert float(out[1]) == float(T.isfinite().sum())
        tol = 1e-5 if s == 0 else 5e-4
        assert abs(float(out[0]) - ref_losses[s]) <= tol * max(1.0, abs(ref_losses[s]))
        assert abs(float(out[0]) - mod_losses[s]) <= tol * max(1.0, abs(mod_losses[s]))
        if kind == "qm9":
            assert str(tr.last_route).startswith("mega16"), tr.last_route
        else:
            assert not str(tr.last_route).startswith("mega"), tr.last_route
        my_grads.append([tr.sync.views[i].detach().cpu().clone() for i in range(len(names))])
        if s == 0:
            assert abs(float(loss_node) - ref_losses[0]) <= 1e-5 * max(1.0, abs(ref_losses[0]))
            preds = tr.preds.detach().cpu().reshape(n, TASKS)
            e_ref, e_mod = parity_err(preds.numpy(), ref_raws[0].numpy()), parity_err(preds.numpy(), mod_raws[0].numpy())
            print(f"MCCSTEP {cid} preds: vs float64 {e_ref:.2e}, vs torch ops {e_mod:.2e}")
            assert e_ref <= 2e-5 and e_mod <= 2e-5
            for k, gf in zip(names, my_grads[0]):
                e_ref, e_mod = parity_err(gf.numpy(), ref_grads[0][k].numpy()), parity_err(gf.numpy(), mod_grads[0][k].numpy())
                e_node = parity_err(gf.numpy(), node_grads[k].numpy())
                print(f"MCCSTEP {cid} d{k}: vs float64 {e_ref:.2e}, vs torch ops {e_mod:.2e}, vs the one node {e_node:.2e}, "
                      f"max|ref| {float(ref_grads[0][k].abs().max()):.2e}")
                assert e_ref <= 2e-5 and e_mod <= 2e-5 and e_node <= 2e-5, (k, e_ref, e_mod, e_node)
        if s in (0, STEPS - 1):   # the parameters after one step and after three
            want = _adam_reference(p0, my_grads)
            for k, p, wnt in zip(names, [p for _, p in model.named_parameters() if p.requires_grad], want):
                got = p.detach().cpu().numpy()
                keep = adam_comparable(arrs, k, s + 1)
                assert parity_err(got, wnt.numpy()) <= 2e-6, (s, k)
                assert parity_err_where(got, ref_params[s][k].numpy(), keep) <= 2e-4, (s, k)
                assert parity_err_where(got, mod_params[s][k].numpy(), keep) <= 2e-4, (s, k)
    assert int(model.bn.num_batches_tracked) == STEPS


def test_hip_mpnn_takes_a_binary_mcc_model_on_the_one_call_route(stub_chemprop, gpu_device):  # noqa: F811
    from chemprop_amd.model import BinaryClassificationFFN, BinaryMCC

    S = stub_chemprop
    integ = S.integration
    integ.enable()
    HipM = integ.hip_mpnn_class()[1]
    torch.manual_seed(3)
    mp = S.mods["chemprop.nn"].BondMessagePassing(d_h=64)
    agg = S.mods["chemprop.nn"].agg.MeanAggregation()
    pred = BinaryClassificationFFN(n_tasks=TASKS, input_dim=64, criterion=BinaryMCC(torch.ones(TASKS)))
    model = HipM(mp, agg, pred, batch_norm=True, init_lr=1e-3).to(gpu_device).train()
    integ.accelerate(model)
    st = model._hip_state()
    assert st["fused"] is not None and st["why"] is None, st["why"]
    assert st["fused"].head.kind == "mcc"
    opt = model.configure_optimizers()["optimizer"]
    model._trainer = types.SimpleNamespace(optimizers=[opt], accumulate_grad_batches=1, gradient_clip_val=None, gradient_clip_algorithm=None,
                                           strategy=None)
    _, bmg, T, w = _batch(64, "qm9")
    bmg.to(gpu_device)
    before = {k: p.detach().clone() for k, p in model.named_parameters()}
    opt.step(lambda: model.training_step((bmg, None, None, T.to(gpu_device), w.to(gpu_device), None, None), 0))
    torch.cuda.synchronize()
    assert model.__dict__["_hip"]["route"].startswith("fused:"), model.__dict__["_hip"]
    for k in ("message_passing.W_h.weight", "predictor.ffn.0.0.weight", "predictor.ffn.1.2.weight"):
        assert not torch.equal(dict(model.named_parameters())[k].detach(), before[k]), k
