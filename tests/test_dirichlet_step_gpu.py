"""Dirichlet classification heads on the one-call step (``FusedTrainer.step`` -> ``dmpnn_train_step``) and on the module path's
one-node head (``MPNN.loss`` -> ``head_loss`` -> ``_HeadLoss``), against a float64 restatement of the whole model on the CPU: the block
through ``oracle.dmpnn_torch.forward``, the head (aggregation, batch norm on batch statistics, the MLP, ``DirichletLoss`` on
``softplus + 1``) through this file's own ops, Adam through ``torch.optim.Adam`` in float64.

Bars: those of ``tests/test_model.py::test_fused_step_at_size_vs_restatement_and_module_path`` — the loss within ``1e-5 max(1, |ref|)``,
every gradient within ``parity_err <= 2e-5``.  That test holds no parameters; for the parameters after two Adam steps the suite's own
two bars are used (``tests/test_model.py``): ``2e-6`` against Adam on the CPU fed with the gradients the kernels produced (the update
itself), and the functional ``2e-4`` against the float64 restatement's own two steps on the entries ``conftest.adam_comparable`` keeps
(Adam normalises a gradient by its magnitude: an entry whose gradient is rounding noise moves by ``lr`` in the noise's direction).

The two batches: 24 QM9-shaped molecules (the tile kernels) and 12 ZINC-shaped ones (molecules beyond the tile: the per-step route the
engine's rule picks, ``fused`` at this size).  The lean step kernels are the home of block dropout beyond the tile; their masks are
not restated here — the composition test below runs a Dirichlet model on them.

The definitions restated here are chemprop 2.3.1's as ``include/dmpnn.h`` states them; they were not run against the reference's code."""
import copy
import math

import pytest
import torch

from conftest import adam_comparable, parity_err, parity_err_where

F = torch.nn.functional
pytestmark = pytest.mark.gpu
LR = 1e-3


def _model(head, kind, d_xd=0, dropout=0.0, seed=7, act="tanh", mp_dropout=0.0):
    from chemprop_amd import agg as cagg
    from chemprop_amd.model import MPNN, BinaryDirichletFFN, Dirichlet, MulticlassDirichletFFN
    from chemprop_amd.nn import BondMessagePassing

    torch.manual_seed(seed)
    d_h = 64
    mp = BondMessagePassing(d_h=d_h, depth=3, activation=act, dropout=mp_dropout)
    kw = dict(input_dim=d_h + d_xd, hidden_dim=32, n_layers=1, dropout=dropout, activation=act)
    if head == "binary":
        pred = BinaryDirichletFFN(n_tasks=3, criterion=Dirichlet(torch.tensor([0.5, 1.0, 1.5]), v_kl=0.2), **kw)
    else:
        pred = MulticlassDirichletFFN(4, n_tasks=2, criterion=Dirichlet(torch.tensor([1.25, 0.75]), v_kl=0.3), **kw)
    agg = cagg.MeanAggregation() if kind == "qm9" else cagg.NormAggregation()
    return MPNN(mp, agg, pred, batch_norm=True).train()


def _batch(n, kind, K, t, seed=41):
    from chemprop_amd import synth

    gen = torch.Generator().manual_seed(seed)
    T = torch.randint(0, K, (n, t), generator=gen).float()
    T[torch.rand(n, t, generator=gen) < 0.15] = float("nan")
    return synth.random_batch(n, kind, seed=seed), synth.random_batch(n, kind, seed=seed), T, 0.5 + torch.rand(n, 1, generator=gen)


def dirichlet_loss64(Y, T, w, tw, K, v_kl):
    """``DirichletLoss`` (unreduced, then ``sum(L w_row w_task [finite]) / #finite``) on the raw outputs ``Y [B, t K]``."""
    B, t = T.shape
    mask = T.isfinite()
    y = F.one_hot(torch.where(mask, T, torch.zeros_like(T)).long(), K).to(Y.dtype)
    alpha = F.softplus(Y.reshape(B, t, K)) + 1
    S = alpha.sum(-1, keepdim=True)
    p = alpha / S
    L = ((y - p) ** 2).sum(-1) + (p * (1 - p) / (S + 1)).sum(-1)
    a_t = y + (1 - y) * alpha
    S_t = a_t.sum(-1, keepdim=True)
    L = L + v_kl * (torch.lgamma(S_t).squeeze(-1) - torch.lgamma(a_t).sum(-1) - math.lgamma(K)
                    + ((a_t - 1) * (torch.digamma(a_t) - torch.digamma(S_t))).sum(-1))
    return (torch.where(mask, L, torch.zeros_like(L)) * w.view(-1, 1) * tw.view(1, -1)).sum() / mask.sum()


def fingerprint64(m, bmg):
    """Block, aggregation and batch norm (batch statistics) of the float64 copy ``m`` on the CPU batch ``bmg``."""
    from oracle import dmpnn_torch as od

    mp = m.message_passing
    w = od.MPWeights(mp.W_i.weight, mp.W_h.weight, mp.W_o.weight, mp.W_o.bias)
    Hv = od.forward(bmg.V.double(), bmg.E.double(), bmg.edge_index, bmg.rev_edge_index, w, depth=mp.depth, activation="tanh")
    n = len(bmg)
    H = torch.zeros(n, Hv.shape[1], dtype=torch.float64).index_add(0, bmg.batch, Hv)
    if getattr(m.agg, "mode", None) == "mean":
        H = H / torch.bincount(bmg.batch, minlength=n).clamp(min=1).double().view(-1, 1)
    else:
        assert m.agg.mode == "norm"
        H = H / m.agg.norm
    return H


def raw64(m, Z):
    for l, blk in enumerate(m.predictor.ffn):
        Z = F.linear(torch.tanh(Z) if l else Z, blk[-1].weight, blk[-1].bias)
    return Z


def float64_steps(model, bmg, T, w, K, steps=2):
    """``steps`` training steps of a float64 copy of ``model`` on the CPU; per step the loss and the gradients by name, then the
    parameters after the last one."""
    m = copy.deepcopy(model).cpu().double().train()
    opt = torch.optim.Adam([p for p in m.parameters()], LR)
    losses, grads = [], []
    for _ in range(steps):
        opt.zero_grad()
        H = fingerprint64(m, bmg)
        Z = F.batch_norm(H, m.bn.running_mean, m.bn.running_var, m.bn.weight, m.bn.bias, training=True, momentum=m.bn.momentum, eps=m.bn.eps)
        c = m.predictor.criterion
        loss = dirichlet_loss64(raw64(m, Z), T.double(), w.double(), c.task_weights.reshape(-1), K, c.v_kl)
        loss.backward()
        losses.append(float(loss.detach()))
        grads.append({k: p.grad.clone() for k, p in m.named_parameters()})
        opt.step()
    return losses, grads, {k: p.detach() for k, p in m.named_parameters()}, m


def _adam_reference(params0, grads_per_step):
    ps = [p.clone().requires_grad_(True) for p in params0]
    opt = torch.optim.Adam(ps, LR)
    for gs in grads_per_step:
        for p, gr in zip(ps, gs):
            p.grad = gr.clone()
        opt.step()
    return [p.detach() for p in ps]


CASES = [("qm9x24-binary-t3", 24, "qm9", "binary", 2, 3), ("zincx12-K4-t2", 12, "zinc", "multi", 4, 2)]


@pytest.mark.parametrize("cid,n,kind,head,K,t", CASES, ids=[c[0] for c in CASES])
def test_one_call_step_and_module_path_against_float64(cid, n, kind, head, K, t, gpu_device):
    """Two ``FusedTrainer.step`` calls: losses, every gradient of the first step and the parameters after the second against the
    float64 restatement; the module path's loss is ONE ``_HeadLoss`` node and its gradients equal the one-call step's."""
    from chemprop_amd.model import FusedTrainer, HeadSpec

    cpu_model = _model(head, kind)
    cpu_bmg, bmg, T, w = _batch(n, kind, K, t)
    ref_losses, ref_grads, ref_params, _ = float64_steps(cpu_model, cpu_bmg, T, w, K)

    model = copy.deepcopy(cpu_model).to(gpu_device).train()
    bmg.to(gpu_device)
    Tg, wg = T.to(gpu_device), w.to(gpu_device)
    state = copy.deepcopy(model.state_dict())
    # the module path first (it leaves the parameters alone)
    loss_mod = model.loss(bmg, Tg, wg)
    assert type(loss_mod.grad_fn).__name__ == "_HeadLossBackward", type(loss_mod.grad_fn).__name__
    spec = model.__dict__["_dmpnn_head_spec"][1]
    assert isinstance(spec, HeadSpec) and (spec.kind, spec.n_classes, spec.n_tasks) == ("dirichlet", K, t)
    loss_mod.backward()
    mod_grads = {k: p.grad.detach().cpu().clone() for k, p in model.named_parameters()}
    model.load_state_dict(state)   # (the module path's forward updated the running statistics once)
    model.zero_grad(set_to_none=True)

    tr = FusedTrainer(model, lr=LR)
    names = [k for k, p in model.named_parameters() if p.requires_grad]
    p0 = [p.detach().cpu().clone() for _, p in model.named_parameters() if p.requires_grad]
    my_grads = []
    for s in range(2):
        out = tr.step(bmg, Tg, wg)
        torch.cuda.synchronize()
        print(f"DIRSTEP {cid} step {s} route {tr.last_route} loss {float(out[0]):.8f} float64 {ref_losses[s]:.8f}")
        assert float(out[1]) == float(T.isfinite().sum())
        if s == 0:
            assert abs(float(out[0]) - ref_losses[0]) <= 1e-5 * max(1.0, abs(ref_losses[0]))
            assert abs(float(loss_mod) - ref_losses[0]) <= 1e-5 * max(1.0, abs(ref_losses[0]))
        else:   # (parameters after ONE Adam step: the functional bar of tests/test_model.py::test_fused_step_matches_goldens)
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
                print(f"DIRSTEP {cid} d{k}: vs float64 {e_ref:.2e}, vs module path {e_mod:.2e}, max|ref| {float(ref_grads[0][k].abs().max()):.2e}")
                assert e_ref <= 2e-5 and e_mod <= 2e-5, (k, e_ref, e_mod)
                assert parity_err(mod_grads[k].numpy(), ref_grads[0][k].numpy()) <= 2e-5, k
    want = _adam_reference(p0, my_grads)
    arrs = {f"g{s}.{k}": ref_grads[s][k].numpy() for s in range(2) for k in names}
    for k, p, wnt in zip(names, [p for _, p in model.named_parameters() if p.requires_grad], want):
        got = p.detach().cpu().numpy()
        assert parity_err(got, wnt.numpy()) <= 2e-6, k
        assert parity_err_where(got, ref_params[k].numpy(), adam_comparable(arrs, k, 2)) <= 2e-4, k
    assert int(model.bn.num_batches_tracked) == 2


@pytest.mark.parametrize("what", ["ffn-dropout", "x_d", "block-dropout-lean"])
def test_the_step_composes_with_dropout_and_descriptors(what, gpu_device):
    """No new switch: ``FusedTrainer(..., ffn_dropout=True)`` takes a Dirichlet model with predictor dropout (p = 0.2), one with
    molecule descriptors (``d_xd`` = 8) and one with dropout inside a ReLU block on 12 ZINC-shaped molecules (beyond the tile: the lean
    step kernels); the step's loss is finite.  (The mask arithmetic and the descriptors' path have their own tests.)"""
    from chemprop_amd.model import FusedTrainer

    lean = what == "block-dropout-lean"
    kind, n = ("zinc", 12) if lean else ("qm9", 24)
    model = _model("multi", kind, d_xd=8 if what == "x_d" else 0, dropout=0.2 if what == "ffn-dropout" else 0.0, act="relu" if lean else "tanh",
                   mp_dropout=0.1 if lean else 0.0).to(gpu_device).train()
    _, bmg, T, w = _batch(n, kind, 4, 2)
    bmg.to(gpu_device)
    X = torch.randn(n, 8, generator=torch.Generator().manual_seed(3)).to(gpu_device) if what == "x_d" else None
    tr = FusedTrainer(model, lr=LR, ffn_dropout=True)
    assert tr.head.kind == "dirichlet" and tr.head.drop.p == (0.2 if what == "ffn-dropout" else 0.0) and tr.head.d_xd == (8 if what == "x_d" else 0)
    out = tr.step(bmg, T.to(gpu_device), w.to(gpu_device), X_d=X, clip=(1.0, "norm"))
    torch.cuda.synchronize()
    assert math.isfinite(float(out[0])) and float(out[1]) == float(T.isfinite().sum())
    assert str(tr.last_route).startswith("fused16/lean" if lean else "mega16"), tr.last_route
    assert all(bool(torch.isfinite(p).all()) for p in model.parameters())


def test_predict_falls_back_to_the_modules_and_stays_correct(gpu_device):
    """``MPNN.predict`` on the binary model: ``PredictSpec`` refuses it, the modules answer ``(p_1, 2 / S) [B, t, 2]`` — equal to the
    mirror's eval-mode ``forward`` in float64 on the same fingerprint."""
    from chemprop_amd.predict import predict_spec

    model = _model("binary", "qm9").to(gpu_device).eval()
    _, bmg, _, _ = _batch(24, "qm9", 2, 3)
    bmg.to(gpu_device)
    assert predict_spec(model) is None
    got = model.predict(bmg)
    assert tuple(got.shape) == (24, 3, 2) and not got.requires_grad
    with torch.no_grad():
        fp = model.fingerprint(bmg).cpu().double()
        m64 = copy.deepcopy(model).cpu().double()
        alpha = F.softplus(raw64(m64, fp)).reshape(24, 3, 2) + 1
        S = alpha.sum(-1)
        want = torch.stack((alpha[..., 1] / S, 2 / S), 2)
    assert parity_err(got.cpu().numpy(), want.numpy()) <= 2e-5
    assert float(got[..., 0].min()) > 0 and float(got[..., 0].max()) < 1 and float(got[..., 1].max()) <= 1
