"""A SELU model (block and predictor: ``chemprop train --activation selu``) on the one-call step: ``FusedTrainer.step``, the module
path ``MPNN.loss().backward()`` + ``FlatAdam.step`` (``head_loss`` + ``FusedMP``) and a float64 restatement of the whole model — loss,
every gradient and the parameters after one Adam step — at 64 QM9-shaped molecules (the tile route), at 20 ZINC-shaped ones (beyond
the tile) and, with ``p = 0.2`` inside the block and ``rows_dropout=True``, the row kernels given the step's masks.

The restatement is ``tests/test_dropout_gpu.py``'s ``_restated_forward`` on a double copy of the model (``nn.SELU`` is ``F.selu``),
``oracle.agg_torch``, ``F.batch_norm``, ``oracle.ffn_torch.mlp_forward`` with ``F.selu`` and the model's criterion, then
``torch.optim.Adam``; run in float32 it is the yardstick.  Adam's ``eps`` is 1e-4 on every side, as in ``tests/test_attentive_step_gpu.py``:
with 1e-8 the first step is ``lr sign(g)``, which turns the rounding of a gradient entry near zero (there are some below 1e-6 here) into
``lr`` — the float32 restatement itself then misses float64 by more than the cap.  Every case asserts on the block's float64 pre-activations: at every site a
quarter negative and a quarter positive, one below -5, one exactly 0 (the synthetic features scaled by 8 — by 4 the freshly initialised
block stays above -5 at 64 QM9-shaped molecules — and row ``C0`` of ``W_i`` zeroed: see ``tests/test_selu_block_gpu.py``).

Judged by the suite's rule: ``err = max|got - ref| / max|ref|`` within ``min(rows_harness.MARGIN max(e32, 2**-23), cap)``, caps 1e-5
(loss, parameters) and 2e-5 (gradients); one ``SELUBAR`` line per tensor printed before judging.  Measured on the MI355X (126
comparisons): the worst ``err / max(e32, 2**-23)`` is 2.59 — ``W_h`` after the Adam step at 20 ZINC-shaped molecules, the one-call step and
the module path alike (err 3.1e-7 against a float32 draw of 1.1e-7) — then 2.24 (the gradient of ``W_o``'s bias there: 7.6e-6 against
3.4e-6, a sum the batch norm behind it nearly cancels; its bar is the cap, 2e-5)."""
import copy
import types

import pytest
import torch
import torch.nn.functional as F

import rows_harness as rh
from chemprop_amd import _lib
from test_dropout_gpu import ReplayDropout, _restated_forward
from test_rows_dropout_gpu import _masks, _scale32

pytestmark = pytest.mark.gpu

LR, ADAM_EPS, SCALE, C0, D_H = 1e-4, 1e-4, 8.0, 1, 64   # (lr: the trainer's default)
CASES = {"qm9-64-tile": (64, "qm9", 0.0), "zinc-20-beyond-the-tile": (20, "zinc", 0.0), "qm9-64-rows-dropout": (64, "qm9", 0.2),
         "zinc-20-rows-dropout": (20, "zinc", 0.2)}


def _report(s):
    print(s.replace("ROWSBAR", "SELUBAR"))


def _model(p):
    from chemprop_amd import agg as cagg
    from chemprop_amd.model import MPNN, RegressionFFN
    from chemprop_amd.nn import BondMessagePassing

    torch.manual_seed(31)
    mp = BondMessagePassing(d_h=D_H, activation="selu", dropout=p)
    model = MPNN(mp, cagg.MeanAggregation(), RegressionFFN(n_tasks=2, input_dim=D_H, hidden_dim=32, activation="selu"), batch_norm=True)
    with torch.no_grad():
        mp.W_i.weight[C0] = 0.0
        model.bn.weight.uniform_(0.5, 1.5), model.bn.bias.uniform_(-0.5, 0.5)
    assert type(mp.tau) is torch.nn.SELU and type(model.predictor.ffn[1][0]) is torch.nn.SELU
    return model.train()


def _batch(n, kind):
    from chemprop_amd import synth

    bmg = synth.random_batch(n, kind, seed=17)
    bmg.V, bmg.E = bmg.V * SCALE, bmg.E * SCALE
    y = torch.randn(n, 2, generator=torch.Generator().manual_seed(18))
    return bmg, y


class _Rec(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.pre = []

    def forward(self, z):
        self.pre.append(z.detach())
        return F.selu(z)


def _restate(before, cpu, y, p, keeps, dtype):
    """The whole step in ``dtype`` on the CPU -> (named tensors: loss, every gradient ``g.<name>``, every parameter after one Adam step
    ``p.<name>``; the block's pre-activations)."""
    from chemprop_amd.model import criterion_loss
    from oracle import agg_torch, ffn_torch

    ref = copy.deepcopy(before).cpu().to(dtype)
    rec = ref.message_passing.tau = _Rec()
    g = types.SimpleNamespace(V=cpu.V.to(dtype), E=cpu.E.to(dtype), edge_index=cpu.edge_index, rev_edge_index=cpu.rev_edge_index)
    drop = (lambda x: x) if keeps is None else ReplayDropout(p, [k.to(dtype) * _scale32(p) for k in keeps])
    Hv = _restated_forward(g, ref.message_passing, drop)
    H = agg_torch.mean(Hv, cpu.batch)
    H = F.batch_norm(H, ref.bn.running_mean.clone(), ref.bn.running_var.clone(), ref.bn.weight, ref.bn.bias, True, ref.bn.momentum, ref.bn.eps)
    lin = [m for m in ref.predictor.ffn.modules() if isinstance(m, torch.nn.Linear)]
    preds = ffn_torch.mlp_forward(H, [m.weight for m in lin], [m.bias for m in lin], F.selu)
    loss = criterion_loss(ref.criterion, preds, y.to(dtype))
    loss.backward()
    out = {"loss": loss.detach().reshape(1)}
    out.update({"g." + k: q.grad.clone() for k, q in ref.named_parameters()})
    torch.optim.Adam(ref.parameters(), lr=LR, eps=ADAM_EPS).step()
    out.update({"p." + k: q.detach().clone() for k, q in ref.named_parameters()})
    return out, rec.pre


def _condition(pre, name):
    for i, z in enumerate(pre):
        n = z.numel()
        assert int((z < 0).sum()) * 4 >= n and int((z > 0).sum()) * 4 >= n, (name, i)
    assert any(bool((z < -5).any()) for z in pre), name
    assert bool((pre[0][:, C0] == 0).all()), name


def _kinds(t):
    return {k: ("grad" if k.startswith("g.") else "fwd") for k in t}


def _expected_route(bmg, p):
    from chemprop_amd import engine

    nV, nE, n = int(bmg.V.shape[0]), int(bmg.E.shape[0]), len(bmg)
    info = engine.train_route(nV, nE, int(bmg.V.shape[1]), int(bmg.E.shape[1]), D_H, 3, "selu", n, dropout_p=p, have_batch=True,
                              oversize=getattr(bmg, "oversize", None), max_level=1 if nE > 30 * n else 2)
    return _lib.ROUTES[info.route]


@pytest.mark.parametrize("name", list(CASES))
def test_selu_one_call_step(name, gpu_device):
    from chemprop_amd import distributed as ddp
    from chemprop_amd.model import FusedTrainer
    from chemprop_amd.optim import FlatAdam

    n, kind, p = CASES[name]
    dev = gpu_device
    cpu, y = _batch(n, kind)
    before = _model(p)
    model = copy.deepcopy(before).to(dev).train()
    bmg, _ = _batch(n, kind)
    bmg.to(dev)
    if p:
        rng = torch.get_rng_state()
        with pytest.raises(NotImplementedError, match="rows_dropout"):     # (refused at construction: no seed was drawn)
            FusedTrainer(copy.deepcopy(model), lr=LR)
        assert torch.equal(torch.get_rng_state(), rng)
    tr = FusedTrainer(model, lr=LR, eps=ADAM_EPS, rows_dropout=bool(p))
    torch.manual_seed(99)
    first = int(torch.randint(0, 2 ** 62, (1,), dtype=torch.int64).item())
    torch.manual_seed(99)
    loss = tr.step(bmg, y.to(dev))
    torch.cuda.synchronize()
    nV, nE = int(cpu.V.shape[0]), int(cpu.E.shape[0])
    keeps = None
    if p:
        assert tr.last_dropout_seed == first and tr.last_route == "general16", (tr.last_route, tr.last_dropout_seed)
        keeps = _masks(first, p, 3, nE, nV, D_H)
    else:
        assert tr.last_route == _expected_route(cpu, 0.0), (tr.last_route, _expected_route(cpu, 0.0))
        assert tr.last_route == ("mega16" if kind == "qm9" else tr.last_route) and tr.last_route != "rows"
    ref, pre = _restate(before, cpu, y, p, keeps, torch.float64)
    _condition(pre, name)
    e32 = rh.yardstick(ref, _restate(before, cpu, y, p, keeps, torch.float32)[0])
    got = {"loss": loss[:1].detach().cpu()}
    got.update({"g." + k: tr._views[id(q)].detach().cpu().clone() for k, q in model.named_parameters()})
    got.update({"p." + k: q.detach().cpu().clone() for k, q in model.named_parameters()})
    assert set(got) == set(ref)
    fails = rh.compare(f"selu-step-{name}", got, ref, e32, _kinds(ref), report=_report)
    assert not fails, f"{name}: " + "; ".join(fails)
    if p:
        return
    # the module path on the same parameters: MPNN.loss().backward() + FlatAdam.step (head_loss + FusedMP)
    m2 = copy.deepcopy(before).to(dev).train()
    sync = ddp.GradSync(list(m2.parameters()), modules=[m2])
    opt = FlatAdam(sync, lr=LR, eps=ADAM_EPS)
    with ddp.backward_on_calling_thread():
        sync.zero_grad()
        l2 = m2.loss(bmg, y.to(dev))
        l2.backward()
    sync.allreduce()
    grads2 = {"g." + k: q.grad.detach().cpu().clone() for k, q in m2.named_parameters()}
    opt.step()
    sync.wait()
    torch.cuda.synchronize()
    assert str(m2.message_passing.__dict__.get("_dmpnn_route")) != "rows", "the module path of a SELU block is the fused one (FusedMP), not the row chain"
    got2 = {"loss": l2.detach().reshape(1).cpu(), **grads2, **{"p." + k: q.detach().cpu().clone() for k, q in m2.named_parameters()}}
    fails = rh.compare(f"selu-module-path-{name}", got2, ref, e32, _kinds(ref), report=_report)
    assert not fails, f"{name} (module path): " + "; ".join(fails)


def test_selu_model_predicts_on_the_inference_head(gpu_device):
    """``MPNN.predict`` of the SELU model in eval mode goes through ``fused_predict`` (one ``dmpnn_predict_head`` call behind the
    block) and equals the module forward at the suite's ``TOL``."""
    from chemprop_amd.predict import fused_predict
    from conftest import TOL, parity_err

    dev = gpu_device
    model = _model(0.0).to(dev).eval()
    bmg, _ = _batch(64, "qm9")
    bmg.to(dev)
    with torch.no_grad():
        r = fused_predict(model, bmg)
        assert r is not None, "the inference head refused a SELU model"
        want = model(bmg)
    err = parity_err(r.preds.cpu().numpy(), want.cpu().numpy())
    print(f"SELUPREDICT err={err:.3e} bar={TOL:.1e}")
    assert err <= TOL
    assert parity_err(model.predict(bmg).cpu().numpy(), want.cpu().numpy()) <= TOL
