"""``MPNN.predict`` / ``fused_predict`` on an eval-mode ``BinaryClassificationFFN`` model trained with ``BinaryMCC``: the sigmoid
probabilities (``DMPNN_PT_SIGMOID``) and, with targets, the MCC ``val_loss`` — ``k_mcc_cols`` + ``k_mcc_finish`` without a gradient,
one workgroup — against the float64 restatement behind the block's own output (aggregation, eval-mode batch norm, the MLP, the
criterion of ``tests/test_mcc_head.py``) and against the modules in eval mode.  12 tasks (the output layer rides in ``k_predict_tail``)
and 65 (the contraction kernels' rows), 64 QM9-shaped and 8 ZINC-shaped molecules.

Bars: those ``tests/test_predict_head_gpu.py`` / ``tests/test_spectral_predict_gpu.py`` hold — per tensor ``err = max|got - ref64| /
max|ref64|`` within ``min(MARGIN max(e32, 2**-23), cap)``, ``MARGIN = 4``, ``e32`` the float32 restatement's own error, the caps
``head_harness.CAP``.  Every comparison prints one ``PREDBAR`` line before it is judged."""
import pytest
import torch

import head_harness as hh
from chemprop_amd import _lib
from conftest import parity_err_unfloored
from test_mcc_head import mcc_criterion

F = torch.nn.functional
pytestmark = pytest.mark.gpu
MARGIN = 4.0   # (tests/test_predict_head_gpu.py)
D_H, HIDDEN = 16, 12


def _model(t, dev, mcc=True):
    from chemprop_amd import agg as cagg
    from chemprop_amd import model as cm
    from chemprop_amd.nn import BondMessagePassing

    torch.manual_seed(11)
    mp = BondMessagePassing(d_h=D_H, depth=2)
    tw = 0.5 + torch.rand(t, generator=torch.Generator().manual_seed(2))
    pred = cm.BinaryClassificationFFN(n_tasks=t, input_dim=D_H, hidden_dim=HIDDEN, activation="tanh", criterion=(cm.BinaryMCC if mcc else cm.BCE)(tw))
    model = cm.MPNN(mp, cagg.MeanAggregation(), pred, batch_norm=True).to(dev).eval()
    with torch.no_grad():
        model.bn.weight.uniform_(0.5, 1.5), model.bn.bias.uniform_(-0.5, 0.5)
        model.bn.running_mean.uniform_(-0.1, 0.1), model.bn.running_var.uniform_(0.5, 2.0)
    return model


def _restate(model, Hv, batch, n, T, w, dtype):
    f = lambda x: x.detach().cpu().to(dtype)
    b = batch.cpu()
    H = torch.zeros(n, D_H, dtype=dtype).index_add(0, b, f(Hv))
    H = H / torch.bincount(b, minlength=n).clamp(min=1).to(dtype).view(-1, 1)
    bn = model.bn
    Z = F.batch_norm(H, f(bn.running_mean), f(bn.running_var), f(bn.weight), f(bn.bias), training=False, eps=bn.eps)
    for l, blk in enumerate(model.predictor.ffn):
        Z = F.linear(torch.tanh(Z) if l else Z, f(blk[-1].weight), f(blk[-1].bias))
    tw = f(model.predictor.criterion.task_weights).reshape(-1)
    return dict(raw=Z, preds=torch.sigmoid(Z), loss=mcc_criterion(Z, T.to(dtype), w.to(dtype), tw))


def _judge(cid, name, got, ref64, ref32, fails):
    g, r = got.double().reshape(-1).cpu(), ref64.double().reshape(-1)
    e32 = parity_err_unfloored(ref32.double().reshape(-1).numpy(), r.numpy())
    err = parity_err_unfloored(g.numpy(), r.numpy())
    bar = min(MARGIN * max(e32, hh.EPS32), hh.cap_of(name))
    print(f"PREDBAR {cid} {name} err={err:.3e} e32={e32:.3e} ratio={err / max(e32, hh.EPS32):.2f} bar={bar:.3e} maxref={float(r.abs().max()):.3e}")
    if not (bool(torch.isfinite(g).all()) and err <= bar):
        fails.append(f"{name}: err {err:.3e} > bar {bar:.3e}")


CASES = [(12, 64, "qm9"), (12, 8, "zinc"), (65, 64, "qm9"), (1, 64, "qm9")]


@pytest.mark.parametrize("t,n,kind", CASES, ids=[f"t{t}-{k}x{n}" for t, n, k in CASES])
def test_fused_predict_on_a_binary_mcc_model(t, n, kind, gpu_device):
    from chemprop_amd import synth
    from chemprop_amd.predict import fused_predict, predict_spec

    dev = gpu_device
    model = _model(t, dev)
    spec = predict_spec(model)
    assert spec is not None and spec.transform == "sigmoid" and spec.kind == "mcc"
    bmg = synth.random_batch(n, kind, seed=21)
    bmg.to(dev)
    g = torch.Generator().manual_seed(5)
    T = (torch.rand(n, t, generator=g) < 0.3).float()
    T[torch.rand(n, t, generator=g) < 0.2] = float("nan")
    w = 0.5 + torch.rand(n, generator=torch.Generator().manual_seed(3))
    state = {k: v.clone() for k, v in model.state_dict().items()}
    lib = _lib.load()
    with torch.no_grad():
        Hv = model.message_passing(bmg, None)
        model.message_passing.forward = lambda *a, **k: Hv   # (every path reads THIS output: the block is not part of the comparison)
        try:
            first = fused_predict(model, bmg, targets=T.to(dev), weights=w.to(dev))
            res = fused_predict(model, bmg, targets=T.to(dev), weights=w.to(dev))   # (the split images are ready now)
            n_loss = int(lib.dmpnn_last_launch_count())
            plain = fused_predict(model, bmg)
            n_plain = int(lib.dmpnn_last_launch_count())
            via_predict = model.predict(bmg)
            mod = model(bmg)
        finally:
            del model.message_passing.forward
    assert first is not None and res is not None and plain is not None
    torch.cuda.synchronize()
    assert tuple(res.preds.shape) == (n, t) == tuple(mod.shape)
    assert torch.equal(via_predict, plain.preds) and torch.equal(plain.preds, res.preds) and torch.equal(first.preds, res.preds)
    assert torch.equal(plain.raw, res.raw) and plain.loss is None and torch.equal(first.loss, res.loss)
    for k, v in model.state_dict().items():
        assert torch.equal(v, state[k]), k
    r64 = _restate(model, Hv, bmg.batch, n, T, w, torch.float64)
    r32 = _restate(model, Hv, bmg.batch, n, T, w, torch.float32)
    cid, fails = f"t{t}-{kind}x{n}", []
    _judge(cid, "raw", res.raw, r64["raw"], r32["raw"], fails)
    _judge(cid, "preds", res.preds, r64["preds"], r32["preds"], fails)
    _judge(cid, "loss", res.loss[0], r64["loss"], r32["loss"], fails)
    _judge(cid + "/module", "preds", mod, r64["preds"], r32["preds"], fails)
    assert not fails, (cid, fails)
    assert float(res.loss[1]) == float(T.isfinite().sum())
    # the modules in eval mode: the criterion module on the module's own logits
    with torch.no_grad():
        logits = torch.logit(mod.double().cpu())
    same = float(model.predictor.criterion.double().cpu()(logits, T.double(), weights=w.double()))
    model.predictor.criterion.float().to(dev)
    assert abs(float(res.loss[0]) - same) <= hh.CAP["loss"] * max(1.0, abs(same))
    # launches: the BCE model's of the same shape; with targets at most one more (the MCC stage is two launches where k_loss is one)
    bce = _model(t, dev, mcc=False)
    with torch.no_grad():
        bce.message_passing.forward = lambda *a, **k: Hv
        try:
            assert fused_predict(bce, bmg, targets=T.to(dev), weights=w.to(dev)) is not None
            fused_predict(bce, bmg, targets=T.to(dev), weights=w.to(dev))
            r_loss = int(lib.dmpnn_last_launch_count())
            fused_predict(bce, bmg)
            r_plain = int(lib.dmpnn_last_launch_count())
        finally:
            del bce.message_passing.forward
    print(f"PREDBAR {cid} launches mcc {n_plain} | {n_loss} bce {r_plain} | {r_loss}")
    assert n_plain == r_plain > 0 and n_loss == r_loss + 1


def test_a_batch_without_targets_is_val_loss_one(gpu_device):
    from chemprop_amd import synth
    from chemprop_amd.predict import fused_predict

    model = _model(12, gpu_device)
    bmg = synth.random_batch(8, "qm9", seed=21)
    bmg.to(gpu_device)
    with torch.no_grad():
        res = fused_predict(model, bmg, targets=torch.full((8, 12), float("nan"), device=gpu_device))
    assert float(res.loss[0]) == 1.0 and float(res.loss[1]) == 0.0 and bool(torch.isfinite(res.preds).all())
