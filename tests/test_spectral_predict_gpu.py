"""``MPNN.predict`` / ``fused_predict`` on an eval-mode model with a ``SpectralFFN``: ``DMPNN_PT_SPECTRAL`` in ``k_predict_tail`` —
``t = 3`` (the build whose output layer rides in the tail, ``n_out <= DMPNN_PREDICT_MAX_OUT``) and ``t = 65``, ``t = 1801`` (the build
that reads the contraction kernels' rows: what a real spectrum takes), softplus and exp — against the float64 restatement behind the
block's own output (aggregation, eval-mode batch norm, the MLP, ``p = a / sum a``: ``tests/test_spectral_head.py``).

Bars: those ``tests/test_predict_head_gpu.py`` holds — per tensor ``err = max|got - ref64| / max|ref64|`` within ``min(MARGIN max(e32,
2**-23), cap)``, ``MARGIN = 4``, ``e32`` the float32 restatement's own error, the caps ``head_harness.CAP``.  Every comparison prints
one ``PREDBAR`` line before it is judged."""
import copy

import pytest
import torch

import head_harness as hh
from chemprop_amd import _lib
from conftest import parity_err_unfloored
from test_spectral_head import spectral_criterion, spectral_p, spectral_targets

F = torch.nn.functional
pytestmark = pytest.mark.gpu
MARGIN = 4.0   # (tests/test_predict_head_gpu.py)
N_MOLS, D_H, HIDDEN = 17, 16, 12


def _model(t, sact, crit, dev, spectral=True):
    from chemprop_amd import agg as cagg
    from chemprop_amd import model as cm
    from chemprop_amd.nn import BondMessagePassing

    torch.manual_seed(11)
    mp = BondMessagePassing(d_h=D_H, depth=2)
    tw = 0.5 + torch.rand(t, generator=torch.Generator().manual_seed(2))
    if spectral:
        pred = cm.SpectralFFN(n_tasks=t, input_dim=D_H, hidden_dim=HIDDEN, activation="tanh", spectral_activation=sact,
                              criterion=(cm.SID if crit == "sid" else cm.Wasserstein)(tw))
    else:
        pred = cm.RegressionFFN(n_tasks=t, input_dim=D_H, hidden_dim=HIDDEN, activation="tanh", criterion=cm.MSE(tw))
    model = cm.MPNN(mp, cagg.MeanAggregation(), pred, batch_norm=True).to(dev).eval()
    with torch.no_grad():
        model.bn.weight.uniform_(0.5, 1.5), model.bn.bias.uniform_(-0.5, 0.5)
        model.bn.running_mean.uniform_(-0.1, 0.1), model.bn.running_var.uniform_(0.5, 2.0)
    return model


def _restate(model, Hv, batch, T, w, sact, crit, dtype):
    from chemprop_amd.ffn import mlp_blocks

    f = lambda x: x.detach().cpu().to(dtype)
    b = batch.cpu()
    H = torch.zeros(N_MOLS, D_H, dtype=dtype).index_add(0, b, f(Hv))
    H = H / torch.bincount(b, minlength=N_MOLS).clamp(min=1).to(dtype).view(-1, 1)
    bn = model.bn
    Z = F.batch_norm(H, f(bn.running_mean), f(bn.running_var), f(bn.weight), f(bn.bias), training=False, eps=bn.eps)
    for l, blk in enumerate(mlp_blocks(model.predictor.ffn)):
        Z = F.linear(torch.tanh(Z) if l else Z, f(blk[-1].weight), f(blk[-1].bias))
    tw = f(model.predictor.criterion.task_weights).reshape(-1)
    return dict(raw=Z, preds=spectral_p(Z, sact), loss=spectral_criterion(crit, Z, T.to(dtype), w.to(dtype), tw, sact))


def _judge(cid, name, got, ref64, ref32, fails):
    g, r = got.double().reshape(-1).cpu(), ref64.double().reshape(-1)
    e32 = parity_err_unfloored(ref32.double().reshape(-1).numpy(), r.numpy())
    err = parity_err_unfloored(g.numpy(), r.numpy())
    bar = min(MARGIN * max(e32, hh.EPS32), hh.cap_of(name))
    print(f"PREDBAR {cid} {name} err={err:.3e} e32={e32:.3e} ratio={err / max(e32, hh.EPS32):.2f} bar={bar:.3e} maxref={float(r.abs().max()):.3e}")
    if not (bool(torch.isfinite(g).all()) and err <= bar):
        fails.append(f"{name}: err {err:.3e} > bar {bar:.3e}")


CASES = [(3, "softplus", "sid"), (3, "exp", "wasserstein"), (65, "softplus", "wasserstein"), (65, "exp", "sid"), (1801, "softplus", "sid"),
         (1801, "exp", "wasserstein")]


@pytest.mark.parametrize("t,sact,crit", CASES, ids=[f"t{t}-{a}-{c}" for t, a, c in CASES])
def test_fused_predict_on_a_spectral_model(t, sact, crit, gpu_device):
    from chemprop_amd import synth
    from chemprop_amd.predict import fused_predict, predict_spec

    dev = gpu_device
    assert (t <= _lib.PREDICT_MAX_OUT) == (t == 3)
    model = _model(t, sact, crit, dev)
    spec = predict_spec(model)
    assert spec is not None and spec.transform == "spectral" and spec.kind == crit
    bmg = synth.random_batch(N_MOLS, "qm9", seed=21)
    bmg.to(dev)
    T = spectral_targets(N_MOLS, t, "some", 5)
    w = 0.5 + torch.rand(N_MOLS, generator=torch.Generator().manual_seed(3))
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
    assert first is not None and res is not None and plain is not None   # (no longer None for such a model)
    torch.cuda.synchronize()
    assert tuple(res.preds.shape) == (N_MOLS, t) == tuple(mod.shape)
    assert torch.equal(via_predict, plain.preds) and torch.equal(plain.preds, res.preds) and torch.equal(first.preds, res.preds)
    assert torch.equal(plain.raw, res.raw) and plain.loss is None
    for k, v in model.state_dict().items():
        assert torch.equal(v, state[k]), k
    r64 = _restate(model, Hv, bmg.batch, T, w, sact, crit, torch.float64)
    r32 = _restate(model, Hv, bmg.batch, T, w, sact, crit, torch.float32)
    cid, fails = f"t{t}-{sact}-{crit}", []
    _judge(cid, "raw", res.raw, r64["raw"], r32["raw"], fails)       # (what train_step's input was: the MLP's own output)
    _judge(cid, "preds", res.preds, r64["preds"], r32["preds"], fails)
    _judge(cid, "loss", res.loss[0], r64["loss"], r32["loss"], fails)
    _judge(cid + "/module", "preds", mod, r64["preds"], r32["preds"], fails)
    assert not fails, (cid, fails)
    assert float(res.loss[1]) == float(T.isfinite().sum())
    assert float((res.preds.double().sum(1) - 1).abs().max()) <= t * hh.EPS32
    # the training criterion's value on the same raw outputs
    tw = model.predictor.criterion.task_weights.reshape(-1).double().cpu()
    same = float(spectral_criterion(crit, res.raw.double().cpu(), T.double(), w.double(), tw, sact))
    assert abs(float(res.loss[0]) - same) <= hh.CAP["loss"] * abs(same)
    # launches: the regression model's of the same shape; with targets at most one more (the spectral stage is two launches)
    reg = _model(t, sact, crit, dev, spectral=False)
    Tr = torch.randn(N_MOLS, t).to(dev)
    with torch.no_grad():
        reg.message_passing.forward = lambda *a, **k: Hv
        try:
            assert fused_predict(reg, bmg, targets=Tr, weights=w.to(dev)) is not None
            fused_predict(reg, bmg, targets=Tr, weights=w.to(dev))
            r_loss = int(lib.dmpnn_last_launch_count())
            fused_predict(reg, bmg)
            r_plain = int(lib.dmpnn_last_launch_count())
        finally:
            del reg.message_passing.forward
    print(f"PREDBAR {cid} launches spectral {n_plain} | {n_loss} regression {r_plain} | {r_loss}")
    assert n_plain == r_plain > 0 and r_loss <= n_loss <= r_loss + 1


def test_the_transform_refuses_a_scale_and_an_unknown_activation(gpu_device):
    """``DMPNN_PT_SPECTRAL`` with ``out_mean`` / ``out_scale``, or with a ``spectral_act`` that is neither 0 nor 1: a code, not a crash."""
    import ctypes as C

    from chemprop_amd import engine

    dev = gpu_device
    lib = _lib.load()
    B, d, t = 4, 8, 5
    Hv, batch = torch.randn(B, d, device=dev), torch.arange(B, device=dev)
    W, b, raw, preds = torch.randn(t, d, device=dev), torch.zeros(t, device=dev), torch.empty(B, t, device=dev), torch.empty(B, t, device=dev)
    ones = torch.ones(t, device=dev)

    def call(act=0, scale=False):
        p = _lib.PredictArgs()
        h = p.head
        h.n_atoms, h.n_mols, h.d_h, h.batch, h.agg_mode, h.agg_norm = B, B, d, batch.data_ptr(), 0, 1.0
        h.n_layers, h.dims[0], h.dims[1] = 1, d, t
        h.W[0], h.b[0], h.preds = W.data_ptr(), b.data_ptr(), raw.data_ptr()
        h.spectral_act = act
        p.transform, p.preds = _lib.PT_SPECTRAL, preds.data_ptr()
        if scale:
            p.out_mean, p.out_scale = ones.data_ptr(), ones.data_ptr()
        nb = int(lib.dmpnn_predict_head_ws_bytes(C.byref(p)))
        ws = torch.empty(max(nb, 16), dtype=torch.uint8, device=dev)
        h.ws, h.ws_bytes = ws.data_ptr(), nb
        rc = lib.dmpnn_predict_head(C.byref(p), Hv.data_ptr(), Hv.stride(0), engine._stream_ptr(dev))
        torch.cuda.synchronize()
        return rc

    assert call() == 0
    assert float((preds.sum(1) - 1).abs().max()) <= t * hh.EPS32
    assert call(act=2) != 0 and call(scale=True) != 0
