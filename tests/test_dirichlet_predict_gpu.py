"""``MPNN.predict`` / ``fused_predict`` on an eval-mode model with a Dirichlet classification head: ``DMPNN_PT_DIRICHLET_BINARY`` and
``DMPNN_PT_DIRICHLET_MULTICLASS`` in ``k_predict_tail`` — both builds (``n_out <= DMPNN_PREDICT_MAX_OUT``: the output layer rides in
the tail; beyond it the rows come from the contraction kernels), one task and several, a task wider than a wave, the output layer
rescaled so that the raw outputs have a standard deviation of 1 and of 25 (``softplus`` on its linear branch beyond 20, ``2 / S``
small), and one model each with ``X_d``, attentive aggregation and two components — against the float64 restatement behind the block's
own output: aggregation, eval-mode batch norm, the MLP, ``alpha = softplus + 1``, the predictions, and the loss by
``tests/test_dirichlet_head.closed_form``.

Bars: those ``tests/test_predict_head_gpu.py`` holds — per tensor ``err = max|got - ref64| / max|ref64|`` within ``min(MARGIN max(e32,
2**-23), cap)``, ``e32`` the float32 restatement's own error, the caps ``head_harness.CAP``.  The binary head's two columns are judged
apart, each against its own ``max|ref64|``: the uncertainty ``2 / S`` must not hide behind probabilities near 1.  Every comparison
prints one ``PREDBAR`` line before it is judged.

MARGIN, measured on the MI355X against the float64 restatement over the 24 model cases of this module (120 tensor comparisons; every
line in ``profiles/dirichlet_predict_bars.txt``), starting from the 4.0 ``tests/test_predict_head_gpu.py`` holds: the worst ``err /
max(e32, 2**-23)`` is 4.71 — the loss of ``binary-K2-t3-std25`` (err 5.6e-7 on a loss of 1.375, where the float32 restatement drew
4.6e-8, below the floor: ``k_loss``'s single workgroup sums 51 terms as a tree, torch sequentially; the criterion kernel is the training
step's, unchanged, and ``tests/test_dirichlet_head_gpu.py`` measured 3.59 for the same tensor at the same range of evidence).  Then 3.13
(the MODULE path's uncertainty column of the same case: torch's own ops), 2.89 and 2.49 (loss and predictions of ``multiclass-K65-t1-std1``);
the new transforms' own worst is that 2.49, the binary columns' 1.92 (``2 / S``) and 1.36 (``p``), the raw outputs' 1.42.
2 x 4.71 = 9.4 -> MARGIN = 16: above 4 because of the loss alone; the caps (1e-5 for the loss, 2e-5 for the predictions) stay."""
import pytest
import torch

import head_harness as hh
from chemprop_amd import _lib
from conftest import parity_err_unfloored
from test_dirichlet_head import closed_form

F = torch.nn.functional
pytestmark = pytest.mark.gpu
MARGIN = 16.0   # (the module docstring: measured 4.71, doubled, rounded up to a power of two)
N_MOLS, D_H, HIDDEN, D_XD = 17, 16, 12, 8
SCALES = (1.0, 25.0)   # (tests/test_dirichlet_head_gpu.py: alpha near 1 and softplus's linear branch)


def _model(nc, t, variant, dev, dirichlet=True, binary=False):
    """The tiny model of ``tests/test_spectral_predict_gpu.py`` with a Dirichlet head (``binary``: ``BinaryDirichletFFN``, ``nc == 2``)
    — or, ``dirichlet=False``, the ``MulticlassClassificationFFN`` + cross-entropy model of the same shape."""
    from chemprop_amd import agg as cagg
    from chemprop_amd import model as cm
    from chemprop_amd.nn import BondMessagePassing, MulticomponentMessagePassing

    torch.manual_seed(11)
    n_comp = 2 if variant == "two-component" else 1
    blocks = [BondMessagePassing(d_h=D_H, depth=2) for _ in range(n_comp)]
    mp = MulticomponentMessagePassing(blocks, n_comp) if n_comp > 1 else blocks[0]
    tw = 0.5 + torch.rand(t, generator=torch.Generator().manual_seed(2))
    kw = dict(n_tasks=t, input_dim=n_comp * D_H + (D_XD if variant == "xd" else 0), hidden_dim=HIDDEN, activation="tanh")
    if not dirichlet:
        pred = cm.MulticlassClassificationFFN(nc, criterion=cm.CE(tw), **kw)
    elif binary:
        pred = cm.BinaryDirichletFFN(criterion=cm.Dirichlet(tw, v_kl=0.35), **kw)
    else:
        pred = cm.MulticlassDirichletFFN(nc, criterion=cm.Dirichlet(tw, v_kl=0.35), **kw)
    ag = cagg.AttentiveAggregation(output_size=D_H) if variant == "attentive" else cagg.MeanAggregation()
    model = (cm.MulticomponentMPNN if n_comp > 1 else cm.MPNN)(mp, ag, pred, batch_norm=True).to(dev).eval()
    with torch.no_grad():
        model.bn.weight.uniform_(0.5, 1.5), model.bn.bias.uniform_(-0.5, 0.5)
        model.bn.running_mean.uniform_(-0.1, 0.1), model.bn.running_var.uniform_(0.5, 2.0)
    return model


def _restate(model, Hvs, batches, X_d, T, w, nc, binary, dtype):
    """Everything behind the block(s) on the CPU in ``dtype``, op by op."""
    from chemprop_amd.ffn import mlp_blocks

    f = lambda x: x.detach().cpu().to(dtype)
    aggs = []
    for Hv, b in zip(Hvs, batches):
        H, b = f(Hv), b.cpu()
        if hasattr(model.agg, "W"):   # (AttentiveAggregation: exp(W h) over the molecule's sum of them, as the reference writes it)
            a = F.linear(H, f(model.agg.W.weight), f(model.agg.W.bias)).exp()
            H = H * (a / torch.zeros(N_MOLS, 1, dtype=dtype).index_add(0, b, a)[b])
            aggs.append(torch.zeros(N_MOLS, D_H, dtype=dtype).index_add(0, b, H))
        else:
            S = torch.zeros(N_MOLS, D_H, dtype=dtype).index_add(0, b, H)
            aggs.append(S / torch.bincount(b, minlength=N_MOLS).clamp(min=1).to(dtype).view(-1, 1))
    bn = model.bn
    Z = F.batch_norm(torch.cat(aggs, 1), f(bn.running_mean), f(bn.running_var), f(bn.weight), f(bn.bias), training=False, eps=bn.eps)
    if X_d is not None:
        Z = torch.cat((Z, f(X_d)), 1)
    for l, blk in enumerate(mlp_blocks(model.predictor.ffn)):
        Z = F.linear(torch.tanh(Z) if l else Z, f(blk[-1].weight), f(blk[-1].bias))
    alpha = (F.softplus(Z) + 1).reshape(N_MOLS, -1, nc)
    S = alpha.sum(-1, keepdim=True)
    preds = torch.stack((alpha[..., 1] / S[..., 0], 2 / S[..., 0]), 2) if binary else alpha / S
    crit = model.predictor.criterion
    loss = closed_form(alpha, T.to(dtype), w.to(dtype), f(crit.task_weights).reshape(-1), crit.v_kl)
    return dict(raw=Z, preds=preds, loss=loss)


def _judge(cid, name, got, ref64, ref32, fails):
    g, r = got.double().reshape(-1).cpu(), ref64.double().reshape(-1)
    e32 = parity_err_unfloored(ref32.double().reshape(-1).numpy(), r.numpy())
    err = parity_err_unfloored(g.numpy(), r.numpy())
    bar = min(MARGIN * max(e32, hh.EPS32), hh.CAP["loss" if name == "loss" else "preds"])
    print(f"PREDBAR {cid} {name} err={err:.3e} e32={e32:.3e} ratio={err / max(e32, hh.EPS32):.2f} bar={bar:.3e} maxref={float(r.abs().max()):.3e}")
    if not (bool(torch.isfinite(g).all()) and err <= bar):
        fails.append(f"{name}: err {err:.3e} > bar {bar:.3e}")


def _judge_preds(cid, tag, got, r64, r32, binary, fails):
    if not binary:
        return _judge(cid, "preds" + tag, got, r64, r32, fails)
    _judge(cid, "preds.p" + tag, got[..., 0], r64[..., 0], r32[..., 0], fails)   # (each column against its own max|ref|)
    _judge(cid, "preds.u" + tag, got[..., 1], r64[..., 1], r32[..., 1], fails)


# (head, classes, tasks, variant): n_out = 64 is the last width of the build whose output layer rides in the tail, 65 / 66 the first of the
# build that reads the contraction kernels' rows; (65, 1): one task wider than a wave
SHAPES = [("binary", 2, 1, None), ("binary", 2, 3, None), ("binary", 2, 32, None), ("binary", 2, 33, None),
          ("multiclass", 2, 1, None), ("multiclass", 3, 2, None), ("multiclass", 4, 16, None), ("multiclass", 5, 13, None), ("multiclass", 65, 1, None),
          ("binary", 2, 3, "xd"), ("multiclass", 3, 2, "attentive"), ("binary", 2, 3, "two-component")]
CASES = [s + (scale,) for s in SHAPES for scale in SCALES]


def _id(c):
    return f"{c[0]}-K{c[1]}-t{c[2]}{'-' + c[3] if c[3] else ''}-std{c[4]:g}"


@pytest.mark.parametrize("head,nc,t,variant,scale", CASES, ids=[_id(c) for c in CASES])
def test_fused_predict_on_a_dirichlet_model(head, nc, t, variant, scale, gpu_device):
    from chemprop_amd import synth
    from chemprop_amd.ffn import mlp_blocks
    from chemprop_amd.model import masked_loss
    from chemprop_amd.predict import fused_predict, predict_spec

    dev = gpu_device
    binary, n_out = head == "binary", nc * t
    model = _model(nc, t, variant, dev, binary=binary)
    multi = variant == "two-component"
    bmgs = [synth.random_batch(N_MOLS, "qm9", seed=21 + c) for c in range(2 if multi else 1)]
    for b in bmgs:
        b.to(dev)
    bmg = bmgs if multi else bmgs[0]
    batches = [b.batch for b in bmgs]
    gen = torch.Generator().manual_seed(100 * nc + t)
    X_d = torch.randn(N_MOLS, D_XD, generator=gen).to(dev) if variant == "xd" else None
    T = torch.randint(0, nc, (N_MOLS, t), generator=gen).float()   # (class indices with missing entries: test_dirichlet_head._criterion_inputs)
    T[torch.rand(N_MOLS, t, generator=gen) < 0.2] = float("nan")
    w = 0.5 + torch.rand(N_MOLS, generator=gen)
    lib = _lib.load()
    with torch.no_grad():
        out = model.message_passing(bmg, None)
        Hvs = list(out) if multi else [out]
        # the output layer times scale / std(raw): the raw outputs then have the standard deviation `scale`
        last = mlp_blocks(model.predictor.ffn)[-1][-1]
        s = scale / float(_restate(model, Hvs, batches, X_d, T, w, nc, binary, torch.float64)["raw"].std())
        last.weight.mul_(s), last.bias.mul_(s)
        state = {k: v.clone() for k, v in model.state_dict().items()}
        assert predict_spec(model) is None   # (the default keeps refusing; fused_predict asks with dirichlet=True)
        model.message_passing.forward = lambda *a, **k: out   # (every path reads THIS output: the block is not part of the comparison)
        try:
            first = fused_predict(model, bmg, X_d=X_d, targets=T.to(dev), weights=w.to(dev))
            res = fused_predict(model, bmg, X_d=X_d, targets=T.to(dev), weights=w.to(dev))   # (the split images are ready now)
            n_loss = int(lib.dmpnn_last_launch_count())
            plain = fused_predict(model, bmg, X_d=X_d)
            n_plain = int(lib.dmpnn_last_launch_count())
            via_predict = model.predict(bmg, None, X_d)
            mod = model(bmg, None, X_d)
        finally:
            del model.message_passing.forward
    assert first is not None and res is not None and plain is not None   # (no longer None for such a model)
    torch.cuda.synchronize()
    spec = predict_spec(model, dirichlet=True)
    assert spec.transform == f"dirichlet_{head}" and (spec.n_tasks, spec.n_classes, spec.n_out) == (t, nc, n_out)
    assert (n_out <= _lib.PREDICT_MAX_OUT) == (n_out <= 64)
    assert tuple(res.preds.shape) == (N_MOLS, t, nc) == tuple(mod.shape) and tuple(res.raw.shape) == (N_MOLS, n_out)
    assert torch.equal(via_predict, plain.preds) and torch.equal(plain.preds, res.preds) and torch.equal(first.preds, res.preds)
    assert torch.equal(plain.raw, res.raw) and torch.equal(first.raw, res.raw) and torch.equal(first.loss, res.loss) and plain.loss is None
    for k, v in model.state_dict().items():
        assert torch.equal(v, state[k]), k
    r64 = _restate(model, Hvs, batches, X_d, T, w, nc, binary, torch.float64)
    r32 = _restate(model, Hvs, batches, X_d, T, w, nc, binary, torch.float32)
    assert bool(torch.isfinite(r64["loss"])) and abs(float(r64["raw"].std()) - scale) <= 1e-3 * scale
    cid, fails = _id((head, nc, t, variant, scale)), []
    _judge(cid, "raw", res.raw, r64["raw"], r32["raw"], fails)       # (what train_step's input was: the MLP's own output)
    _judge_preds(cid, "", res.preds, r64["preds"], r32["preds"], binary, fails)
    _judge(cid, "loss", res.loss[0], r64["loss"], r32["loss"], fails)
    _judge_preds(cid, "/module", mod, r64["preds"], r32["preds"], binary, fails)
    assert not fails, (cid, fails)
    assert float(res.loss[1]) == float(T.isfinite().sum())
    P = res.preds.double().cpu()
    if binary:
        assert bool(((P[..., 0] > 0) & (P[..., 0] < 1)).all()) and bool(((P[..., 1] > 0) & (P[..., 1] <= 1)).all())
    else:
        assert float((P.sum(-1) - 1).abs().max()) <= nc * hh.EPS32
    # the training criterion's value on the same raw outputs
    crit = model.predictor.criterion
    alpha = (F.softplus(res.raw.double().cpu()) + 1).reshape(N_MOLS, t, nc)
    same = float(masked_loss(alpha, T.double(), w.double(), crit.task_weights.reshape(-1).double().cpu(), kind="dirichlet", v_kl=crit.v_kl))
    assert abs(float(res.loss[0]) - same) <= hh.CAP["loss"] * abs(same)
    # launches: the multiclass + cross-entropy model's of the same shape, with and without targets (k_loss is one launch for both)
    ce = _model(nc, t, variant, dev, dirichlet=False)
    with torch.no_grad():
        ce.message_passing.forward = lambda *a, **k: out
        try:
            assert fused_predict(ce, bmg, X_d=X_d, targets=T.to(dev), weights=w.to(dev)) is not None
            fused_predict(ce, bmg, X_d=X_d, targets=T.to(dev), weights=w.to(dev))
            c_loss = int(lib.dmpnn_last_launch_count())
            fused_predict(ce, bmg, X_d=X_d)
            c_plain = int(lib.dmpnn_last_launch_count())
        finally:
            del ce.message_passing.forward
    print(f"PREDBAR {cid} launches dirichlet {n_plain} | {n_loss} cross entropy {c_plain} | {c_loss}")
    assert n_plain == c_plain > 0 and n_loss == c_loss > n_plain


def test_the_two_transforms_through_the_abi(gpu_device):
    """``dmpnn_predict_head`` itself on ``B = 4``, ``d = 8``, ``n_out = 6``: both transforms' row sums and ranges; a binary call with three
    classes, and either transform with ``out_mean`` / ``out_scale``: a code, not a crash."""
    import ctypes as C

    from chemprop_amd import engine

    dev = gpu_device
    lib = _lib.load()
    B, d, n_out = 4, 8, 6
    gen = torch.Generator().manual_seed(7)
    Hv, batch = torch.randn(B, d, generator=gen).to(dev), torch.arange(B, device=dev)
    W, b = (3 * torch.randn(n_out, d, generator=gen)).to(dev), torch.randn(n_out, generator=gen).to(dev)
    raw, preds = torch.empty(B, n_out, device=dev), torch.empty(B, n_out, device=dev)
    ones = torch.ones(n_out, device=dev)

    def call(transform, nc, scale=False):
        p = _lib.PredictArgs()
        h = p.head
        h.n_atoms, h.n_mols, h.d_h, h.batch, h.agg_mode, h.agg_norm = B, B, d, batch.data_ptr(), 0, 1.0
        h.n_layers, h.dims[0], h.dims[1] = 1, d, n_out
        h.W[0], h.b[0], h.preds, h.n_classes = W.data_ptr(), b.data_ptr(), raw.data_ptr(), nc
        p.transform, p.preds = transform, preds.data_ptr()
        if scale:
            p.out_mean, p.out_scale = ones.data_ptr(), ones.data_ptr()
        nb = int(lib.dmpnn_predict_head_ws_bytes(C.byref(p)))
        ws = torch.empty(max(nb, 16), dtype=torch.uint8, device=dev)
        h.ws, h.ws_bytes = ws.data_ptr(), nb
        rc = lib.dmpnn_predict_head(C.byref(p), Hv.data_ptr(), Hv.stride(0), engine._stream_ptr(dev))
        torch.cuda.synchronize()
        return rc

    x = F.linear(Hv.double(), W.double(), b.double()).cpu()
    assert call(_lib.PT_DIRICHLET_BINARY, 2) == 0
    alpha = (F.softplus(x) + 1).reshape(B, 3, 2)
    P, S = preds.double().cpu().reshape(B, 3, 2), alpha.sum(-1)
    assert bool(((P[..., 0] > 0) & (P[..., 0] < 1)).all()) and bool(((P[..., 1] > 0) & (P[..., 1] <= 1)).all())
    assert float((P - torch.stack((alpha[..., 1] / S, 2 / S), 2)).abs().max()) <= hh.CAP["preds"]
    assert call(_lib.PT_DIRICHLET_MULTICLASS, 3) == 0
    alpha = (F.softplus(x) + 1).reshape(B, 2, 3)
    P = preds.double().cpu().reshape(B, 2, 3)
    assert float((P.sum(-1) - 1).abs().max()) <= 3 * hh.EPS32 and bool(((P > 0) & (P < 1)).all())
    assert float((P - alpha / alpha.sum(-1, keepdim=True)).abs().max()) <= hh.CAP["preds"]
    assert call(_lib.PT_DIRICHLET_BINARY, 3) != 0
    assert call(_lib.PT_DIRICHLET_BINARY, 2, scale=True) != 0 and call(_lib.PT_DIRICHLET_MULTICLASS, 3, scale=True) != 0
