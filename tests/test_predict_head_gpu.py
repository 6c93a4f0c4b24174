"""The inference head on the device: ``dmpnn_predict_head`` through the C ABI against float64, and ``fused_predict`` /
``MPNN.predict`` against the same restatement on the block's own output.

**Bar.**  Per tensor ``err = max|got - ref64| / max|ref64|`` within ``min(MARGIN * max(e32, 2**-23), cap)``: ``e32`` is the float32
restatement's own error against float64 (``predict_harness.predict_ref``), the caps are ``head_harness.CAP`` (2e-5 for ``raw`` /
``preds`` / ``fingerprint``, 1e-5 for the loss).  ``MARGIN`` is one number for the module, set by the rule of
``tests/test_head_boundaries.py``: twice the worst ``err / max(e32, 2**-23)`` of the first complete run, rounded up to a power of two.

The first complete run on the MI355X (383 comparisons): the worst three ratios were 1.81 (``xd200-bn`` preds: err 2.16e-7 against
e32 1.04e-7), 1.80 (``xd200-bn`` raw) and 1.76 (``d320`` raw: err 7.30e-7 against e32 4.15e-7) — wide reductions, where the f16
pipe's three-product split and fp32 accumulation order differ most from torch's; every model-level ratio was at most 1.03.
2 x 1.81 = 3.62 -> MARGIN = 4, below the head module's 32 (no gradients here: nothing divides by a small count or cancels).

Every comparison prints one ``PREDBAR`` line before it is judged.
"""
import ctypes as C
import dataclasses

import pytest
import torch

import predict_harness as ph
from chemprop_amd import _lib

pytestmark = pytest.mark.gpu

MARGIN = 4.0

PC = ph.PredictCase
MSE3 = dict(tasks=3, kind="mse")


def _build_cases():
    cs = []
    add = lambda id, **kw: cs.append(PC(id=id, **kw))
    # rows: the tail's 4-row workgroups, k_rows16's row tiles, kFuseAggMols and kRowsMaxB; every layout of the batch vector
    for B in (1, 3, 4, 5, 15, 16, 17, 512, 513, 1024, 1025):
        add(f"B{B}", B=B)
    add("ragged", B=17, layout="ragged")
    add("one-each", B=16, layout="one-each")
    add("huge", B=513, layout="huge", agg="norm")
    for d in (4, 6, 300, 320, 324):          # 6: the chain's kernels; 324: beyond kRowsMaxWidth
        add(f"d{d}", d_h=d)
    for N in (2, 5, 16, 17, 320, 322):
        add(f"N{N}", hidden=(N,))
    add("N5x5", hidden=(5, 5))               # (an odd reduction width: the fp32 contraction, a zero-sized slot)
    for n in (1, 4, 5, 63, 64, 65, 130):     # the tail's output layer up to 64, the contraction kernels beyond
        add(f"out{n}", transform="none", n_out=n, unscale=False)
    add("out130-unscale", transform="unscale", tasks=130)
    for hidden in ((), (8, 8), (8,) * 7):
        add(f"layers{len(hidden) + 1}", hidden=hidden)
    add("layers1-xd", hidden=(), d_xd=3, tasks=3)
    for act in ("none", "leakyrelu", "tanh", "elu"):
        add(f"act-{act}", act=act, hidden=(16, 8))
    for agg in ("sum", "norm", "attentive"):
        add(f"agg-{agg}", agg=agg, B=17)
    add("agg-attentive-loss", agg="attentive", B=17, **MSE3)
    add("comp2", n_components=2, B=17)
    add("comp2-chain", n_components=2, B=5, d_h=6)
    for d_xd in (1, 3, 200):
        for bn in (True, False):
            add(f"xd{d_xd}-{'bn' if bn else 'nobn'}", d_xd=d_xd, bn=bn, B=17)
    add("nobn", bn=False)
    for tr in ("none", "unscale", "sigmoid", "mve", "evidential", "quantile"):
        for t in (1, 3):
            for un in (True, False):
                add(f"{tr}-t{t}-{'s' if un else 'id'}", transform=tr, tasks=t, unscale=un, B=17)
    for nc in (2, 3, 7):
        for t in (1, 3):
            add(f"softmax-nc{nc}-t{t}", transform="softmax", nc=nc, tasks=t, unscale=False, B=17)
    add("softmax-nc3-t3-s", transform="softmax", nc=3, tasks=3, B=17)
    # with targets: every criterion that matches the transform; missing targets, sample and task weights, bounds on MSE
    for kind, tr in (("mse", "unscale"), ("mae", "unscale"), ("mse", "none"), ("bce", "sigmoid"), ("mve", "mve"),
                     ("evidential", "evidential"), ("quantile", "quantile")):
        for t in (1, 3):
            add(f"loss-{kind}-{tr}-t{t}", transform=tr, tasks=t, kind=kind, B=17, unscale=tr != "none")
    add("loss-ce-nc3-t3", transform="softmax", nc=3, tasks=3, kind="ce", unscale=False, B=17)
    add("loss-ce-nc2-t1", transform="softmax", nc=2, tasks=1, kind="ce", unscale=False, B=5)
    add("loss-mse-bounded", bounded=True, B=17, **MSE3)
    add("loss-mse-full", missing="none", B=513, **MSE3)
    add("loss-mse-B1025", B=1025, **MSE3)
    return cs


CASES = _build_cases()
_BY_ID = {c.id: c for c in CASES}
assert len(_BY_ID) == len(CASES)


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.id)
def test_predict_head_matches_float64_within_the_float32_yardstick(case, gpu_device):
    """One case of the sweep: the outputs against float64 within the bar; nothing but the outputs written (guard rows, the
    fingerprint's pad columns, the running statistics and ``num_batches_tracked`` bit for bit); a second call and a call on the ready
    split bit-identical to the first; three launches (four with targets) for the usual model."""
    inp = ph.build_inputs(case)
    ref, e32 = ph.yardstick(case, inp)
    call = ph.Call(case, inp, gpu_device)
    first = call.run(0)
    assert call.untouched() == []
    fails = ph.compare(case, first, ref, e32, MARGIN)
    if case.kind is not None:
        assert first["n_finite"] == ref["n_finite"]
    assert not fails, (case.id, fails)
    again = call.run(0)
    assert ph.same_bits(first, again) == [], "a second call differs"
    ready = call.run(1)
    assert ph.same_bits(first, ready) == [], "a call on the ready split differs"
    assert call.untouched() == []
    if case.usual:
        assert call.launches == 3 + (case.kind is not None), (case.id, call.launches)


@pytest.mark.parametrize("cid", ["B17", "layers3", "N5x5"])
def test_without_a_split_cache_the_hidden_layers_run_in_fp32(cid, gpu_device):
    """``wsplit == NULL``: no cache, every hidden layer on the fp32 contraction — the same bar."""
    case = _BY_ID[cid]
    inp = ph.build_inputs(case)
    ref, e32 = ph.yardstick(case, inp)
    got = ph.Call(case, inp, gpu_device, wsplit=False).run(0)
    assert not ph.compare(case, got, ref, e32, MARGIN, tag="/fp32")


@pytest.mark.parametrize("cid", ["B17", "layers3", "xd3-bn"])
def test_a_changed_hidden_weight_is_followed_when_the_split_is_not_ready(cid, gpu_device):
    """After an in-place change of a hidden weight a call with ``wsplit_ready = 0`` gives, bit for bit, what a fresh call on the new
    weight gives — and not what the old weight gave."""
    case = _BY_ID[cid]
    inp = ph.build_inputs(case)
    call = ph.Call(case, inp, gpu_device)
    old = call.run(0)
    W0 = inp["W0"] * 1.5 + 0.01
    call.keep["W0"].copy_(W0.to(gpu_device))
    new = call.run(0)
    fresh = ph.Call(case, dict(inp, W0=W0), gpu_device).run(0)
    assert ph.same_bits(new, fresh) == []
    assert "raw" in ph.same_bits(new, old)
    ref, e32 = ph.yardstick(case, dict(inp, W0=W0))
    assert not ph.compare(case, new, ref, e32, MARGIN, tag="/newW")


@pytest.mark.parametrize("cid", ["B17", "d6", "B1025", "comp2"])
def test_an_unsorted_batch_vector_gives_what_dmpnn_head_gives(cid, gpu_device):
    """A batch vector that is not non-decreasing: exactly the raw outputs of ``dmpnn_head`` (forward only) on it — NaN rows, never a
    number."""
    from chemprop_amd import engine

    case = _BY_ID[cid]
    inp = ph.build_inputs(case)
    b = inp["batch"].clone()
    b[0], b[-1] = b[-1].item(), b[0].item()
    assert bool((b[1:] < b[:-1]).any())
    call = ph.Call(case, dict(inp, batch=b), gpu_device)
    got = call.run(0)
    h = _lib.HeadArgs.from_buffer_copy(call.p.head)
    raw = torch.full((case.B, case.width), 7.0, device=gpu_device)
    h.preds = raw.data_ptr()
    nb = int(call.lib.dmpnn_head_ws_bytes(C.byref(h)))
    ws = torch.empty(nb, dtype=torch.uint8, device=gpu_device)
    h.ws, h.ws_bytes = ws.data_ptr(), nb
    Hv = call.keep["Hv"]
    _lib.check(call.lib.dmpnn_head(C.byref(h), Hv.data_ptr(), Hv.stride(0), engine._stream_ptr(gpu_device)), "dmpnn_head")
    torch.cuda.synchronize()
    assert bool(torch.isnan(raw).all()) and bool(torch.isnan(got["raw"]).all()) and bool(torch.isnan(got["preds"]).all())
    assert tuple(got["raw"].shape) == tuple(raw.shape)   # (every element NaN on both sides; a NaN's sign and payload are not part of the value)


# ---- model level: fused_predict / MPNN.predict on the mirror predictors --------------------------------------------------------------
def _model(kind, dev):
    from chemprop_amd import agg as cagg
    from chemprop_amd import model as cm
    from chemprop_amd.nn import BondMessagePassing, MulticomponentMessagePassing

    torch.manual_seed(11)
    d, d_xd, d_vd = 16, 0, None
    ffn = dict(n_tasks=3, hidden_dim=12, n_layers=1)
    ag = cagg.MeanAggregation()
    if kind == "regression-xd":
        d_xd = 5
    if kind == "binary-vd":
        d_vd = 4
    if kind == "evidential-attentive":
        ag = cagg.AttentiveAggregation(output_size=d)
    width = d + (d_vd or 0)
    if kind == "mve-multi":
        mp = MulticomponentMessagePassing([BondMessagePassing(d_h=d, depth=2), BondMessagePassing(d_h=d, depth=2)], 2)
        width = 2 * d
    else:
        mp = BondMessagePassing(d_h=d, depth=2, d_vd=d_vd)
    cls = dict(regression=cm.RegressionFFN, binary=cm.BinaryClassificationFFN, multiclass=cm.MulticlassClassificationFFN, mve=cm.MveFFN,
               evidential=cm.EvidentialFFN, quantile=cm.QuantileFFN)[kind.split("-")[0]]
    pred = cls(4, input_dim=width + d_xd, **ffn) if cls is cm.MulticlassClassificationFFN else cls(input_dim=width + d_xd, **ffn)
    model = (cm.MulticomponentMPNN if kind == "mve-multi" else cm.MPNN)(mp, ag, pred, batch_norm=True).to(dev).eval()
    with torch.no_grad():
        model.bn.weight.uniform_(0.5, 1.5), model.bn.bias.uniform_(-0.5, 0.5)
        model.bn.running_mean.uniform_(-0.1, 0.1), model.bn.running_var.uniform_(0.5, 2.0)
    return model, d_xd, d_vd


def _model_case(model, spec, n_mols, d_out, d_xd, with_loss):
    """The ``PredictCase`` and the harness inputs that restate ``model`` behind its block."""
    kind = spec.kind if with_loss else None
    hidden = tuple(int(l.out_features) for l in spec.layers[:-1])
    agg = "attentive" if spec.att is not None else {v: k for k, v in __import__("chemprop_amd.agg", fromlist=["MODES"]).MODES.items()}[spec.agg_mode]
    return PC(id="model", B=n_mols, d_h=d_out, hidden=hidden, tasks=spec.n_tasks, transform=spec.transform, nc=spec.n_classes, unscale=False,
              kind=kind, act=spec.f_act, agg=agg, bn=True, d_xd=d_xd, n_components=spec.n_components)


MODEL_KINDS = ["regression-xd", "binary-vd", "multiclass", "mve-multi", "evidential-attentive", "quantile"]


@pytest.mark.parametrize("kind", MODEL_KINDS)
def test_fused_predict_and_the_module_path_match_float64_behind_the_block(kind, gpu_device):
    """``fused_predict(...).preds`` / ``.fingerprint`` / ``.loss`` and the module path ``model(...)`` on a 17-molecule batch against
    ``predict_ref`` on the block's own ``H_v`` (taken once: the block is not part of the comparison); no parameter or buffer of the
    model changes; ``MPNN.predict`` returns ``fused_predict``'s predictions."""
    from chemprop_amd import synth
    from chemprop_amd.model import _component_batch
    from chemprop_amd.predict import fused_predict, predict_spec

    dev = gpu_device
    model, d_xd, d_vd = _model(kind, dev)
    spec = predict_spec(model)
    assert spec is not None
    n = 17
    gen = torch.Generator().manual_seed(3)
    multi = kind == "mve-multi"
    bmgs = [synth.random_batch(n, "qm9", seed=21 + c) for c in range(2 if multi else 1)]
    for b in bmgs:
        b.to(dev)
    bmg = bmgs if multi else bmgs[0]
    V_d = torch.randn(int(bmgs[0].V.shape[0]), d_vd, generator=gen).to(dev) if d_vd else None
    X_d = torch.randn(n, d_xd, generator=gen).to(dev) if d_xd else None
    T = torch.randn(n, spec.n_tasks, generator=gen)
    if spec.kind == "bce":
        T = T.gt(0).float()
    if spec.kind == "ce":
        T = torch.randint(0, spec.n_classes, (n, spec.n_tasks), generator=gen).float()
    T[torch.rand(n, spec.n_tasks, generator=gen) < 0.2] = float("nan")
    w = 0.5 + torch.rand(n, generator=gen)
    state = {k: v.clone() for k, v in model.state_dict().items()}
    with torch.no_grad():
        out = model.message_passing(bmg, V_d)
        Hv = torch.cat(list(out)) if multi else out
        # (every path below reads THIS output: a block's first and later forwards may take different routes, equal only to rounding)
        model.message_passing.forward = lambda *a, **k: out
        try:
            res = fused_predict(model, bmg, V_d, X_d, targets=T.to(dev), weights=w.to(dev), fingerprint=True)
            mod = model(bmg, V_d, X_d)
            via_predict = model.predict(bmg, V_d, X_d)
        finally:
            del model.message_passing.forward
    assert res is not None
    torch.cuda.synchronize()
    assert tuple(res.preds.shape) == tuple(mod.shape)
    assert torch.equal(via_predict, res.preds)
    for k, v in model.state_dict().items():
        assert torch.equal(v, state[k]), k
    # the restatement on the block's own H_v
    case = _model_case(model, spec, n, int(Hv.shape[1]), d_xd, True)
    inp = dict(batch=_component_batch([b.batch for b in bmgs], n).cpu(), Hv=Hv.cpu(), agg_norm=spec.agg_norm, bn_eps=model.bn.eps, bn_momentum=model.bn.momentum,
               bn_weight=model.bn.weight.detach().cpu(), bn_bias=model.bn.bias.detach().cpu(), running_mean=model.bn.running_mean.cpu(),
               running_var=model.bn.running_var.cpu(), T=T, w=w, tw=model.criterion.task_weights.reshape(-1).cpu().expand(spec.n_tasks).contiguous())
    if spec.att is not None:
        inp.update(att_W=spec.att.weight.detach().cpu(), att_b=spec.att.bias.detach().cpu())
    if X_d is not None:
        inp["X"] = X_d.cpu()
    for l, lin in enumerate(spec.layers):
        inp[f"W{l}"], inp[f"b{l}"] = lin.weight.detach().cpu(), lin.bias.detach().cpu()
    ref, e32 = ph.yardstick(case, inp)
    got = dict(fingerprint=res.fingerprint.cpu(), raw=res.raw.cpu(), preds=res.preds.cpu(), loss=res.loss[0].cpu())
    fails = ph.compare(dataclasses.replace(case, id=f"model-{kind}"), got, ref, e32, MARGIN)
    assert float(res.loss[1]) == ref["n_finite"]
    fails += ph.compare(dataclasses.replace(case, id=f"model-{kind}", kind=None), dict(preds=mod.cpu()), ref, e32, MARGIN, tag="/module")
    assert not fails, fails


def test_predict_on_a_refused_model_is_the_module_path_bit_for_bit(gpu_device):
    """A model the inference head refuses (a PReLU predictor): ``MPNN.predict`` is ``model(...)``."""
    from chemprop_amd import agg as cagg
    from chemprop_amd import synth
    from chemprop_amd.model import MPNN, RegressionFFN
    from chemprop_amd.nn import BondMessagePassing
    from chemprop_amd.predict import fused_predict

    torch.manual_seed(5)
    model = MPNN(BondMessagePassing(d_h=16, depth=2), cagg.MeanAggregation(), RegressionFFN(n_tasks=2, input_dim=16, hidden_dim=8, activation="prelu"),
                 batch_norm=True).to(gpu_device).eval()
    bmg = synth.random_batch(17, "qm9", seed=2)
    bmg.to(gpu_device)
    with torch.no_grad():
        assert fused_predict(model, bmg) is None
        assert torch.equal(model.predict(bmg), model(bmg))
