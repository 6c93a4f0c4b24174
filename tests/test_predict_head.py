"""The inference head without a device: the ABI of ``dmpnn_predict_head`` (exports, struct layout, every argument rule, the size
functions), the float64 restatement ``predict_harness.predict_ref`` held to the mirror predictors and to a hand-written
``UnscaleTransform``, the bar of the GPU test shown to catch three deliberate mistakes, and ``PredictSpec`` / ``fused_predict``'s
refusals."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest
import torch

import predict_harness as ph
from chemprop_amd import _lib
from conftest import parity_err_unfloored
from test_predict_head_gpu import MARGIN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = torch.nn.functional
NEW = ("dmpnn_predict_head_ws_bytes", "dmpnn_predict_head_wsplit_bytes", "dmpnn_predict_head")
EINVAL, ENOSPC = -1, -3
PT = _lib.PREDICT_TRANSFORM


def test_the_three_entry_points_are_exported():
    lib = _lib.load()
    for n in NEW:
        assert n in _lib.EXPORTS and hasattr(lib, n), n


def test_predict_args_mirror_matches_the_header(tmp_path):
    """Field order against the header; ``sizeof`` / ``offsetof`` against gcc (the method of ``tests/test_abi.py``)."""
    src = open(os.path.join(ROOT, "include", "dmpnn.h")).read()
    body = re.search(r"typedef struct dmpnn_predict_args \{(.*?)\} dmpnn_predict_args;", src, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        for part in decl.strip().split(",") if decl.strip() else []:
            fields.append(re.findall(r"([A-Za-z_0-9]+)\s*$", part.strip())[0])
    assert fields == [f[0] for f in _lib.PredictArgs._fields_]
    assert {name: PT[name] for name in PT} == dict(none=0, unscale=1, sigmoid=2, softmax=3, mve=4, evidential=5, quantile=6)
    assert re.search(r"#define DMPNN_PREDICT_MAX_OUT (\d+)", src).group(1) == str(_lib.PREDICT_MAX_OUT)
    enum = re.search(r"enum dmpnn_predict_transform \{(.*?)\}", src, re.S).group(1)
    assert [e.strip().split("=")[0].strip() for e in enum.split(",")] == ["DMPNN_PT_" + k.upper() for k in PT]
    if not shutil.which("gcc"):
        pytest.skip("no gcc")
    m = _lib.PredictArgs
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "dmpnn.h"', "int main(void) {",
             'printf("size %zu\\n", sizeof(dmpnn_predict_args));']
    lines += [f'printf("{f[0]} %zu\\n", offsetof(dmpnn_predict_args, {f[0]}));' for f in m._fields_] + ["return 0; }"]
    (tmp_path / "layout.c").write_text("\n".join(lines))
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(tmp_path / "layout.c"), "-o", str(tmp_path / "layout")], check=True)
    out = dict(l.split() for l in subprocess.run([str(tmp_path / "layout")], capture_output=True, text=True, check=True).stdout.splitlines())
    assert int(out["size"]) == C.sizeof(m)
    for f in m._fields_:
        assert int(out[f[0]]) == getattr(m, f[0]).offset, f[0]


PTR = 4096   # a non-NULL, 16-byte aligned stand-in: every check below stops before anything is dereferenced


def _valid(n_out=1, transform="unscale", n_mols=4, hidden=(8,), d_h=8):
    p = _lib.PredictArgs()
    h = p.head
    h.n_atoms, h.n_mols, h.d_h, h.batch = 10, n_mols, d_h, PTR
    dims = (d_h,) + tuple(hidden) + (n_out,)
    h.n_layers, h.act = len(dims) - 1, _lib.ACT["relu"]
    for i, v in enumerate(dims):
        h.dims[i] = v
    for l in range(len(dims) - 1):
        h.W[l] = PTR
    h.preds = PTR
    p.transform = PT[transform]
    return p


def _call(p):
    lib = _lib.load()
    rc = lib.dmpnn_predict_head(C.byref(p), PTR, p.head.d_h, None)
    return rc, lib.dmpnn_last_error_string().decode()


def _set(**kw):
    def f(p):
        for k, v in kw.items():
            obj, name = (p.head, k[5:]) if k.startswith("head_") else (p, k)
            setattr(obj, name, v)
    return f


def _gw0(p):
    p.head.gW[0] = PTR


def _gb1(p):
    p.head.gb[1] = PTR


# (rule, how the valid call is spoiled, the valid call's shape, the code, what the message names)
ERRORS = [
    ("gHv", _set(head_gHv=PTR), {}, EINVAL, "gradient"),
    ("gW", _gw0, {}, EINVAL, "gradient"),
    ("gb", _gb1, {}, EINVAL, "gradient"),
    ("g_bn_weight", _set(head_g_bn_weight=PTR), {}, EINVAL, "gradient"),
    ("g_bn_bias", _set(head_g_bn_bias=PTR), {}, EINVAL, "gradient"),
    ("g_att_W", _set(head_g_att_W=PTR), {}, EINVAL, "gradient"),
    ("g_att_b", _set(head_g_att_b=PTR), {}, EINVAL, "gradient"),
    ("bn_training", _set(head_bn_training=1), {}, EINVAL, "bn_training"),
    ("ffn_dropout_p", _set(head_ffn_dropout_p=0.25), {}, EINVAL, "ffn_dropout_p"),
    ("out_mean alone", _set(out_mean=PTR), {}, EINVAL, "out_mean and out_scale"),
    ("out_scale alone", _set(out_scale=PTR), {}, EINVAL, "out_mean and out_scale"),
    ("transform 7", _set(transform=7), {}, EINVAL, "unknown transform"),
    ("transform -1", _set(transform=-1), {}, EINVAL, "unknown transform"),
    ("softmax, one class", _set(head_n_classes=1), dict(transform="softmax", n_out=4), EINVAL, "softmax"),
    ("softmax, classes do not divide", _set(head_n_classes=3), dict(transform="softmax", n_out=4), EINVAL, "softmax"),
    ("mve, odd width", _set(), dict(transform="mve", n_out=3), EINVAL, "MVE / quantile"),
    ("quantile, odd width", _set(), dict(transform="quantile", n_out=5), EINVAL, "MVE / quantile"),
    ("evidential, width % 4", _set(), dict(transform="evidential", n_out=6), EINVAL, "evidential"),
    ("criterion against transform", _set(head_targets=PTR, head_loss_out=PTR, head_loss=_lib.LOSS["mve"]), dict(n_out=2), EINVAL, "disagree"),
    ("ce against sigmoid", _set(head_targets=PTR, head_loss_out=PTR, head_loss=_lib.LOSS["ce"], head_n_classes=2), dict(transform="sigmoid", n_out=2), EINVAL,
     "disagree"),
    ("targets without loss_out", _set(head_targets=PTR), {}, EINVAL, "loss_out"),
    ("ld_fp", _set(fingerprint=PTR, ld_fp=7), {}, EINVAL, "ld_fp"),
    ("no raw outputs", _set(head_preds=None), {}, EINVAL, "preds"),
    ("no layers", _set(head_n_layers=0), {}, EINVAL, "predictor layers"),
    ("workspace missing", _set(), {}, ENOSPC, "workspace"),
    ("workspace too small", _set(head_ws=PTR, head_ws_bytes=64), {}, ENOSPC, "workspace"),
    ("wsplit too small", _set(wsplit=PTR, wsplit_bytes=64), {}, ENOSPC, "wsplit"),
]


@pytest.mark.parametrize("rule,spoil,shape,code,names", ERRORS, ids=[e[0] for e in ERRORS])
def test_argument_errors_are_codes_before_any_device_work(rule, spoil, shape, code, names):
    """Every rule of ``dmpnn.h``: the return code, and ``dmpnn_last_error_string()`` names the rule.  The pointers are stand-ins and
    there is no device here: a check that came after device work would crash instead."""
    p = _valid(**shape)
    spoil(p)
    rc, msg = _call(p)
    assert rc == code, (rule, rc, msg)
    assert names in msg, (rule, msg)


def test_null_args_and_the_valid_call_up_to_its_workspace():
    lib = _lib.load()
    assert lib.dmpnn_predict_head(None, PTR, 8, None) == EINVAL
    assert "null args" in lib.dmpnn_last_error_string().decode()
    # the valid stand-in passes every argument rule: what stops it is the missing workspace
    for shape in ({}, dict(transform="mve", n_out=6), dict(transform="evidential", n_out=8), dict(transform="none", n_out=130)):
        rc, msg = _call(_valid(**shape))
        assert rc == ENOSPC and "workspace" in msg, (shape, rc, msg)


def test_size_functions_are_zero_for_malformed_structs_and_monotone_in_the_molecules():
    lib = _lib.load()
    ws, wsp = lib.dmpnn_predict_head_ws_bytes, lib.dmpnn_predict_head_wsplit_bytes
    assert ws(None) == 0 and wsp(None) == 0
    for spoil in (_set(head_n_layers=0), _set(head_n_layers=9), _set(head_d_h=0), _set(transform=9), _set(head_n_mols=-1), _set(head_n_components=9)):
        p = _valid()
        spoil(p)
        assert ws(C.byref(p)) == 0 and wsp(C.byref(p)) == 0
    last = 0
    for n in (0, 1, 16, 17, 512, 513, 1024, 1025, 4096):
        p = _valid(n_mols=n, hidden=(16, 8))
        b = int(ws(C.byref(p)))
        assert b >= last and b > 0
        last = b
        # the split images belong to the weights: one slot per hidden layer, whatever the batch
        assert int(wsp(C.byref(p))) == lib.dmpnn_linear16_wsplit_bytes(16, 8) + lib.dmpnn_linear16_wsplit_bytes(8, 16)
    assert int(ws(C.byref(_valid()))) == int(lib.dmpnn_head_ws_bytes(C.byref(_valid().head)))
    # an odd reduction width: that layer runs in fp32 and its slot is empty; no hidden layer: nothing to keep
    assert int(wsp(C.byref(_valid(hidden=(5, 5))))) == lib.dmpnn_linear16_wsplit_bytes(5, 8)
    assert int(wsp(C.byref(_valid(hidden=(8,), d_h=6)))) == lib.dmpnn_linear16_wsplit_bytes(8, 6)
    assert int(wsp(C.byref(_valid(hidden=(8,), d_h=5)))) == 0
    assert int(wsp(C.byref(_valid(hidden=())))) == 0


# ---- the restatement -----------------------------------------------------------------------------------------------------------------
def _mirror(name):
    from chemprop_amd import model as cm

    return dict(unscale=cm.RegressionFFN, sigmoid=cm.BinaryClassificationFFN, softmax=cm.MulticlassClassificationFFN, mve=cm.MveFFN,
                evidential=cm.EvidentialFFN, quantile=cm.QuantileFFN)[name]


@pytest.mark.parametrize("transform", ["unscale", "sigmoid", "softmax", "mve", "evidential", "quantile"])
def test_predict_ref_is_the_mirror_predictors_eval_forward(transform, monkeypatch):
    """``s = 1``, ``m = 0``: ``predict_ref`` equals ``forward`` of this package's six predictor classes, in float64, on the
    restatement's own fingerprint.  (The mirror MLP runs on the device only; it IS an ``nn.Sequential`` of torch modules, whose own
    ``forward`` stands in for it here.)"""
    from chemprop_amd.ffn import MLP

    monkeypatch.setattr(MLP, "forward", torch.nn.Sequential.forward)
    case = ph.PredictCase(id="m", B=7, d_h=8, hidden=(12,), tasks=3, transform=transform, nc=4 if transform == "softmax" else 0, unscale=False, d_xd=2)
    inp = ph.build_inputs(case)
    ref = ph.predict_ref(case, inp)
    cls = _mirror(transform)
    kw = dict(n_tasks=3, input_dim=10, hidden_dim=12, n_layers=1)
    pred = (cls(4, **kw) if transform == "softmax" else cls(**kw)).double().eval()
    with torch.no_grad():
        for l, blk in enumerate(pred.ffn):
            blk[-1].weight.copy_(inp[f"W{l}"]), blk[-1].bias.copy_(inp[f"b{l}"])
        out = pred(ref["fingerprint"])
        raw = pred.train_step(ref["fingerprint"]) if transform in ("sigmoid", "softmax") else None
    assert out.shape == ref["preds"].shape
    assert parity_err_unfloored(ref["preds"].numpy(), out.numpy()) <= 1e-14
    if raw is not None:
        assert parity_err_unfloored(ref["raw"].numpy(), raw.reshape(7, -1).numpy()) <= 1e-14


class _Unscale(torch.nn.Module):
    """``chemprop.nn.transforms.UnscaleTransform`` restated by hand: the identity while training, ``X * scale + mean`` in eval mode;
    ``transform_variance``: ``var * scale ** 2``."""

    def __init__(self, mean, scale):
        super().__init__()
        self.register_buffer("mean", mean.reshape(1, -1))
        self.register_buffer("scale", scale.reshape(1, -1))

    def forward(self, X):
        return X if self.training else X * self.scale + self.mean

    def transform_variance(self, var):
        return var if self.training else var * self.scale ** 2


def _reference_forward(name, Y, ot):
    """``forward`` of the reference's predictors (``nn/predictors.py``) on the MLP's output ``Y``, written as they are there."""
    sp = F.softplus
    if name == "unscale":
        return ot(Y)
    if name == "mve":
        mean, var = torch.chunk(Y, 2, 1)
        return torch.stack((ot(mean), ot.transform_variance(sp(var))), dim=2)
    if name == "evidential":
        mean, v, alpha, beta = torch.chunk(Y, 4, 1)
        return torch.stack((ot(mean), sp(v), sp(alpha) + 1, ot.transform_variance(sp(beta))), dim=2)
    lower, upper = torch.chunk(Y, 2, 1)
    lower, upper = ot(lower), ot(upper)
    return torch.stack(((lower + upper) / 2, upper - lower), dim=2)


@pytest.mark.parametrize("transform", ["unscale", "mve", "evidential", "quantile"])
def test_predict_ref_is_the_reference_forward_under_an_unscale_transform(transform):
    """``s, m`` away from the identity: the scale on the means, its SQUARE on MVE's variance and on the evidential beta."""
    case = ph.PredictCase(id="u", B=7, hidden=(8,), tasks=3, transform=transform)
    inp = ph.build_inputs(case)
    assert float((inp["out_scale"] - 1).abs().min()) > 1e-3
    ref = ph.predict_ref(case, inp)
    ot = _Unscale(inp["out_mean"].double(), inp["out_scale"].double()).eval()
    want = _reference_forward(transform, ref["raw"], ot)
    assert want.shape == ref["preds"].shape and parity_err_unfloored(ref["preds"].numpy(), want.numpy()) <= 1e-14
    assert torch.equal(_reference_forward(transform, ref["raw"], ot.train()), _reference_forward(transform, ref["raw"], _Unscale(torch.zeros(3), torch.ones(3)).double().eval()))


@pytest.mark.parametrize("wrong,transform,name", [("s_not_squared", "mve", "preds"), ("s_not_squared", "evidential", "preds"),
                                                 ("stacked", "mve", "preds"), ("stacked", "evidential", "preds"), ("stacked", "quantile", "preds"),
                                                 ("batch_stats", "unscale", "fingerprint"), ("batch_stats", "unscale", "preds")])
def test_the_bar_catches_a_wrong_restatement(wrong, transform, name):
    """``s`` for ``s**2``, stacked for chunked columns, batch for running statistics: each, in float64, misses the GPU test's bar on
    the CPU yardstick."""
    case = ph.PredictCase(id="w", B=17, hidden=(8,), tasks=3, transform=transform)
    inp = ph.build_inputs(case)
    ref, e32 = ph.yardstick(case, inp)
    assert all(e32[k] <= ph.CAP["preds"] for k in ("fingerprint", "raw", "preds"))   # (plain fp32 itself is inside the caps)
    bad = ph.predict_ref(case, inp, torch.float64, wrong=wrong)
    fails = ph.compare(case, {name: bad[name]}, ref, e32, MARGIN, report=lambda s: None)
    assert len(fails) == 1 and fails[0].startswith(name), fails
    assert not ph.compare(case, ph.predict_ref(case, inp, torch.float32), ref, e32, MARGIN, report=lambda s: None)


# ---- PredictSpec / fused_predict -----------------------------------------------------------------------------------------------------
def _model(cls_name="RegressionFFN", activation="relu", agg=None, **pred_kw):
    from chemprop_amd import agg as cagg
    from chemprop_amd import model as cm
    from chemprop_amd.nn import BondMessagePassing

    cls = getattr(cm, cls_name)
    kw = dict(n_tasks=3, input_dim=16, hidden_dim=8, activation=activation, **pred_kw)
    pred = cls(4, **kw) if cls_name == "MulticlassClassificationFFN" else cls(**kw)
    return cm.MPNN(BondMessagePassing(d_h=16, depth=2), agg if agg is not None else cagg.MeanAggregation(), pred, batch_norm=True)


@pytest.mark.parametrize("cls,transform", [("RegressionFFN", "unscale"), ("BinaryClassificationFFN", "sigmoid"), ("MulticlassClassificationFFN", "softmax"),
                                           ("MveFFN", "mve"), ("EvidentialFFN", "evidential"), ("QuantileFFN", "quantile")])
def test_predict_spec_tells_the_transform_from_the_predictor_class(cls, transform):
    from chemprop_amd.predict import PredictSpec

    spec = PredictSpec(_model(cls))
    assert spec.transform == transform and spec.unscale is None and spec.n_tasks == 3
    assert spec.out_shape(5) == {"softmax": (5, 3, 4), "mve": (5, 3, 2), "evidential": (5, 3, 4), "quantile": (5, 3, 2)}.get(transform, (5, 3))


def test_predict_spec_reads_and_refuses_an_unscale_transform():
    from chemprop_amd.predict import PredictSpec

    class UnscaleTransform(_Unscale):
        pass

    model = _model("MveFFN")
    model.predictor.output_transform = UnscaleTransform(torch.tensor([1.0, 2.0, 3.0]), torch.tensor([2.0, 3.0, 4.0]))
    assert PredictSpec(model).unscale is model.predictor.output_transform
    model.predictor.output_transform = UnscaleTransform(torch.tensor([1.0, 2.0]), torch.tensor([2.0, 3.0, 4.0]))   # a mean of the wrong length
    with pytest.raises(NotImplementedError, match="UnscaleTransform"):
        PredictSpec(model)


def test_predict_spec_refusals_and_the_cache():
    from chemprop_amd import model as cm
    from chemprop_amd.predict import PredictSpec, predict_spec

    with pytest.raises(NotImplementedError):
        PredictSpec(_model(activation="prelu"))

    class Custom(torch.nn.Module):
        def forward(self, H, batch):
            return H[:1]

    with pytest.raises(NotImplementedError):
        PredictSpec(_model(agg=Custom()))

    class Other(torch.nn.Module):     # a predictor of no known class
        input_dim, n_tasks, n_targets = 16, 3, 1

        def __init__(self, like):
            super().__init__()
            self.ffn, self.criterion, self.output_transform = like.ffn, like.criterion, like.output_transform

    model = _model()
    model.predictor = Other(model.predictor)
    with pytest.raises(NotImplementedError, match="known class"):
        PredictSpec(model)
    assert predict_spec(model) is None and predict_spec(_model(activation="prelu")) is None
    # the cache follows a swapped predictor
    model = _model()
    first = predict_spec(model)
    assert first is not None and predict_spec(model) is first and first.transform == "unscale"
    model.predictor = cm.MveFFN(n_tasks=3, input_dim=16, hidden_dim=8)
    second = predict_spec(model)
    assert second is not first and second.transform == "mve"


def test_fused_predict_leaves_training_mode_and_grad_mode_to_the_module_path(monkeypatch):
    """``None`` in training mode and with grad enabled, before anything is handed to the library (whose call is made to fail here)."""
    from chemprop_amd import predict, synth

    class NoLib:
        def __getattr__(self, name):
            raise AssertionError(f"the library was reached ({name})")

    model = _model()
    bmg = synth.random_batch(5, "qm9", seed=1)
    monkeypatch.setattr(predict._lib, "load", lambda: NoLib())
    model.train()
    with torch.no_grad():
        assert predict.fused_predict(model, bmg) is None
    model.eval()
    with torch.enable_grad():
        assert predict.fused_predict(model, bmg) is None
    with torch.no_grad():   # (eval mode, no grad, but the model lives on the CPU: the module path)
        assert predict.fused_predict(model, bmg) is None
