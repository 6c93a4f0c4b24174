"""One-call inference for the Dirichlet classification heads (``DMPNN_PT_DIRICHLET_BINARY`` = 10, ``DMPNN_PT_DIRICHLET_MULTICLASS`` = 11) —
everything that needs no GPU: the header against ``_lib``, the argument rules of ``dmpnn_predict_head`` for the two transforms (stand-in
pointers: every check stops before anything is dereferenced, the style of ``tests/test_predict_head.py``), what ``PredictSpec(model,
dirichlet=True)`` takes and refuses, the default's unchanged refusal with the cache-slot rule of ``predict_spec``, and the module path
as the fallback off the device."""
import ctypes as C
import os
import re

import pytest
import torch
from torch import nn

from chemprop_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, ENOSPC = -1, -3
PTR = 4096   # a non-NULL, 16-byte aligned stand-in
BINARY, MULTI = 10, 11
DIRICHLET, MSE = _lib.LOSS["dirichlet"], _lib.LOSS["mse"]


# ---- header and mirror -----------------------------------------------------------------------------------------------------------
def test_the_header_and_lib_agree_on_the_two_transforms():
    src = open(os.path.join(ROOT, "include", "dmpnn.h")).read()
    assert int(re.search(r"#define DMPNN_PT_DIRICHLET_BINARY (\d+)", src).group(1)) == _lib.PT_DIRICHLET_BINARY == BINARY
    assert int(re.search(r"#define DMPNN_PT_DIRICHLET_MULTICLASS (\d+)", src).group(1)) == _lib.PT_DIRICHLET_MULTICLASS == MULTI
    assert not {"dirichlet_binary", "dirichlet_multiclass"} & set(_lib.PREDICT_TRANSFORM)   # (the enum's values stay what they were)
    assert re.search(r"#define DMPNN_ABI_VERSION (\d+)", src).group(1) == "15" and _lib.load().dmpnn_version() == 15
    for unknown in (7, 9, 12):
        rc, msg = _call(_args(unknown, 2, 6))
        assert rc == EINVAL and "unknown transform" in msg, (unknown, rc, msg)


# ---- the argument rules of dmpnn_predict_head ------------------------------------------------------------------------------------
def _args(transform, n_classes, n_out, loss=None, **kw):
    p = _lib.PredictArgs()
    h = p.head
    h.n_atoms, h.n_mols, h.d_h, h.batch = 10, 4, 8, PTR
    h.n_layers, h.act = 2, _lib.ACT["relu"]
    for i, v in enumerate((8, 8, n_out)):
        h.dims[i] = v
    h.W[0] = h.W[1] = PTR
    h.preds, h.n_classes, h.evid_v_kl = PTR, n_classes, 0.2
    if loss is not None:
        h.targets, h.loss_out, h.loss = PTR, PTR, loss
    p.transform = transform
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def _call(p):
    lib = _lib.load()
    rc = lib.dmpnn_predict_head(C.byref(p), PTR, 8, None)
    return rc, lib.dmpnn_last_error_string().decode()


BOTH = dict(out_mean=PTR, out_scale=PTR)
RULES = [
    ("binary, valid", (BINARY, 2, 6), {}, ENOSPC, "workspace"),
    ("multiclass, valid", (MULTI, 3, 6), {}, ENOSPC, "workspace"),
    ("multiclass, two classes", (MULTI, 2, 6), {}, ENOSPC, "workspace"),
    ("binary, three classes", (BINARY, 3, 6), {}, EINVAL, "binary Dirichlet transform needs head.n_classes == 2"),
    ("binary, no classes", (BINARY, 0, 6), {}, EINVAL, "binary Dirichlet transform needs head.n_classes == 2"),
    ("binary, odd width", (BINARY, 2, 7), {}, EINVAL, "binary Dirichlet transform needs head.n_classes == 2"),
    ("multiclass, one class", (MULTI, 1, 6), {}, EINVAL, "multiclass Dirichlet transform needs head.n_classes >= 2 dividing"),
    ("multiclass, no classes", (MULTI, 0, 6), {}, EINVAL, "multiclass Dirichlet transform needs head.n_classes >= 2 dividing"),
    ("multiclass, classes do not divide", (MULTI, 4, 6), {}, EINVAL, "multiclass Dirichlet transform needs head.n_classes >= 2 dividing"),
    ("binary, out_mean / out_scale", (BINARY, 2, 6), BOTH, EINVAL, "Dirichlet transforms take no out_mean / out_scale"),
    ("multiclass, out_mean / out_scale", (MULTI, 3, 6), BOTH, EINVAL, "Dirichlet transforms take no out_mean / out_scale"),
    ("binary beside the Dirichlet criterion", (BINARY, 2, 6, DIRICHLET), {}, ENOSPC, "workspace"),
    ("multiclass beside the Dirichlet criterion", (MULTI, 3, 6, DIRICHLET), {}, ENOSPC, "workspace"),
    ("binary beside MSE", (BINARY, 2, 6, MSE), {}, EINVAL, "disagree"),
    ("multiclass beside MSE", (MULTI, 3, 6, MSE), {}, EINVAL, "disagree"),
]


@pytest.mark.parametrize("rule,args,extra,code,names", RULES, ids=[r[0] for r in RULES])
def test_predict_head_argument_rules(rule, args, extra, code, names):
    rc, msg = _call(_args(*args, **extra))
    assert rc == code and names in msg, (rule, rc, msg)


def test_the_size_functions_know_the_two_transforms():
    lib = _lib.load()
    for tr, nc in ((BINARY, 2), (MULTI, 3)):
        assert lib.dmpnn_predict_head_ws_bytes(C.byref(_args(tr, nc, 6))) > 0
    for unknown in (7, 9, 12):
        assert lib.dmpnn_predict_head_ws_bytes(C.byref(_args(unknown, 2, 6))) == 0


# ---- PredictSpec / predict_spec --------------------------------------------------------------------------------------------------
def _model(pred, d_h=16):
    from chemprop_amd import agg as cagg
    from chemprop_amd.model import MPNN
    from chemprop_amd.nn import BondMessagePassing

    return MPNN(BondMessagePassing(d_h=d_h, depth=2), cagg.MeanAggregation(), pred, batch_norm=True)


def _mirrors():
    from chemprop_amd.model import BinaryDirichletFFN, MulticlassDirichletFFN

    return (BinaryDirichletFFN(n_tasks=3, input_dim=16, hidden_dim=8), MulticlassDirichletFFN(4, n_tasks=2, input_dim=16, hidden_dim=8))


def test_predictspec_takes_both_mirror_pairs_with_the_flag():
    from chemprop_amd.predict import PredictSpec

    b, m = (PredictSpec(_model(p), dirichlet=True) for p in _mirrors())
    assert (b.transform, b.kind, b.n_tasks, b.n_classes, b.n_out) == ("dirichlet_binary", "dirichlet", 3, 2, 6)
    assert b.out_shape(5) == (5, 3, 2) and b.unscale is None
    assert (m.transform, m.kind, m.n_tasks, m.n_classes, m.n_out) == ("dirichlet_multiclass", "dirichlet", 2, 4, 8)
    assert m.out_shape(5) == (5, 2, 4) and m.unscale is None


def test_predictspec_tells_the_reference_classes_by_name():
    """Stand-ins that carry the reference's class names in their MRO and none of the mirrors' marks (``tests/test_dirichlet_head.py``)."""
    from chemprop_amd.model import MulticlassClassificationFFN, RegressionFFN
    from chemprop_amd.predict import PredictSpec

    class DirichletLoss(nn.Module):
        def __init__(self, t, v_kl=0.2):
            super().__init__()
            self.register_buffer("task_weights", torch.ones(1, t))
            self.v_kl = v_kl

    RefBinary = type("BinaryDirichletFFN", (RegressionFFN,), {"n_targets": 2})
    RefMulti = type("MulticlassDirichletFFN", (MulticlassClassificationFFN,), {})
    Sub = type("MyHead", (RefBinary,), {})
    for cls in (RefBinary, Sub):
        s = PredictSpec(_model(cls(n_tasks=3, input_dim=16, hidden_dim=8, criterion=DirichletLoss(3, 0.4))), dirichlet=True)
        assert (s.transform, s.n_tasks, s.n_classes, s.out_shape(7)) == ("dirichlet_binary", 3, 2, (7, 3, 2)) and s.v_kl == pytest.approx(0.4)
    s = PredictSpec(_model(RefMulti(3, n_tasks=2, input_dim=16, hidden_dim=8, criterion=DirichletLoss(2))), dirichlet=True)
    assert (s.transform, s.n_tasks, s.n_classes, s.out_shape(7)) == ("dirichlet_multiclass", 2, 3, (7, 2, 3))


def test_predictspec_refuses_an_output_transform_and_a_crossed_pair():
    from chemprop_amd.model import BCE, BinaryDirichletFFN
    from chemprop_amd.predict import PredictSpec

    class UnscaleTransform(nn.Module):
        def __init__(self, t):
            super().__init__()
            self.register_buffer("mean", torch.zeros(1, t))
            self.register_buffer("scale", torch.ones(1, t))

    for pred in _mirrors():
        pred.output_transform = UnscaleTransform(pred.n_tasks)
        with pytest.raises(NotImplementedError, match="Dirichlet predictor with an output transform that is not the identity"):
            PredictSpec(_model(pred), dirichlet=True)
    with pytest.raises(NotImplementedError, match="criterion other than DirichletLoss"):   # (HeadSpec's pairs, no others)
        PredictSpec(_model(BinaryDirichletFFN(n_tasks=2, input_dim=16, hidden_dim=8, criterion=BCE(1.0))), dirichlet=True)


def test_the_flag_changes_nothing_for_the_other_predictors():
    from chemprop_amd.model import MulticlassClassificationFFN, RegressionFFN
    from chemprop_amd.predict import PredictSpec, predict_spec

    assert PredictSpec(_model(RegressionFFN(n_tasks=3, input_dim=16, hidden_dim=8)), dirichlet=True).transform == "unscale"
    m = _model(MulticlassClassificationFFN(4, n_tasks=2, input_dim=16, hidden_dim=8))
    assert PredictSpec(m, dirichlet=True).transform == "softmax"
    assert predict_spec(m, dirichlet=True) is predict_spec(m)   # (one spec — one workspace — however such a model is asked for)


def test_the_default_still_refuses_and_its_cached_refusal_does_not_answer_the_opt_in():
    from chemprop_amd.predict import PredictSpec, predict_spec

    for pred in _mirrors():
        m = _model(pred)
        with pytest.raises(NotImplementedError, match="Dirichlet predictor .* its eval-mode forward runs on the modules"):
            PredictSpec(m)
        assert predict_spec(m) is None                      # (cached now, as a refusal)
        spec = predict_spec(m, dirichlet=True)
        assert spec is not None and spec.transform.startswith("dirichlet_")
        assert predict_spec(m, dirichlet=True) is spec      # (and the opt-in's answer is cached in a slot of its own)
        assert predict_spec(m) is None and predict_spec(m, False) is None


# ---- the fallback off the device -------------------------------------------------------------------------------------------------
def test_off_the_device_predict_is_the_modules_forward(monkeypatch):
    """A CPU model: ``fused_predict`` is ``None`` and ``MPNN.predict`` is ``forward``.  (The mirror MLP and the block run on the device
    only: ``nn.Sequential``'s own ``forward`` and a fixed ``H_v`` stand in for them.)"""
    from chemprop_amd import synth
    from chemprop_amd.ffn import MLP
    from chemprop_amd.predict import fused_predict

    monkeypatch.setattr(MLP, "forward", torch.nn.Sequential.forward)
    bmg = synth.random_batch(5, "qm9", seed=1)
    Hv = torch.randn(int(bmg.V.shape[0]), 16, generator=torch.Generator().manual_seed(4))
    for pred in _mirrors():
        model = _model(pred).eval()
        model.message_passing.forward = lambda *a, **k: Hv
        model.agg.forward = lambda H, batch: torch.zeros(5, 16).index_add(0, batch, H) / torch.bincount(batch, minlength=5).view(-1, 1)
        with torch.no_grad():
            assert fused_predict(model, bmg) is None
            got, want = model.predict(bmg), model(bmg)
        assert tuple(got.shape) == (5, pred.n_tasks, 2 if pred.n_tasks == 3 else 4) and torch.equal(got, want)
