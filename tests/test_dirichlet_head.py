"""Dirichlet classification heads (``DMPNN_LOSS_DIRICHLET``) — everything that needs no GPU: ``masked_loss(kind="dirichlet")`` against an
independent closed form, the mirror predictors, what ``HeadSpec`` / ``PredictSpec`` take and refuse, the argument rules of
``dmpnn_head`` for the new criterion (stand-in pointers: every check stops before anything is dereferenced), and the agreement of
``include/dmpnn.h`` with ``_lib.LOSS``.

The definitions are those of chemprop 2.3.1 (``nn/predictors.py``, ``nn/metrics.py``) as the header states them.  The closed form used
here shares none of their arithmetic: the first term is the expected squared error ``E |y - p|^2`` under ``Dir(alpha)`` written with
the Dirichlet's mean and variance, the second is ``torch.distributions.kl_divergence(Dirichlet(alpha~), Dirichlet(1))``."""
import ctypes as C
import os
import re

import pytest
import torch
from torch import nn

from chemprop_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = torch.nn.functional
EINVAL, ENOSPC = -1, -3
PTR = 4096   # a non-NULL, 16-byte aligned stand-in


# ---- the criterion ---------------------------------------------------------------------------------------------------------------
def closed_form(alpha, T, w, tw, v_kl=0.2):
    """``sum(L w_row w_task [target finite]) / #finite`` with ``L = E_{p ~ Dir(alpha)} |y - p|^2 + v_kl KL(Dir(alpha~) || Dir(1))``."""
    D = torch.distributions
    K = alpha.shape[-1]
    mask = T.isfinite()
    y = F.one_hot(T.nan_to_num(nan=0.0).long(), K).to(alpha.dtype)
    S = alpha.sum(-1, keepdim=True)
    mean, var = alpha / S, alpha * (S - alpha) / (S * S * (S + 1))
    L = ((y - mean) ** 2 + var).sum(-1)   # (E (y - p)^2 = (y - E p)^2 + Var p, per class)
    a_t = torch.where(y > 0, torch.ones_like(alpha), alpha)
    L = L + v_kl * D.kl_divergence(D.Dirichlet(a_t), D.Dirichlet(torch.ones_like(a_t)))
    return (L * w.view(-1, 1) * tw.view(1, -1) * mask).sum() / mask.sum()


def _criterion_inputs(K, B=23, t=4, missing="some", seed=0):
    g = torch.Generator().manual_seed(100 * K + seed)
    alpha = F.softplus(3.0 * torch.randn(B, t, K, generator=g, dtype=torch.float64)) + 1
    T = torch.randint(0, K, (B, t), generator=g).double()
    if missing in ("some", "dead"):
        T[torch.rand(B, t, generator=g) < 0.2] = float("nan")
    if missing == "dead":
        T[:, 1] = float("nan")
    if missing == "all":
        T[:] = float("nan")
    return alpha, T, 0.5 + torch.rand(B, generator=g, dtype=torch.float64), 0.5 + torch.rand(t, generator=g, dtype=torch.float64)


@pytest.mark.parametrize("K", [2, 3, 7])
@pytest.mark.parametrize("missing", ["none", "some", "dead"])
def test_masked_loss_dirichlet_equals_the_closed_form(K, missing):
    from chemprop_amd.model import masked_loss

    alpha, T, w, tw = _criterion_inputs(K, missing=missing)
    for v_kl in (0.2, 1.5):
        got = masked_loss(alpha, T, w, tw, kind="dirichlet", v_kl=v_kl)
        want = closed_form(alpha, T, w, tw, v_kl)
        assert abs(float(got) - float(want)) <= 1e-12 * abs(float(want)), (K, missing, float(got), float(want))
    # unit weights: the defaults
    got, want = masked_loss(alpha, T, kind="dirichlet"), closed_form(alpha, T, torch.ones_like(w), torch.ones_like(tw))
    assert abs(float(got) - float(want)) <= 1e-12 * abs(float(want))
    # bounds are ignored
    m = torch.ones_like(T, dtype=torch.bool)
    assert float(masked_loss(alpha, T, lt_mask=m, gt_mask=m, kind="dirichlet")) == float(got)


def test_masked_loss_dirichlet_without_any_finite_target_is_nan():
    from chemprop_amd.model import masked_loss

    alpha, T, w, tw = _criterion_inputs(3, missing="all")
    assert torch.isnan(masked_loss(alpha, T, w, tw, kind="dirichlet")) and torch.isnan(closed_form(alpha, T, w, tw))


def test_masked_loss_dirichlet_gradient_matches_the_closed_form():
    from chemprop_amd.model import masked_loss

    alpha, T, w, tw = _criterion_inputs(7)
    a1, a2 = alpha.clone().requires_grad_(), alpha.clone().requires_grad_()
    masked_loss(a1, T, w, tw, kind="dirichlet").backward()
    closed_form(a2, T, w, tw).backward()
    assert float((a1.grad - a2.grad).abs().max()) <= 1e-12 * float(a2.grad.abs().max())
    assert bool((a1.grad[~T.isfinite()] == 0).all())


# ---- the mirrors -----------------------------------------------------------------------------------------------------------------
def test_mirror_predictors_follow_the_formulas(monkeypatch):
    """(The mirror MLP runs on the device only; it IS an ``nn.Sequential`` of torch modules, whose own ``forward`` stands in for it.)"""
    from chemprop_amd.ffn import MLP
    from chemprop_amd.model import (BinaryClassificationFFN, BinaryDirichletFFN, Dirichlet, MulticlassClassificationFFN,
                                    MulticlassDirichletFFN)

    monkeypatch.setattr(MLP, "forward", torch.nn.Sequential.forward)
    torch.manual_seed(3)
    Z = torch.randn(5, 16, dtype=torch.float64)
    b = BinaryDirichletFFN(n_tasks=3, input_dim=16, hidden_dim=8).double()
    m = MulticlassDirichletFFN(4, n_tasks=2, input_dim=16, hidden_dim=8).double()
    assert isinstance(b.criterion, Dirichlet) and isinstance(m.criterion, Dirichlet) and b.criterion.v_kl == 0.2
    assert b.criterion.kind == "dirichlet" and tuple(b.criterion.task_weights.shape) == (1, 3) and tuple(m.criterion.task_weights.shape) == (1, 2)
    assert (b.n_targets, b.n_tasks, b.output_dim) == (2, 3, 6) and (m.n_classes, m.n_tasks, m.output_dim) == (4, 2, 8)
    for pred, K in ((b, 2), (m, 4)):
        with torch.no_grad():
            alpha = F.softplus(pred.ffn(Z)).reshape(5, -1, K) + 1
            assert torch.equal(pred.train_step(Z), alpha) and tuple(alpha.shape) == (5, pred.n_tasks, K)
            S = alpha.sum(-1)
            want = torch.stack((alpha[..., 1] / S, 2 / S), 2) if K == 2 else alpha / S.unsqueeze(-1)
            got = pred.eval()(Z)
        assert tuple(got.shape) == (5, pred.n_tasks, K) and float((got - want).abs().max()) <= 1e-15
    # the same MLP as the plain classification mirrors of the same width: the state dicts move between them
    assert list(b.state_dict()) == list(BinaryClassificationFFN(n_tasks=6, input_dim=16, hidden_dim=8).state_dict())
    assert list(m.state_dict()) == list(MulticlassClassificationFFN(4, n_tasks=2, input_dim=16, hidden_dim=8).state_dict())
    for pred in (b, m):
        hp = {k: v for k, v in pred.hparams.items() if k != "cls"}
        clone = pred.hparams["cls"](**hp)
        assert type(clone) is type(pred) and clone.output_dim == pred.output_dim and clone.n_tasks == pred.n_tasks


def test_the_mirrors_are_exported():
    import chemprop_amd.model as M

    for n in ("Dirichlet", "BinaryDirichletFFN", "MulticlassDirichletFFN"):
        assert n in M.__all__ and hasattr(M, n)


# ---- HeadSpec / PredictSpec --------------------------------------------------------------------------------------------------------
def _model(pred, d_h=16):
    from chemprop_amd import agg as cagg
    from chemprop_amd.model import MPNN
    from chemprop_amd.nn import BondMessagePassing

    return MPNN(BondMessagePassing(d_h=d_h, depth=2), cagg.MeanAggregation(), pred, batch_norm=True)


def test_headspec_takes_both_mirror_pairs():
    from chemprop_amd.model import BinaryDirichletFFN, Dirichlet, HeadSpec, MulticlassDirichletFFN

    s = HeadSpec(_model(BinaryDirichletFFN(n_tasks=3, input_dim=16, hidden_dim=8, criterion=Dirichlet(torch.ones(3), v_kl=0.35))))
    assert (s.kind, s.n_classes, s.n_tasks, s.n_out, s.bounded) == ("dirichlet", 2, 3, 6, False) and s.v_kl == pytest.approx(0.35)
    s = HeadSpec(_model(MulticlassDirichletFFN(5, n_tasks=4, input_dim=16, hidden_dim=8)))
    assert (s.kind, s.n_classes, s.n_tasks, s.n_out) == ("dirichlet", 5, 4, 20) and s.v_kl == pytest.approx(0.2)
    h = _lib.HeadArgs()
    T = torch.zeros(6, 4)
    keep = s.fill(h, 10, 6, 16, torch.zeros(10, dtype=torch.int64), T, None, None, None, lambda p: None)
    assert (h.loss, h.n_classes, h.dims[h.n_layers]) == (_lib.LOSS["dirichlet"], 5, 20) and h.evid_v_kl == pytest.approx(0.2)
    del keep


def test_headspec_tells_the_reference_classes_by_name():
    """Stand-ins that carry the reference's class names in their MRO and none of the mirrors' marks (no ``kind`` on the criterion)."""
    from chemprop_amd.model import HeadSpec, MulticlassClassificationFFN, RegressionFFN

    class DirichletLoss(nn.Module):
        def __init__(self, t, v_kl=0.2):
            super().__init__()
            self.register_buffer("task_weights", torch.ones(1, t))
            self.v_kl = v_kl

    RefBinary = type("BinaryDirichletFFN", (RegressionFFN,), {"n_targets": 2})
    RefMulti = type("MulticlassDirichletFFN", (MulticlassClassificationFFN,), {})
    Sub = type("MyHead", (RefBinary,), {})
    for cls in (RefBinary, Sub):
        s = HeadSpec(_model(cls(n_tasks=3, input_dim=16, hidden_dim=8, criterion=DirichletLoss(3, 0.4))))
        assert (s.kind, s.n_classes, s.n_tasks, s.n_out) == ("dirichlet", 2, 3, 6) and s.v_kl == pytest.approx(0.4)
    s = HeadSpec(_model(RefMulti(3, n_tasks=2, input_dim=16, hidden_dim=8, criterion=DirichletLoss(2))))
    assert (s.kind, s.n_classes, s.n_tasks, s.n_out) == ("dirichlet", 3, 2, 6)


def test_headspec_refuses_the_crossed_pairs():
    from chemprop_amd.model import (BCE, CE, MSE, BinaryClassificationFFN, BinaryDirichletFFN, Dirichlet, HeadSpec, MulticlassClassificationFFN,
                                    MulticlassDirichletFFN, MveFFN, RegressionFFN)

    kw = dict(input_dim=16, hidden_dim=8)
    for pred in (BinaryClassificationFFN(n_tasks=4, criterion=Dirichlet(1.0), **kw), RegressionFFN(n_tasks=4, criterion=Dirichlet(1.0), **kw),
                 MulticlassClassificationFFN(3, n_tasks=2, criterion=Dirichlet(1.0), **kw), MveFFN(n_tasks=2, criterion=Dirichlet(1.0), **kw)):
        with pytest.raises(NotImplementedError, match="Dirichlet criterion on a predictor"):
            HeadSpec(_model(pred))
    for pred in (BinaryDirichletFFN(n_tasks=2, criterion=BCE(1.0), **kw), BinaryDirichletFFN(n_tasks=2, criterion=MSE(1.0), **kw),
                 MulticlassDirichletFFN(3, n_tasks=2, criterion=CE(1.0), **kw)):
        with pytest.raises(NotImplementedError, match="Dirichlet predictor .* criterion other than DirichletLoss"):
            HeadSpec(_model(pred))


def test_predictspec_refuses_dirichlet_predictors():
    from chemprop_amd.model import BinaryDirichletFFN, MulticlassDirichletFFN
    from chemprop_amd.predict import PredictSpec, predict_spec

    for pred in (BinaryDirichletFFN(n_tasks=3, input_dim=16, hidden_dim=8), MulticlassDirichletFFN(4, n_tasks=2, input_dim=16, hidden_dim=8)):
        m = _model(pred)
        with pytest.raises(NotImplementedError, match="Dirichlet predictor"):
            PredictSpec(m)
        assert predict_spec(m) is None


def test_fused_trainer_refusals_name_the_pair():
    """The refusal is ``HeadSpec``'s: a crossed pair says which half is wrong before any device is asked for."""
    from chemprop_amd.model import BCE, BinaryDirichletFFN, FusedTrainer

    with pytest.raises(NotImplementedError, match="FusedTrainer: a Dirichlet predictor"):
        FusedTrainer(_model(BinaryDirichletFFN(n_tasks=2, input_dim=16, hidden_dim=8, criterion=BCE(1.0))))


# ---- the argument rules of dmpnn_head --------------------------------------------------------------------------------------------
def _head(loss, n_classes, n_out, **kw):
    h = _lib.HeadArgs()
    h.n_atoms, h.n_mols, h.d_h, h.batch = 10, 4, 8, PTR
    dims = (8, 8, n_out)
    h.n_layers, h.act = 2, _lib.ACT["relu"]
    for i, v in enumerate(dims):
        h.dims[i] = v
    h.W[0] = h.W[1] = PTR
    h.preds, h.targets, h.loss_out = PTR, PTR, PTR
    h.loss, h.n_classes, h.evid_v_kl = loss, n_classes, 0.2
    for k, v in kw.items():
        setattr(h, k, v)
    return h


RULES = [
    ("dirichlet, valid", _lib.LOSS.get("dirichlet", 7), 2, 6, {}, ENOSPC, "workspace"),
    ("dirichlet, valid, 3 classes", _lib.LOSS.get("dirichlet", 7), 3, 6, {}, ENOSPC, "workspace"),
    ("loss 8", 8, 2, 6, {}, EINVAL, "unknown criterion"),
    ("loss -1", -1, 2, 6, {}, EINVAL, "unknown criterion"),
    ("dirichlet, one class", 7, 1, 6, {}, EINVAL, "Dirichlet criterion needs n_classes"),
    ("dirichlet, no classes", 7, 0, 6, {}, EINVAL, "Dirichlet criterion needs n_classes"),
    ("dirichlet, classes do not divide", 7, 4, 6, {}, EINVAL, "Dirichlet criterion needs n_classes"),
    ("dirichlet, lt_mask", 7, 2, 6, dict(lt_mask=PTR), EINVAL, "bounds"),
    ("dirichlet, gt_mask", 7, 2, 6, dict(gt_mask=PTR), EINVAL, "bounds"),
]


@pytest.mark.parametrize("rule,loss,n_classes,n_out,extra,code,names", RULES, ids=[r[0] for r in RULES])
def test_head_argument_rules(rule, loss, n_classes, n_out, extra, code, names):
    lib = _lib.load()
    h = _head(loss, n_classes, n_out, **extra)
    rc = lib.dmpnn_head(C.byref(h), PTR, 8, None)
    msg = lib.dmpnn_last_error_string().decode()
    assert rc == code and names in msg, (rule, rc, msg)


def test_predict_head_takes_the_criterion_beside_the_softmax_transform():
    """``dmpnn_predict_head`` with targets: the criterion's range check knows 7, and its outputs per task are the softmax's."""
    lib = _lib.load()
    p = _lib.PredictArgs()
    h = _head(7, 3, 6)
    C.memmove(C.byref(p.head), C.byref(h), C.sizeof(h))
    p.transform = _lib.PREDICT_TRANSFORM["softmax"]
    assert lib.dmpnn_predict_head(C.byref(p), PTR, 8, None) == ENOSPC and "workspace" in lib.dmpnn_last_error_string().decode()
    p.head.loss = 8
    assert lib.dmpnn_predict_head(C.byref(p), PTR, 8, None) == EINVAL and "unknown criterion" in lib.dmpnn_last_error_string().decode()
    p.head.loss, p.transform = 7, _lib.PREDICT_TRANSFORM["sigmoid"]
    assert lib.dmpnn_predict_head(C.byref(p), PTR, 8, None) == EINVAL and "disagree" in lib.dmpnn_last_error_string().decode()


# ---- header and mirror -----------------------------------------------------------------------------------------------------------
def test_the_header_and_lib_agree_on_the_criteria_and_the_abi_version_stays():
    src = open(os.path.join(ROOT, "include", "dmpnn.h")).read()
    enum = re.search(r"enum dmpnn_loss \{(.*?)\};", src, re.S).group(1)
    enum = re.sub(r"/\*.*?\*/", "", enum, flags=re.S)
    in_header = {m.group(1).lower(): int(m.group(2)) for m in re.finditer(r"DMPNN_LOSS_([A-Z]+)\s*=\s*(\d+)", enum)}
    assert in_header == _lib.LOSS and in_header["dirichlet"] == 7
    assert re.search(r"#define DMPNN_ABI_VERSION (\d+)", src).group(1) == "15"
    assert _lib.load().dmpnn_version() == 15
