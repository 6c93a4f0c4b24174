"""Binary MCC heads (``BinaryClassificationFFN`` with ``BinaryMCCLoss``) without a GPU: the contract of ``include/dmpnn.h`` ("The
binary MCC criterion") — ``masked_loss(kind="mcc")``, the module path's criterion and the restatement the GPU files of this feature
import as their float64 reference and float32 yardstick (``mcc_criterion``) — against the header's closed-form gradient worked out
here independently (``mcc_closed_form``), the corner cases the header declares, and what ``HeadSpec`` / ``PredictSpec`` / ``_lib`` and
the library's argument rules make of such a model.
"""
import ctypes as C
import re
from pathlib import Path

import pytest
import torch

from chemprop_amd import _lib
from chemprop_amd import agg as cagg
from chemprop_amd.model import (BCE, MPNN, BinaryClassificationFFN, BinaryMCC, HeadSpec, MulticlassClassificationFFN, RegressionFFN,
                                criterion_kind, criterion_loss, masked_loss)
from chemprop_amd.nn import BondMessagePassing

ROOT = Path(__file__).resolve().parents[1]


# ---- the contract ---------------------------------------------------------------------------------------------------------------------
def mcc_criterion(x, T, w, tw):
    """The criterion on the raw logits ``x [B, t]``: the torch-op restatement of the header (differentiable, any dtype)."""
    return masked_loss(x, T, w, tw, kind="mcc")


def mcc_closed_form(x, T, w, tw):
    """``(loss, dloss/dx, MCC_j)`` by the header's formulas, without autograd: the four sums, ``g(dN, dD)``, ``alpha_j``, ``beta_j``."""
    m = T.isfinite()
    y = torch.where(m, T, torch.zeros_like(T))
    p = torch.sigmoid(x)
    a = w.view(-1, 1) * m
    t = x.shape[1]
    TP, FP = (a * y * p).sum(0), (a * (1 - y) * p).sum(0)
    TN, FN = (a * (1 - y) * (1 - p)).sum(0), (a * y * (1 - p)).sum(0)
    A, Bq, Cq, E = TP + FP, TP + FN, TN + FP, TN + FN
    S, N = (A * Bq * Cq * E + 1e-8).sqrt(), TP * TN - FP * FN
    g = lambda dN, dD: dN / S - N * dD / (2 * S ** 3)
    alpha = g(TN, Bq * Cq * E + A * Cq * E) - g(-FP, A * Cq * E + A * Bq * Cq)
    beta = g(-FN, Bq * Cq * E + A * Bq * E) - g(TP, A * Bq * E + A * Bq * Cq)
    mcc = N / S
    grad = -(tw.view(1, -1) / t) * a * (y * alpha.view(1, -1) + (1 - y) * beta.view(1, -1)) * p * (1 - p)
    return 1 - (tw * mcc).sum() / t, grad, mcc


def mcc_targets(B, t, missing, seed, positives=0.3):
    """0 / 1 targets ``[B, t]`` (float32) with about ``positives`` ones.  ``missing``: ``none``; ``some`` (20 %); ``first`` (column 0
    in every row); ``task`` (column ``t // 2`` in every row); ``all``."""
    g = torch.Generator().manual_seed(7000 + seed)
    T = (torch.rand(B, t, generator=g) < positives).float()
    if missing == "some":
        T[torch.rand(B, t, generator=g) < 0.2] = float("nan")
    elif missing == "first":
        T[:, 0] = float("nan")
    elif missing == "task":
        T[:, t // 2] = float("nan")
    elif missing == "all":
        T[:] = float("nan")
    else:
        assert missing == "none", missing
    return T


def _inputs(B=23, t=5, seed=0, missing="some"):
    g = torch.Generator().manual_seed(seed)
    x = 2 * torch.randn(B, t, generator=g, dtype=torch.float64)
    return x, mcc_targets(B, t, missing, seed).double(), (0.5 + torch.rand(B, generator=g)).double(), (0.5 + torch.rand(t, generator=g)).double()


@pytest.mark.parametrize("missing", ["none", "some", "first", "task"])
@pytest.mark.parametrize("B,t", [(1, 1), (2, 3), (23, 5), (130, 12)])
def test_masked_loss_is_the_headers_closed_form(B, t, missing):
    if missing in ("first", "task") and t == 1:
        missing = "none"
    x, T, w, tw = _inputs(B, t, missing=missing)
    x.requires_grad_()
    got = mcc_criterion(x, T, w, tw)
    (gg,) = torch.autograd.grad(got, x)
    loss, grad, _ = mcc_closed_form(x.detach(), T, w, tw)
    assert abs(float(got.detach()) - float(loss)) <= 1e-14
    assert float((gg - grad).abs().max()) <= 1e-13 * max(float(grad.abs().max()), 1e-3)
    if B >= 23 and missing == "none":
        assert float(grad.abs().max()) > 1e-4 and abs(float(loss) - 1) > 1e-3   # (not a vacuous comparison)


def test_the_criterion_module_and_criterion_loss_give_the_same_number():
    x, T, w, tw = _inputs()
    crit = BinaryMCC(tw).double()
    want = float(mcc_criterion(x, T, w, tw))
    for v in (criterion_loss(crit, x, T, w), crit(x, T, weights=w), crit(x, T.nan_to_num(), mask=T.isfinite(), weights=w)):
        assert abs(float(v) - want) <= 1e-15
    assert abs(float(masked_loss(x, T, None, None, kind="mcc")) - float(mcc_criterion(x, T, torch.ones(23).double(), torch.ones(5).double()))) <= 1e-15
    # (bounds masks are not the criterion's business)
    assert float(masked_loss(x, T, w, tw, lt_mask=torch.ones_like(T, dtype=torch.bool), kind="mcc")) == want


def test_a_perfect_and_an_inverted_classifier():
    T = mcc_targets(40, 3, "none", 1).double()
    one, tw = torch.ones(40).double(), torch.ones(3).double()
    assert abs(float(mcc_criterion(40 * (2 * T - 1), T, one, tw))) <= 1e-12            # MCC = 1: loss 0
    assert abs(float(mcc_criterion(-40 * (2 * T - 1), T, one, tw)) - 2) <= 1e-12       # MCC = -1: loss 2


# ---- the corner cases the header declares ---------------------------------------------------------------------------------------------
def test_a_task_without_a_finite_target_has_mcc_zero_and_gradient_exactly_zero():
    x, T, w, tw = _inputs(missing="task")
    x.requires_grad_()
    loss = mcc_criterion(x, T, w, tw)
    (g,) = torch.autograd.grad(loss, x)
    _, grad, mcc = mcc_closed_form(x.detach(), T, w, tw)
    col = T.shape[1] // 2
    assert float(mcc[col]) == 0.0 and float(g[:, col].abs().max()) == 0.0 and float(grad[:, col].abs().max()) == 0.0
    # the mean runs over all t tasks: the same batch without that column, rescaled
    keep = [j for j in range(T.shape[1]) if j != col]
    rest = mcc_criterion(x.detach()[:, keep], T[:, keep], w, tw[keep])
    assert abs((1 - float(loss)) * T.shape[1] - (1 - float(rest)) * len(keep)) <= 1e-14


@pytest.mark.parametrize("cls", [0.0, 1.0])
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_a_one_class_task_has_mcc_zero_and_gradient_exactly_zero(cls, dtype):
    x, T, w, tw = (v.to(dtype) for v in _inputs(missing="some"))
    T[T[:, 1].isfinite(), 1] = cls
    x.requires_grad_()
    (g,) = torch.autograd.grad(mcc_criterion(x, T, w, tw), x)
    _, grad, mcc = mcc_closed_form(x.detach(), T, w, tw)
    assert float(mcc[1]) == 0.0 and float(grad[:, 1].abs().max()) == 0.0    # (exactly: N and the present class's dN, dD vanish)
    assert float(g[:, 1].abs().max()) <= 1e-6                               # (autograd of the quotient: merely small)
    assert float(grad[:, 0].abs().max()) > 1e-4


def test_a_batch_without_a_finite_target_is_loss_one():
    x, T, w, tw = _inputs(missing="all")
    x.requires_grad_()
    loss = mcc_criterion(x, T, w, tw)
    (g,) = torch.autograd.grad(loss, x)
    assert float(loss) == 1.0 and float(g.abs().max()) == 0.0
    assert float(mcc_closed_form(x.detach(), T, w, tw)[0]) == 1.0


def test_rows_of_weight_zero_take_no_part():
    x, T, w, tw = _inputs(B=40, missing="some")
    w[::4] = 0.0
    x.requires_grad_()
    loss = mcc_criterion(x, T, w, tw)
    (g,) = torch.autograd.grad(loss, x)
    assert float(g[::4].abs().max()) == 0.0 and float(g.abs().max()) > 1e-4
    keep = w > 0
    assert abs(float(loss) - float(mcc_criterion(x.detach()[keep], T[keep], w[keep], tw))) <= 1e-14
    w[:] = 0.0
    assert float(mcc_criterion(x.detach(), T, w, tw)) == 1.0


# ---- HeadSpec / PredictSpec / criterion_kind ------------------------------------------------------------------------------------------
def _model(t=7, crit=None, pred_cls=BinaryClassificationFFN, d_h=8, **kw):
    torch.manual_seed(3)
    mp = BondMessagePassing(d_h=d_h, depth=2, activation="tanh")
    pred = pred_cls(n_tasks=t, input_dim=d_h, hidden_dim=11, activation="tanh", criterion=BinaryMCC(torch.ones(t)) if crit is None else crit, **kw)
    return MPNN(mp, cagg.MeanAggregation(), pred, batch_norm=True)


def test_headspec_accepts_the_pair():
    spec = HeadSpec(_model())
    assert (spec.kind, spec.bounded, spec.n_tasks, spec.n_out, spec.n_classes, spec.n_targets) == ("mcc", False, 7, 7, 0, 1)
    h = _lib.HeadArgs()
    spec.fill(h, 9, 4, 8, torch.zeros(9, dtype=torch.int64), torch.zeros(4, 7), None, None, None, lambda p: None)
    assert (h.loss, h.n_classes, h.n_layers, h.dims[2]) == (11, 0, 2, 7)


def test_predictspec_inherits_and_maps_to_the_sigmoid():
    from chemprop_amd.predict import PredictSpec

    spec = PredictSpec(_model())
    assert (spec.kind, spec.transform, spec.out_shape(5)) == ("mcc", "sigmoid", (5, 7))


def test_headspec_refusals_each_by_its_message():
    with pytest.raises(NotImplementedError, match="binary MCC criterion on a predictor that is not a BinaryClassificationFFN"):
        HeadSpec(_model(pred_cls=RegressionFFN))
    with pytest.raises(NotImplementedError, match="binary MCC criterion on a predictor that is not a BinaryClassificationFFN"):
        torch.manual_seed(0)
        HeadSpec(MPNN(BondMessagePassing(d_h=8, depth=2), cagg.MeanAggregation(),
                      MulticlassClassificationFFN(3, n_tasks=7, input_dim=8, hidden_dim=11, criterion=BinaryMCC(torch.ones(7)))))

    class Multi(torch.nn.Module):
        pass

    Multi.__name__ = "MulticlassMCCLoss"
    assert criterion_kind(Multi()) == (None, False)
    with pytest.raises(NotImplementedError, match="MulticlassMCCLoss stays on torch ops"):
        HeadSpec(_model(crit=Multi()))

    class Unknown(torch.nn.Module):
        pass

    with pytest.raises(NotImplementedError, match="Wasserstein or binary MCC"):
        HeadSpec(_model(crit=Unknown()))
    assert HeadSpec(_model(crit=BCE(torch.ones(7)))).kind == "bce"   # (the same predictor keeps its other criterion)


def test_criterion_kind_on_a_class_merely_named_binarymccloss():
    class Named(torch.nn.Module):   # (the reference's classes are told by MRO name)
        pass

    Named.__name__ = "BinaryMCCLoss"
    assert criterion_kind(Named()) == ("mcc", False)

    class Metric(Named):            # (BinaryMCCMetric derives from the loss)
        pass

    assert criterion_kind(Metric()) == ("mcc", False)
    assert criterion_kind(BinaryMCC(1.0)) == ("mcc", False)
    assert HeadSpec(_model(crit=Named())).kind == "mcc"


# ---- the header and _lib ----------------------------------------------------------------------------------------------------------------
def test_lib_mirrors_follow_the_header():
    text = (ROOT / "include" / "dmpnn.h").read_text()
    body = re.search(r"enum dmpnn_loss \{(.*?)\};", text, re.S).group(1)
    assert re.search(r"DMPNN_LOSS_MCC\s*=\s*11\b", body) and not re.search(r"=\s*10\b", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert _lib.LOSS["mcc"] == 11 and 10 not in _lib.LOSS.values()
    assert int(re.search(r"#define DMPNN_ABI_VERSION (\d+)", text).group(1)) == 15 == _lib.ABI_VERSION
    assert [f[0] for f in _lib.HeadArgs._fields_][-3:] == ["g_att_b", "spectral_act", "spectral_threshold"]   # (no field added)
    for word in ("The binary MCC criterion", "1e-8", "always applied", "loss 1.0", "exactly 0"):
        assert word in text, word


# ---- argument rules through the C ABI: codes before any device work (the pointers are stand-ins, never read) ------------------------
EINVAL, ENOSPC, PTR = -1, -3, 4096


def _head(loss, n_classes=0, n_out=6, **kw):
    h = _lib.HeadArgs()
    h.n_atoms, h.n_mols, h.d_h, h.batch = 10, 4, 8, PTR
    h.n_layers, h.act = 2, _lib.ACT["relu"]
    for i, v in enumerate((8, 8, n_out)):
        h.dims[i] = v
    h.W[0] = h.W[1] = PTR
    h.preds, h.targets, h.loss_out = PTR, PTR, PTR
    h.loss, h.n_classes = loss, n_classes
    for k, v in kw.items():
        setattr(h, k, v)
    return h


HEAD_RULES = [
    ("mcc, valid", 11, {}, ENOSPC, "workspace"),
    ("mcc with a class dimension", 11, dict(n_classes=2), EINVAL, "unknown criterion"),
    ("mcc, lt_mask", 11, dict(lt_mask=PTR), EINVAL, "bounds"),
    ("mcc, gt_mask", 11, dict(gt_mask=PTR), EINVAL, "bounds"),
    ("loss 10", 10, {}, EINVAL, "unknown criterion"),
    ("loss 12", 12, {}, EINVAL, "unknown criterion"),
]


@pytest.mark.parametrize("rule,loss,extra,code,names", HEAD_RULES, ids=[r[0] for r in HEAD_RULES])
def test_head_argument_rules(rule, loss, extra, code, names):
    lib = _lib.load()
    h = _head(loss, **extra)
    rc = lib.dmpnn_head(C.byref(h), PTR, 8, None)
    msg = lib.dmpnn_last_error_string().decode()
    assert rc == code and names in msg, (rule, rc, msg)


def test_the_workspace_grows_with_the_criterion_alone_by_the_partial_sums():
    lib = _lib.load()
    src = (ROOT / "chemprop_amd" / "csrc" / "dmpnn_head_kernels.hpp").read_text()
    R = int(re.search(r"constexpr int kMccRows = (\d+);", src).group(1))
    al = lambda n: (n + 255) // 256 * 256
    for B, t in ((4, 6), (R, 6), (R + 1, 6), (3 * R + 5, 617)):
        sizes = []
        for loss in (_lib.LOSS["bce"], _lib.LOSS["mcc"]):
            h = _head(loss, n_out=t)
            h.n_mols = B
            sizes.append(int(lib.dmpnn_head_ws_bytes(C.byref(h))))
        nb, ncb = -(-B // R), -(-t // 256)
        assert sizes[1] - sizes[0] == al(nb * t * 4 * 4) + al(nb * ncb * 4), (B, t, sizes)


def test_predict_head_argument_rules():
    lib = _lib.load()

    def call(transform, **head):
        p = _lib.PredictArgs()
        h = _head(head.pop("loss"), **head)
        C.memmove(C.byref(p.head), C.byref(h), C.sizeof(h))
        p.transform, p.preds = transform, PTR
        rc = lib.dmpnn_predict_head(C.byref(p), PTR, 8, None)
        return rc, lib.dmpnn_last_error_string().decode()

    rc, msg = call(_lib.PREDICT_TRANSFORM["sigmoid"], loss=11)
    assert rc == ENOSPC and "workspace" in msg, (rc, msg)
    rc, msg = call(_lib.PREDICT_TRANSFORM["sigmoid"], loss=11, n_classes=2)
    assert rc == EINVAL and "unknown criterion" in msg, (rc, msg)
    rc, msg = call(_lib.PREDICT_TRANSFORM["mve"], loss=11)   # (two outputs per task against the criterion's one)
    assert rc == EINVAL and "disagree" in msg, (rc, msg)
