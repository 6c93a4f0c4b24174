"""The prediction heads: the criteria (``chemprop.nn.metrics``), the predictors (``chemprop.nn.predictors``) and the two tables that say
which of them meet and how their outputs are laid out, :data:`CRITERIA` and :data:`PREDICTORS` — read by ``model.HeadSpec``,
``predict.PredictSpec`` and ``metrics.kind_of_model``.  A new head: its criterion on torch ops, a row in each table, the mirror classes."""
from __future__ import annotations

import math
from collections import namedtuple
from typing import Optional

import torch
from torch import Tensor, nn

from . import _lib
from .ffn import MLP

F = torch.nn.functional


# ---- the criteria on torch ops: fn(preds, targets, **what masked_loss knows) -> the loss of every (molecule, task) ------------------------
def _mve(preds, targets, **_):   # MVELoss, metrics.py:203-219; preds [b, t, 2 | 4]: what MveFFN / EvidentialFFN / QuantileFFN.train_step stack
    mean, var = torch.unbind(preds, dim=-1)
    return (mean - targets) ** 2 / (2 * var) + (2 * torch.pi * var).log() / 2


def _evidential(preds, targets, v_kl, eps, **_):   # EvidentialLoss, metrics.py:222-262
    mean, v, alpha, beta = torch.unbind(preds, dim=-1)
    residuals = targets - mean
    two_b_lambda = 2 * beta * (1 + v)
    L_nll = (0.5 * (torch.pi / v).log() - alpha * two_b_lambda.log() + (alpha + 0.5) * torch.log(v * residuals**2 + two_b_lambda)
             + torch.lgamma(alpha) - torch.lgamma(alpha + 0.5))
    return L_nll + v_kl * ((2 * v + alpha) * residuals.abs() - eps)


def _quantile(preds, targets, alpha, **_):   # QuantileLoss, metrics.py:589-610
    mean, interval = torch.unbind(preds, dim=-1)
    bounds = torch.tensor([-0.5, 0.5], device=preds.device).view(-1, 1, 1)
    tau = torch.tensor([[alpha / 2, 1 - alpha / 2], [alpha / 2 - 1, -alpha / 2]], device=preds.device).view(2, 2, 1, 1)
    return (tau * (targets - (mean + bounds * interval))).amax(0).sum(0)


def _dirichlet(preds, targets, v_kl, **_):   # preds [b, t, c] = alpha (the Dirichlet predictors' train_step), targets [b, t] class indices
    y = F.one_hot(targets.long(), preds.shape[-1]).to(preds.dtype)
    S = preds.sum(-1, keepdim=True)
    p = preds / S
    L_mse = ((y - p) ** 2).sum(-1) + (p * (1 - p) / (S + 1)).sum(-1)
    a_t = y + (1 - y) * preds    # (1 at the true class: the KL term leaves its evidence alone)
    S_t = a_t.sum(-1, keepdim=True)
    L_kl = (torch.lgamma(S_t).squeeze(-1) - torch.lgamma(a_t).sum(-1) - math.lgamma(preds.shape[-1])
            + ((a_t - 1) * (torch.digamma(a_t) - torch.digamma(S_t))).sum(-1))
    return L_mse + v_kl * L_kl


def _sid(preds, targets, mask, threshold, **_):   # preds [b, t] = p, renormalised over the finite targets (masked q and y filled with 1: a zero term)
    c = preds if threshold is None else preds.clamp(min=threshold)
    q = c / (c * mask).sum(1, keepdim=True)
    one = torch.ones_like(q)
    qm, ym = torch.where(mask, q, one), torch.where(mask, targets, one)
    return qm * (qm / ym).log() + ym * (ym / qm).log()


def _wasserstein(preds, targets, mask, threshold, **_):   # (the running sum of q includes the masked columns; only y is 0 there)
    c = preds if threshold is None else preds.clamp(min=threshold)
    return (targets.cumsum(1) - (c / (c * mask).sum(1, keepdim=True)).cumsum(1)).abs()


def _mcc(preds, targets, mask, w, tw, **_):
    """The BATCH's value: BinaryMCCLoss on logits [b, t] as include/dmpnn.h restates it (1 - p as sigmoid(-x); the mean over ALL tasks)"""
    a = w.view(-1, 1) * mask
    p, q = preds.sigmoid(), (-preds).sigmoid()
    TP, FP = (a * targets * p).sum(0), (a * (1 - targets) * p).sum(0)
    TN, FN = (a * (1 - targets) * q).sum(0), (a * targets * q).sum(0)
    mcc = (TP * TN - FP * FN) / ((TP + FP) * (TP + FN) * (TN + FP) * (TN + FN) + 1e-8).sqrt()
    return 1 - (mcc * tw).sum() / targets.shape[1]


# A criterion: `kind`, a key of _lib.LOSS; `name`, the reference's class that means it (in the MRO: the first row that matches); `bounded`:
# applies lt_mask / gt_mask (a reference class: with BoundedMixin); `values`: the outputs per task it reads (the chunks MveFFN / ... stack);
# `classes`: reads a class dimension [b, t, c]; `fn`: the criterion on torch ops; `predictors`: the only classes it is taken with (None: any
# whose layout fits) and `refusal`, HeadSpec's word on another; `alone`: those predictors take no other criterion, and its word on one that does.
Criterion = namedtuple("Criterion", "kind name bounded values classes fn predictors refusal alone", defaults=(None, None, None))
ONE_VALUE_PER_TASK = "one value per task, or MveFFN with MVELoss / EvidentialFFN with EvidentialLoss / QuantileFFN with QuantileLoss"
_SPECTRAL = (("SpectralFFN",), "a spectral criterion ({kind}) on a predictor that is not a SpectralFFN",
             "a SpectralFFN with a criterion other than SID / Wasserstein (got {kind})")
CRITERIA = (   # in match order (Wasserstein derives from SID); HeadSpec holds a model to the rows with `alone` in this order too
    Criterion("mve",         "MVELoss",          False, 2, False, _mve, ("MveFFN",), ONE_VALUE_PER_TASK),
    Criterion("evidential",  "EvidentialLoss",   False, 4, False, _evidential, ("EvidentialFFN",), ONE_VALUE_PER_TASK),
    Criterion("quantile",    "QuantileLoss",     False, 2, False, _quantile, ("QuantileFFN",), ONE_VALUE_PER_TASK),
    Criterion("mcc",         "BinaryMCCLoss",    False, 1, False, _mcc, ("BinaryClassificationFFN",),
              "a binary MCC criterion on a predictor that is not a BinaryClassificationFFN (got {cls})"),
    Criterion("bce",         "BCELoss",          False, 1, False, lambda p, t, **_: F.binary_cross_entropy_with_logits(p, t, reduction="none")),
    Criterion("ce",          "CrossEntropyLoss", False, 1, True,  lambda p, t, **_: F.cross_entropy(p.transpose(1, 2), t.long(), reduction="none")),
    Criterion("dirichlet",   "DirichletLoss",    False, 1, True,  _dirichlet, ("BinaryDirichletFFN", "MulticlassDirichletFFN"),
              "a Dirichlet criterion on a predictor that is neither BinaryDirichletFFN nor MulticlassDirichletFFN",
              "a Dirichlet predictor ({cls}) with a criterion other than DirichletLoss (got {kind})"),
    Criterion("wasserstein", "Wasserstein",      False, 1, False, _wasserstein, *_SPECTRAL),
    Criterion("sid",         "SID",              False, 1, False, _sid, *_SPECTRAL),
    Criterion("mse",         "MSE",              True,  1, False, lambda p, t, **_: F.mse_loss(p, t, reduction="none")),
    Criterion("mae",         "MAE",              True,  1, False, lambda p, t, **_: (p - t).abs()),
)
CRITERION = {c.kind: c for c in CRITERIA}
# the reference's criteria that are not built in whatever else their MRO names (RMSE: an MSE; PointQuantileLoss: a QuantileLoss), HeadSpec's refusals
UNKNOWN_CRITERION = "MSE / MAE criterion (bounded or not), BCE, cross entropy, MVE, evidential, quantile, Dirichlet, SID, Wasserstein or binary MCC"
NOT_BUILT_IN = {"RMSE": UNKNOWN_CRITERION, "PointQuantileLoss": UNKNOWN_CRITERION,
                "MulticlassMCCLoss": "MulticlassMCCLoss stays on torch ops: it reaches the logits through argmax counts and sum(softmax) alone, "
                                     "so its gradient is zero and a kernel for it would train nothing (binary MCC is built in)"}

# A predictor: `name`, the class (mirror and reference, in the MRO: the first row that matches); its eval-mode forward returns per task `values`
# numbers (> 1: a last dimension) or a class dimension, `classes`: 0 none, OWN (its n_classes), 2 (the binary Dirichlet head, whatever n_targets
# says); `transform`: that forward behind the MLP by name, `code`: as dmpnn_predict_args.transform takes it; `metric`: a key of _lib.METRIC;
# `no_unscale`: PredictSpec's refusal of an UnscaleTransform behind it (None: taken); `opt_in`: PredictSpec takes it with dirichlet=True only.
Predictor = namedtuple("Predictor", "name values classes transform code metric no_unscale opt_in", defaults=(None, False))
OWN, _PT = -1, _lib.PREDICT_TRANSFORM
_CLASSIFIER, _IDENTITY = "a classification predictor without an UnscaleTransform", "a Dirichlet predictor with an output transform that is not the identity"
PREDICTORS = (   # the specific classes first: all derive from RegressionFFN, MulticlassDirichletFFN from MulticlassClassificationFFN
    Predictor("BinaryDirichletFFN",          1, 2,   "dirichlet_binary",     _lib.PT_DIRICHLET_BINARY,     "binary",     _IDENTITY, True),
    Predictor("MulticlassDirichletFFN",      1, OWN, "dirichlet_multiclass", _lib.PT_DIRICHLET_MULTICLASS, "multiclass", _IDENTITY, True),
    Predictor("SpectralFFN",                 1, 0,   "spectral",             _lib.PT_SPECTRAL,             "none",
              "a SpectralFFN with an output transform that is not the identity"),
    Predictor("MveFFN",                      2, 0,   "mve",                  _PT["mve"],                   "regression"),
    Predictor("EvidentialFFN",               4, 0,   "evidential",           _PT["evidential"],            "regression"),
    Predictor("QuantileFFN",                 2, 0,   "quantile",             _PT["quantile"],              "regression"),
    Predictor("MulticlassClassificationFFN", 1, OWN, "softmax",              _PT["softmax"],               "multiclass", _CLASSIFIER),
    Predictor("BinaryClassificationFFN",     1, 0,   "sigmoid",              _PT["sigmoid"],               "binary",     _CLASSIFIER),
    Predictor("RegressionFFN",               1, 0,   "unscale",              _PT["unscale"],               "regression"),
)


def _mro_names(obj) -> set:
    return {c.__name__ for c in type(obj).__mro__}


def predictor_row(pred) -> Optional[Predictor]:
    """The row of :data:`PREDICTORS` for a predictor (``None``: no known class in its MRO)."""
    return next((p for p in PREDICTORS if p.name in _mro_names(pred)), None)


def criterion_kind(crit) -> tuple[Optional[str], bool]:
    """``(kind, bounded)``: a key of ``_lib.LOSS`` and whether ``lt_mask`` / ``gt_mask`` apply.  This package's criteria carry ``.kind``
    (``mse`` / ``mae``: bounded iff masks are handed over); the reference's are told by name (``MSE`` / ``MAE`` ignore the masks,
    ``BoundedMSE`` / ``BoundedMAE`` apply them: ``nn/metrics.py:139-177``).  ``(None, False)``: an unknown class, or a :data:`NOT_BUILT_IN` name
    anywhere in the MRO (the ``if`` chain before the table met ``MulticlassMCCLoss`` behind MVE / evidential / quantile and let a
    ``PointQuantileLoss`` fall through to the later names: no class of the reference tells the two apart)."""
    kind = getattr(crit, "kind", None)
    if kind in CRITERION:
        return kind, CRITERION[kind].bounded
    names = _mro_names(crit)
    row = None if names & NOT_BUILT_IN.keys() else next((c for c in CRITERIA if c.name in names), None)
    return (None, False) if row is None else (row.kind, row.bounded and "BoundedMixin" in names)


def criterion_bounded(crit) -> bool:
    """Whether ``lt_mask`` / ``gt_mask`` reach the criterion."""
    return criterion_kind(crit)[1]


def masked_loss(preds: Tensor, targets: Tensor, weights: Optional[Tensor] = None, task_weights: Optional[Tensor] = None,
                lt_mask: Optional[Tensor] = None, gt_mask: Optional[Tensor] = None, kind: str = "mse", v_kl: float = 0.2, eps: float = 1e-8,
                alpha: float = 0.1, threshold: Optional[float] = None) -> Tensor:
    """``ChempropMetric.update`` + ``compute`` on one batch (``nn/metrics.py:78-127``) with the masking of
    ``MPNN.training_step`` (``models/model.py:152-156``): torch ops, differentiable; the kind's arithmetic is its row's ``fn`` (no row: mse)."""
    row = CRITERION.get(kind, CRITERION["mse"])
    mask = targets.isfinite()
    targets = targets.nan_to_num(nan=0.0)
    w = torch.ones(targets.shape[0], dtype=torch.float, device=targets.device) if weights is None else weights
    tw = 1.0 if task_weights is None else task_weights.view(1, -1)
    if row.bounded:   # (only the Bounded* criteria apply the masks: metrics.py:157-177)
        preds = preds if lt_mask is None else torch.where((preds < targets) & lt_mask, targets, preds)
        preds = preds if gt_mask is None else torch.where((preds > targets) & gt_mask, targets, preds)
    L = row.fn(preds, targets, mask=mask, w=w, tw=tw, v_kl=v_kl, eps=eps, alpha=alpha, threshold=threshold)
    return L if row.kind == "mcc" else (L * w.view(-1, 1) * tw * mask).sum() / mask.sum()


def criterion_loss(c, preds: Tensor, targets: Tensor, weights=None, lt_mask=None, gt_mask=None) -> Tensor:
    """:func:`masked_loss` with what the criterion ``c`` carries — this package's or the reference's (``task_weights``, ``v_kl``, ...)."""
    thr = getattr(c, "threshold", None)
    return masked_loss(preds, targets, weights, getattr(c, "task_weights", None), lt_mask, gt_mask, getattr(c, "kind", "mse"),
                       float(getattr(c, "v_kl", 0.2)), float(getattr(c, "eps", 1e-8)), float(getattr(c, "alpha", 0.1)),
                       None if thr is None else float(thr))


class MSE(nn.Module):
    """The criterion's state (``nn/metrics.py:60-76``: a ``task_weights`` buffer of shape ``[1, t]``) and its batch value; only the
    kinds ``mse`` / ``mae`` apply ``lt_mask`` / ``gt_mask`` (:func:`masked_loss`)."""

    kind = "mse"

    def __init__(self, task_weights=1.0):
        super().__init__()
        self.register_buffer("task_weights", torch.as_tensor(task_weights, dtype=torch.float).view(1, -1))

    def forward(self, preds, targets, mask=None, weights=None, lt_mask=None, gt_mask=None):
        t = targets if mask is None else torch.where(mask, targets, torch.full_like(targets, float("nan")))
        return criterion_loss(self, preds, t, weights, lt_mask, gt_mask)


class MAE(MSE):
    kind = "mae"


class BCE(MSE):
    """``chemprop.nn.metrics.BCELoss`` (``metrics.py:292-295``): binary cross entropy on LOGITS; no bounds."""

    kind = "bce"


class RegressionFFN(nn.Module):
    """``chemprop.nn.predictors.RegressionFFN`` (``predictors.py:101-169``): ``ffn = MLP.build(input_dim, n_tasks, hidden_dim,
    n_layers, dropout, activation)``, criterion MSE, identity output transform while training."""

    n_targets = 1   # (values per task, ``predictors.py:132``: the MLP is ``n_tasks * n_targets`` wide)
    _default_criterion = MSE

    def __init__(self, n_tasks: int = 1, input_dim: int = 300, hidden_dim: int = 300, n_layers: int = 1, dropout: float = 0.0,
                 activation="relu", criterion: Optional[nn.Module] = None, task_weights: Optional[Tensor] = None):
        super().__init__()
        self.hparams = dict(n_tasks=n_tasks, input_dim=input_dim, hidden_dim=hidden_dim, n_layers=n_layers, dropout=dropout,
                            activation=activation, cls=self.__class__)
        self.ffn = MLP.build(input_dim, n_tasks * self.n_targets, hidden_dim, n_layers, dropout, activation)
        self.criterion = criterion if criterion is not None else self._default_criterion(torch.ones(n_tasks) if task_weights is None else task_weights)
        self.output_transform = nn.Identity()

    @property
    def input_dim(self) -> int:
        return self.ffn.input_dim

    @property
    def output_dim(self) -> int:
        return self.ffn.output_dim

    @property
    def n_tasks(self) -> int:
        return self.output_dim // self.n_targets

    def forward(self, Z: Tensor) -> Tensor:
        return self.output_transform(self.ffn(Z))

    train_step = forward


class CE(MSE):
    """``chemprop.nn.metrics.CrossEntropyLoss`` (``metrics.py:298-304``): ``preds [b, t, c]`` logits against class indices; no bounds."""

    kind = "ce"


class MVE(MSE):
    """``chemprop.nn.metrics.MVELoss`` (``metrics.py:203-219``): ``preds [b, t, 2]`` = (mean, variance); no bounds."""

    kind = "mve"


class Evidential(MSE):
    """``chemprop.nn.metrics.EvidentialLoss`` (``metrics.py:222-262``): ``preds [b, t, 4]`` = (mean, v, alpha, beta); no bounds."""

    kind = "evidential"

    def __init__(self, task_weights=1.0, v_kl: float = 0.2, eps: float = 1e-8):
        super().__init__(task_weights)
        self.v_kl, self.eps = v_kl, eps


class Quantile(MSE):
    """``chemprop.nn.metrics.QuantileLoss`` (``metrics.py:589-610``): ``preds [b, t, 2]`` = (mean, interval); no bounds."""

    kind = "quantile"

    def __init__(self, task_weights=1.0, alpha: float = 0.1):
        super().__init__(task_weights)
        self.alpha = alpha
        # (the reference's buffers, metrics.py:594-600: the state dicts match)
        self.register_buffer("bounds", torch.tensor([-1 / 2, 1 / 2]).view(-1, 1, 1))
        self.register_buffer("tau", torch.tensor([[alpha / 2, 1 - alpha / 2], [alpha / 2 - 1, -alpha / 2]]).view(2, 2, 1, 1))


class MveFFN(RegressionFFN):
    """``chemprop.nn.predictors.MveFFN`` (``predictors.py:173-190``): an MLP ``2 n_tasks`` wide, chunked into means and raw variances
    (``softplus``), stacked ``[b, t, 2]``; ``train_step`` is ``forward``.  (The output transform is the identity here, as the
    reference's ``UnscaleTransform`` is while training.)"""

    n_targets = 2
    _default_criterion = MVE

    def forward(self, Z: Tensor) -> Tensor:
        mean, var = torch.chunk(self.ffn(Z), 2, 1)
        return torch.stack((mean, torch.nn.functional.softplus(var)), dim=2)

    train_step = forward


class EvidentialFFN(RegressionFFN):
    """``chemprop.nn.predictors.EvidentialFFN`` (``predictors.py:193-212``): ``4 n_tasks`` wide — mean | v | alpha | beta,
    ``v = softplus``, ``alpha = softplus + 1``, ``beta = softplus``, stacked ``[b, t, 4]``."""

    n_targets = 4
    _default_criterion = Evidential

    def forward(self, Z: Tensor) -> Tensor:
        sp = torch.nn.functional.softplus
        mean, v, alpha, beta = torch.chunk(self.ffn(Z), 4, 1)
        return torch.stack((mean, sp(v), sp(alpha) + 1, sp(beta)), dim=2)

    train_step = forward


class QuantileFFN(RegressionFFN):
    """``chemprop.nn.predictors.QuantileFFN`` (``predictors.py:215-232``): ``2 n_tasks`` wide — lower | upper bounds, stacked as
    ``(mean, interval) [b, t, 2]``."""

    n_targets = 2
    _default_criterion = Quantile

    def forward(self, Z: Tensor) -> Tensor:
        lower, upper = torch.chunk(self.ffn(Z), 2, 1)
        return torch.stack(((lower + upper) / 2, upper - lower), dim=2)

    train_step = forward


class MulticlassClassificationFFN(RegressionFFN):
    """``chemprop.nn.predictors.MulticlassClassificationFFN`` (``predictors.py:271-314``): an MLP ``n_tasks * n_classes`` wide;
    ``forward`` predicts class probabilities ``[b, t, c]`` (softmax), ``train_step`` hands the logits ``[b, t, c]`` to ``CrossEntropyLoss``."""

    _default_criterion = CE

    def __init__(self, n_classes: int, n_tasks: int = 1, input_dim: int = 300, hidden_dim: int = 300, n_layers: int = 1, dropout: float = 0.0,
                 activation="relu", criterion: Optional[nn.Module] = None, task_weights: Optional[Tensor] = None):
        super().__init__(n_tasks * n_classes, input_dim, hidden_dim, n_layers, dropout, activation,
                         criterion if criterion is not None else self._default_criterion(torch.ones(n_tasks) if task_weights is None else task_weights))
        self.n_classes = n_classes
        # (predictors.py:271-314 records n_tasks AND n_classes; the base class saw their product — `cls(**hparams)` must rebuild this width)
        self.hparams.update(n_tasks=n_tasks, n_classes=n_classes)

    @property
    def n_tasks(self) -> int:
        return self.output_dim // (self.n_targets * self.n_classes)

    def forward(self, Z: Tensor) -> Tensor:
        return self.ffn(Z).reshape(Z.shape[0], -1, self.n_classes).softmax(-1)

    def train_step(self, Z: Tensor) -> Tensor:
        return self.ffn(Z).reshape(Z.shape[0], -1, self.n_classes)


class BinaryClassificationFFN(RegressionFFN):
    """``chemprop.nn.predictors.BinaryClassificationFFN`` (``predictors.py:235-247``): the same MLP; ``forward`` predicts
    probabilities (``sigmoid``), ``train_step`` hands the raw logits to ``BCELoss``."""

    _default_criterion = BCE

    def forward(self, Z: Tensor) -> Tensor:
        return self.ffn(Z).sigmoid()

    def train_step(self, Z: Tensor) -> Tensor:
        return self.ffn(Z)


class Dirichlet(MSE):
    """``chemprop.nn.metrics.DirichletLoss``: ``preds [b, t, c]`` = the Dirichlet parameters ``alpha`` against class indices — the
    expected squared error under ``Dir(alpha)`` plus ``v_kl`` times ``KL(Dir(alpha~) || Dir(1))``; no bounds."""

    kind = "dirichlet"

    def __init__(self, task_weights=1.0, v_kl: float = 0.2):
        super().__init__(task_weights)
        self.v_kl = v_kl


class BinaryDirichletFFN(RegressionFFN):
    """``chemprop.nn.predictors.BinaryDirichletFFN``: an MLP ``2 n_tasks`` wide, column ``2 j + k`` the evidence of class ``k`` of task
    ``j``; ``train_step`` hands ``alpha = softplus + 1`` as ``[b, t, 2]`` to ``DirichletLoss``, ``forward`` predicts
    ``(p_1, 2 / S) [b, t, 2]``: the probability of class 1 and the uncertainty.  :meth:`MPNN.predict` on an eval-mode model runs that
    ``forward`` inside the one-call inference head (``DMPNN_PT_DIRICHLET_BINARY``: :func:`chemprop_amd.predict.fused_predict`)."""

    n_targets = 2
    _default_criterion = Dirichlet

    def train_step(self, Z: Tensor) -> Tensor:
        return (torch.nn.functional.softplus(self.ffn(Z)) + 1).reshape(Z.shape[0], -1, 2)

    def forward(self, Z: Tensor) -> Tensor:
        alpha = self.train_step(Z)
        S = alpha.sum(-1)
        return torch.stack((alpha[..., 1] / S, 2 / S), dim=2)


class MulticlassDirichletFFN(MulticlassClassificationFFN):
    """``chemprop.nn.predictors.MulticlassDirichletFFN``: the multiclass MLP (``n_tasks * n_classes`` wide); ``train_step`` hands
    ``alpha = softplus + 1`` as ``[b, t, c]`` to ``DirichletLoss``, ``forward`` predicts ``alpha / sum(alpha) [b, t, c]``.
    :meth:`MPNN.predict` on an eval-mode model runs that ``forward`` inside the one-call inference head
    (``DMPNN_PT_DIRICHLET_MULTICLASS``: :func:`chemprop_amd.predict.fused_predict`)."""

    _default_criterion = Dirichlet

    def train_step(self, Z: Tensor) -> Tensor:
        return (torch.nn.functional.softplus(self.ffn(Z)) + 1).reshape(Z.shape[0], -1, self.n_classes)

    def forward(self, Z: Tensor) -> Tensor:
        alpha = self.train_step(Z)
        return alpha / alpha.sum(-1, keepdim=True)


class SID(MSE):
    """``chemprop.nn.metrics.SID``: the spectral information divergence of ``preds [b, t]`` = ``p`` (``SpectralFFN``) against target
    spectra, both renormalised over the finite targets; ``threshold``: a lower clamp of ``p`` (``None``: none); no bounds."""

    kind = "sid"

    def __init__(self, task_weights=1.0, threshold: Optional[float] = None):
        super().__init__(task_weights)
        self.threshold = threshold


class Wasserstein(SID):
    """``chemprop.nn.metrics.Wasserstein``: ``|cumsum(y) - cumsum(q)|`` per column, the masked columns' ``q`` inside the running sum."""

    kind = "wasserstein"


class BinaryMCC(MSE):
    """``chemprop.nn.metrics.BinaryMCCLoss``: one minus the mean over the tasks of the soft Matthews correlation of ``sigmoid(preds)``
    (``preds [b, t]``: the LOGITS of ``BinaryClassificationFFN.train_step``) against 0 / 1 targets, the four confusion sums taken over
    the whole batch per task; no bounds.  The contract and its declared deviations: ``include/dmpnn.h``."""

    kind = "mcc"


class _Exp(nn.Module):
    def forward(self, x: Tensor) -> Tensor:
        return x.exp()


class SpectralFFN(RegressionFFN):
    """``chemprop.nn.predictors.SpectralFFN``: the MLP ``n_tasks`` wide, then ``a = softplus(x)`` (``spectral_activation="softplus"``) or
    ``exp(x)`` (``"exp"``) and ``p = a / sum_j a``: a spectrum that sums to 1.  The activation is a child of ``ffn`` named
    ``spectral_activation``, as in the reference — not a layer of the MLP; ``train_step`` is ``forward``."""

    _default_criterion = SID

    def __init__(self, n_tasks: int = 1, input_dim: int = 300, hidden_dim: int = 300, n_layers: int = 1, dropout: float = 0.0,
                 activation="relu", criterion: Optional[nn.Module] = None, task_weights: Optional[Tensor] = None,
                 spectral_activation: str = "softplus"):
        super().__init__(n_tasks, input_dim, hidden_dim, n_layers, dropout, activation, criterion, task_weights)
        if spectral_activation not in ("softplus", "exp"):
            raise ValueError(f'spectral_activation must be "softplus" or "exp", got {spectral_activation!r}')
        self.hparams.update(spectral_activation=spectral_activation)
        self.ffn.add_module("spectral_activation", nn.Softplus() if spectral_activation == "softplus" else _Exp())

    def forward(self, Z: Tensor) -> Tensor:
        Y = self.ffn(Z)   # (mlp_forward runs the spectral_activation child last, as nn.Sequential does)
        return Y / Y.sum(1, keepdim=True)

    train_step = forward


def spectral_activation_of(pred) -> Optional[str]:
    """``"softplus" | "exp"`` of a ``SpectralFFN`` (this package's or the reference's, by its ``spectral_activation`` child), ``None``
    for an activation the kernels do not have."""
    act = getattr(pred.ffn, "spectral_activation", None)
    if isinstance(act, nn.Softplus) and act.beta == 1 and act.threshold == 20:
        return "softplus"
    if act is not None and type(act).__name__.lstrip("_").lower() == "exp":
        return "exp"
    return None
