"""Inference behind the block as ONE C call: ``dmpnn_predict_head`` (``include/dmpnn.h``).

``MPNN.forward`` in eval mode runs, after ``message_passing``, the aggregation (one C call), ``nn.BatchNorm1d`` and ``torch.cat``
on torch, one :class:`~chemprop_amd.nn.HipMLP` call per predictor layer and two to six torch ops of the predictor's output transform;
``validation_step`` then forms the fingerprint a second time for ``val_loss``.  :func:`fused_predict` keeps the block's forward as
it is and hands everything behind it — aggregation, eval-mode batch norm, ``X_d``, the predictor, its output transform, and the
criterion on the raw outputs when targets are given — to the library in one call: three launches for the usual model, four with
targets.  The evidential-classification heads (``BinaryDirichletFFN`` / ``MulticlassDirichletFFN`` with ``DirichletLoss``) are taken
too: ``alpha = softplus + 1`` and ``alpha / sum(alpha)`` — the binary head's ``(p_1, 2 / S)`` — are a transform of the last launch, and
``loss`` is the Dirichlet criterion on the raw outputs.  :meth:`chemprop_amd.model.MPNN.predict` is the entry a caller uses; it falls
back to the modules where this returns ``None``.
"""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple, Optional

import torch
from torch import Tensor, nn

from . import _lib, engine
from .heads import predictor_row
from .model import HeadSpec, _batch_vector_ok, _component_batch, _head_spec_key


class PredictResult(NamedTuple):
    """``preds``: what ``model(bmg, V_d, X_d)`` returns in eval mode; ``raw``: the MLP's outputs ``[n_mols, n_out]``
    (``predictor.train_step``'s values, in the MLP's column layout); ``fingerprint``: the predictor's input ``[n_mols, d]`` or
    ``None``; ``loss``: the device tensor ``[loss, n_finite]`` of the criterion on ``raw`` or ``None`` (no targets)."""
    preds: Tensor
    raw: Tensor
    fingerprint: Optional[Tensor]
    loss: Optional[Tensor]


class PredictSpec(HeadSpec):
    """What ``dmpnn_predict_head`` needs to know of the model: :class:`~chemprop_amd.model.HeadSpec` with the predictor's dropout and
    attentive aggregation allowed, plus the predictor's row of ``heads.PREDICTORS`` (``transform``: a key of ``_lib.PREDICT_TRANSFORM``,
    ``"spectral"``, ``"dirichlet_binary"`` or ``"dirichlet_multiclass"``; ``code``: the library's value for it) and the ``UnscaleTransform``
    behind it (``unscale``: the module, or ``None`` for ``nn.Identity``).  Raises ``NotImplementedError`` for what the inference head
    does not take.  ``dirichlet=True`` also takes the Dirichlet pairs ``HeadSpec`` takes for training, with an identity output transform:
    ``DMPNN_PT_DIRICHLET_BINARY`` (``(p_1, 2 / S) [n, t, 2]``) / ``_MULTICLASS`` (``alpha / sum alpha [n, t, n_classes]``); the default
    refuses them, as :func:`predict_spec` does (:func:`fused_predict` opts in).  Also holds the per-model workspace and the cached
    split images of the hidden layers' weights."""

    def __init__(self, model, dirichlet: bool = False):
        super().__init__(model, ffn_dropout=True, attentive=True)
        pred, ot = model.predictor, model.predictor.output_transform
        row = predictor_row(pred)
        if row is None:
            raise NotImplementedError(f"a predictor of a known class (got {type(pred).__name__})")
        if row.opt_in and not dirichlet:   # (the opt-in idiom of HeadSpec's attentive= / ffn_dropout=; HeadSpec took the pair)
            raise NotImplementedError(f"a Dirichlet predictor ({type(pred).__name__}): its eval-mode forward runs on the modules")
        self.transform, self.code, self.metric, self.unscale = row.transform, row.code, row.metric, None
        self.group = self.n_classes if row.classes else row.values if row.values > 1 else 0   # (the predictions' last dimension; 0: none)
        if not isinstance(ot, nn.Identity):   # (HeadSpec: an UnscaleTransform by name — identity while training, X * scale + mean in eval mode)
            if row.no_unscale is not None:    # (probabilities, an uncertainty, a spectrum that sums to 1: no mean / scale)
                raise NotImplementedError(row.no_unscale)
            mean, scale = getattr(ot, "mean", None), getattr(ot, "scale", None)
            if not (torch.is_tensor(mean) and torch.is_tensor(scale) and mean.numel() == self.n_tasks and scale.numel() == self.n_tasks):
                raise NotImplementedError(f"an UnscaleTransform with {self.n_tasks} means and scales (one per task)")
            self.unscale = ot
        self._ws: Optional[Tensor] = None
        self._wsplit: Optional[Tensor] = None
        self._wsplit_key = None
        self._sizes: dict = {}

    def out_shape(self, n_mols: int) -> tuple:
        """The shape ``model(...)`` returns in eval mode (a spectral head: ``[n_mols, n_tasks]``, one value per task)."""
        return (n_mols, self.n_tasks) + ((self.group,) if self.group else ())

    def hidden_key(self) -> tuple:
        """Identity and version of every hidden layer's weight: the split images are current while this does not change."""
        return tuple((lin.weight.data_ptr(), lin.weight._version) for lin in self.layers[:-1])


def predict_spec(model, dirichlet: bool = False) -> Optional[PredictSpec]:
    """The model's :class:`PredictSpec` (``dirichlet``: its opt-in), cached on the model under the identities ``head_loss`` keys its
    own cache on — one slot per value of ``dirichlet``: the default's refusal of a Dirichlet model does not answer the opt-in question
    (any other model has ONE spec, workspace and set of split images, whichever way it is asked for); ``None``: refused."""
    key, flag = _head_spec_key(model), bool(dirichlet)
    slots = model.__dict__.setdefault("_dmpnn_predict_spec", {})
    cached = slots.get(flag)
    if cached is not None and cached[0] == key:
        spec = cached[1]
    else:
        try:
            spec = PredictSpec(model, dirichlet=flag)
        except NotImplementedError as e:
            spec = str(e)
        slots[flag] = (key, spec)
        if not getattr(predictor_row(model.predictor), "opt_in", False):   # (the flag asks nothing of this model: one answer)
            slots[not flag] = (key, spec)
    return None if isinstance(spec, str) else spec


def _grown(buf: Optional[Tensor], nbytes: int, dev) -> Tensor:
    if buf is None or buf.device != dev or buf.numel() < nbytes:
        buf = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=dev)
    return buf


class _HeadCall:
    """One call behind the block, filled but for the workspace: what :func:`fused_predict` and :func:`fused_validate` share."""
    __slots__ = ("spec", "dev", "p", "Hv", "n_mols", "size_key", "wkey", "result", "keep")


def _fill_call(model, bmg, V_d, X_d, p, targets, weights, lt_mask, gt_mask, fingerprint: bool) -> Optional[_HeadCall]:
    """The gates of :func:`fused_predict`, the block's forward and ``p`` (a ``_lib.PredictArgs``) filled from the model and the inputs,
    with fresh outputs; ``None``: the caller takes the module path."""
    spec = predict_spec(model, dirichlet=True)
    if spec is None or model.training or torch.is_grad_enabled():
        return None
    is_list = isinstance(bmg, (list, tuple))
    bmgs = list(bmg) if is_list else [bmg]
    if is_list != (spec.blocks is not None) or len(bmgs) != spec.n_components:
        return None
    dev = spec.layers[0].weight.device
    if dev.type != "cuda":
        return None
    n_mols = len(bmgs[0])
    for b in bmgs:
        if len(b) != n_mols or b.V.device != dev or not _batch_vector_ok(b.batch, int(b.V.shape[0]), dev):
            return None
    try:
        Xd = spec.descriptors(None if X_d is None else model.X_d_transform(X_d), n_mols, dev)
    except ValueError:
        return None
    T = None
    if targets is not None:
        T = targets if (targets.dtype == torch.float32 and targets.is_contiguous()) else targets.float().contiguous()
        if T.device != dev or T.dim() != 2 or tuple(T.shape) != (n_mols, spec.n_tasks):
            return None
        if weights is not None and (weights.numel() != n_mols or weights.device != dev):
            return None
    Hv = model.message_passing(bmg, V_d)
    if is_list:
        batch = _component_batch([b.batch for b in bmgs], n_mols)
        Hv = torch.cat(list(Hv)) if len(Hv) > 1 else Hv[0]
    else:
        batch = bmg.batch
    if Hv.device != dev or Hv.dtype != torch.float32:
        return None
    Hv = engine._f32c(Hv, "H_v")
    nV, d_out = int(Hv.shape[0]), int(Hv.shape[1])
    if spec.n_components * d_out + spec.d_xd != int(spec.layers[0].in_features):
        return None

    h = p.head
    keep = spec.fill(h, nV, n_mols, d_out, batch, Hv if T is None else T, weights if T is not None else None, lt_mask if T is not None else None,
                     gt_mask if T is not None else None, lambda prm: None, bn_training=False, X_d=Xd)
    p.transform = spec.code
    if spec.unscale is not None:
        mean, scale = (t.detach().reshape(-1).to(device=dev, dtype=torch.float32).contiguous() for t in (spec.unscale.mean, spec.unscale.scale))
        p.out_mean, p.out_scale = mean.data_ptr(), scale.data_ptr()
        keep += [mean, scale]
    raw = torch.empty(n_mols, spec.n_out, dtype=torch.float32, device=dev)
    preds = torch.empty(spec.out_shape(n_mols), dtype=torch.float32, device=dev)
    h.preds, p.preds = raw.data_ptr(), preds.data_ptr()
    loss = fp = None
    if T is None:
        h.targets = None
    else:
        loss = torch.empty(2, dtype=torch.float32, device=dev)
        h.loss_out = loss.data_ptr()
        keep.append(T)
    if fingerprint:
        fp = torch.empty(n_mols, int(h.dims[0]), dtype=torch.float32, device=dev)
        p.fingerprint, p.ld_fp = fp.data_ptr(), fp.stride(0)
    c = _HeadCall()
    keep.append(batch)
    c.spec, c.dev, c.p, c.Hv, c.n_mols, c.keep = spec, dev, p, Hv, n_mols, keep
    c.size_key = (nV if spec.att is not None else 0, n_mols, d_out, Xd is not None)
    c.wkey = (spec.hidden_key(), d_out, Xd is not None)
    c.result = PredictResult(preds, raw, fp, loss)
    return c


def _run_call(c: _HeadCall, entry, arg, what: str, ws_bytes, size_tag: tuple = ()) -> PredictResult:
    """The per-model workspace and split images behind ``c.p``, then ``entry(arg, H_v, ld, stream)``; ``ws_bytes()``: what the entry
    asks of ``head.ws`` (cached per shape under ``c.size_key + size_tag``)."""
    spec, p, dev, lib = c.spec, c.p, c.dev, _lib.load()
    h = p.head
    key = c.size_key + size_tag
    sizes = spec._sizes.get(key)
    if sizes is None:
        if len(spec._sizes) > 256:
            spec._sizes.clear()
        sizes = spec._sizes[key] = (int(ws_bytes()), int(lib.dmpnn_predict_head_wsplit_bytes(C.byref(p))))
    spec._ws = _grown(spec._ws, sizes[0], dev)
    h.ws, h.ws_bytes = spec._ws.data_ptr(), spec._ws.numel()
    if sizes[1]:
        if spec._wsplit is None or spec._wsplit.device != dev or spec._wsplit.numel() < sizes[1]:
            spec._wsplit, spec._wsplit_key = _grown(None, sizes[1], dev), None
        p.wsplit, p.wsplit_bytes = spec._wsplit.data_ptr(), spec._wsplit.numel()
        p.wsplit_ready = 1 if spec._wsplit_key == c.wkey else 0
    with engine._OnDevice(dev):
        _lib.check(entry(C.byref(arg), c.Hv.data_ptr(), c.Hv.stride(0), engine._stream_ptr(dev)), what)
    if sizes[1]:
        spec._wsplit_key = c.wkey
    c.keep = None
    return c.result


def fused_predict(model, bmg, V_d=None, X_d=None, *, targets: Optional[Tensor] = None, weights: Optional[Tensor] = None,
                  lt_mask: Optional[Tensor] = None, gt_mask: Optional[Tensor] = None, fingerprint: bool = False) -> Optional[PredictResult]:
    """``model(bmg, V_d, X_d)`` in eval mode: ``model.message_passing`` as it is, then ONE ``dmpnn_predict_head`` call for everything
    behind it.  ``targets`` (with ``weights`` / ``lt_mask`` / ``gt_mask``): also the criterion on the raw outputs, chemprop's
    ``val_loss``.  ``fingerprint=True``: also the predictor's input.  A multicomponent model takes lists, as its ``forward`` does.

    ``None`` — the caller takes the module path — when the model is refused (:class:`PredictSpec`), is in training mode, grad mode
    is on, the inputs are not on the device, a batch vector is not what the kernels read, or ``X_d`` / ``targets`` / ``weights``
    are missing or misshapen.  The workspace and the split images of the hidden weights are kept per model: calls on one model belong
    on one stream.  An in-place change of a hidden weight through ``.data`` does not advance its version: clear
    ``model.__dict__["_dmpnn_predict_spec"]`` after one.  A Dirichlet model is asked for with ``PredictSpec``'s ``dirichlet=True``."""
    p = _lib.PredictArgs()
    c = _fill_call(model, bmg, V_d, X_d, p, targets, weights, lt_mask, gt_mask, fingerprint)
    if c is None:
        return None
    lib = _lib.load()
    return _run_call(c, lib.dmpnn_predict_head, p, "dmpnn_predict_head", lambda: lib.dmpnn_predict_head_ws_bytes(C.byref(p)))


def fused_validate(model, bmg, V_d=None, X_d=None, *, targets: Tensor, stats, metric_targets: Optional[Tensor] = None,
                   weights: Optional[Tensor] = None, lt_mask: Optional[Tensor] = None, gt_mask: Optional[Tensor] = None,
                   fingerprint: bool = False, ranks=None) -> Optional[PredictResult]:
    """One validation step behind the block as ONE ``dmpnn_validate_head`` call: :func:`fused_predict` with ``targets`` — the same
    kernels, the same bits — and, behind it, the batch's metric sums added into ``stats`` (a
    :class:`~chemprop_amd.metrics.MetricStats` on the model's device; at most two launches more).  ``metric_targets``: the targets the
    metrics compare the predictions with where they differ from the criterion's (unscaled against scaled).  The bounds reach the
    statistics where they reach the criterion (a bounded MSE / MAE).

    ``ranks`` (a :class:`~chemprop_amd.metrics.RankStats` on the model's device, binary heads): the call is
    ``dmpnn_validate_head_ranked`` — the same step and one launch more, which appends the batch's (score, label) rows to the epoch's
    rank buffer at ``ranks.rows``; the counter advances only after the call has returned 0.

    ``None`` under :func:`fused_predict`'s conditions, for ``stats`` / ``ranks`` on another device and for misshapen ``metric_targets``;
    ``ValueError`` for ``stats`` of another kind or shape than the model's (:meth:`MetricStats.for_model`), for ``ranks`` of another
    number of tasks and — before anything is launched — for a batch that does not fit ``ranks``."""
    if targets is None:
        raise ValueError("fused_validate: a validation step has targets")
    if ranks is not None and not ranks.fits(int(targets.shape[0])):
        raise ValueError(f"fused_validate: a batch of {int(targets.shape[0])} rows does not fit ranks ({ranks.rows} of {ranks.capacity} used)")
    vr = _lib.ValidateRankArgs() if ranks is not None else None
    v = vr.validate if ranks is not None else _lib.ValidateArgs()
    c = _fill_call(model, bmg, V_d, X_d, v.predict, targets, weights, lt_mask, gt_mask, fingerprint)
    if c is None or stats.device != c.dev or (ranks is not None and ranks.device != c.dev):
        return None
    if ranks is not None and ranks.n_tasks != c.spec.n_tasks:
        raise ValueError(f"fused_validate: ranks of {ranks.n_tasks} tasks, the model has {c.spec.n_tasks}")
    kind = c.spec.metric
    fits = (kind, c.spec.n_tasks, c.spec.n_classes if kind == "multiclass" else 0)
    if fits != (stats.kind, stats.n_tasks, stats.n_classes if kind == "multiclass" else 0):
        raise ValueError(f"fused_validate: stats of kind / tasks / classes {(stats.kind, stats.n_tasks, stats.n_classes)}, the model's are {fits}")
    if metric_targets is not None:
        M = metric_targets if metric_targets.dtype == torch.float32 else metric_targets.float()
        if M.device != c.dev or M.dim() != 2 or tuple(M.shape) != (c.n_mols, stats.n_tasks):
            return None
        if M.stride(1) != 1 or M.stride(0) < stats.n_tasks:
            M = M.contiguous()
        v.metric_targets, v.ld_mt = M.data_ptr(), max(int(M.stride(0)), stats.n_tasks)
        c.keep.append(M)
    v.metric_kind, v.threshold = _lib.METRIC[stats.kind], stats.threshold
    v.stats, v.stats_bytes = stats.stats.data_ptr(), stats.stats.numel() * 8
    lib = _lib.load()
    if ranks is None:
        return _run_call(c, lib.dmpnn_validate_head, v, "dmpnn_validate_head", lambda: lib.dmpnn_validate_head_ws_bytes(C.byref(v)), ("validate", stats.kind))
    vr.keys, vr.labels, vr.capacity, vr.row0 = ranks.keys.data_ptr(), ranks.labels.data_ptr(), ranks.capacity, ranks.rows
    r = _run_call(c, lib.dmpnn_validate_head_ranked, vr, "dmpnn_validate_head_ranked", lambda: lib.dmpnn_validate_head_ranked_ws_bytes(C.byref(vr)),
                  ("validate", stats.kind))
    ranks.rows += c.n_mols
    return r
