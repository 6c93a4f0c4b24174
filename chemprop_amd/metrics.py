"""Epoch metric statistics: the double buffer ``dmpnn_metric_stats`` / ``dmpnn_validate_head`` add a batch's sums into
(``include/dmpnn.h``, "Epoch metric statistics"), and the float64 formulas that turn it into a validation epoch's metrics.

Every metric below is a function of a few per-task sums over the (molecule, task) pairs with a finite target, and sums add across
batches (and across ranks: :meth:`MetricStats.merge` is an addition).  A validation step therefore costs one C call behind the block
(:func:`chemprop_amd.predict.fused_validate`), and the epoch ends with ONE device-to-host copy in :meth:`MetricStats.compute`.

Layout (``stats``, float64): ``[sum loss * n_finite, sum n_finite, calls, molecules]`` and then per task

``regression``  ``n, sum e^2, sum |e|, sum t, sum t^2, sum e_b^2, sum |e_b|, 0`` with ``e = p - t`` and ``e_b = e`` but 0 where
                (``lt_mask`` and ``p < t``) or (``gt_mask`` and ``p > t``); ``p`` is element 0 of the task's group of predictions
``binary``      ``n, TP, FP, TN, FN, 0, 0, 0``: predicted class ``p > threshold`` (strictly), positive target ``t > 0.5``
``multiclass``  ``n_classes^2`` confusion counts ``[target class][argmax]`` (the lowest index among equal maxima; a target outside
                ``[0, n_classes)`` is skipped like a NaN one)
``none``        the header alone (spectral heads: ``val_loss`` only)

Declared deviation — restated from chemprop 2.3.1 and not run against it: the statistics are UNWEIGHTED (validation and test run with
unit weights in the reference); ``weights`` and the criterion's ``task_weights`` go into ``val_loss`` only.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Optional

import numpy as np
import torch
from torch import Tensor

from . import _lib
from .heads import predictor_row

KINDS = tuple(_lib.METRIC)
HEADER = _lib.METRIC_HEADER


def per_task(kind: str, n_classes: int = 0) -> int:
    """Doubles per task of a kind (``dmpnn_metric_stats_doubles`` less the header, over ``n_tasks``)."""
    if kind not in _lib.METRIC:
        raise ValueError(f"kind must be one of {KINDS}, got {kind!r}")
    if kind == "multiclass":
        if not 2 <= int(n_classes) <= _lib.METRIC_MAX_CLASSES:
            raise ValueError(f"multiclass statistics take 2..{_lib.METRIC_MAX_CLASSES} classes, got {n_classes}")
        return int(n_classes) ** 2
    return 0 if kind == "none" else 8


def kind_of_model(model) -> tuple:
    """``(kind, n_tasks, n_classes)`` of a model's predictor, told from its class (this package's mirrors and the reference's, by MRO
    name — its row of ``heads.PREDICTORS``, which :class:`~chemprop_amd.predict.PredictSpec` reads its transform from)."""
    pred = model.predictor
    row = predictor_row(pred)
    if row is None:
        raise NotImplementedError(f"a predictor of a known class (got {type(pred).__name__})")
    return row.metric, int(pred.n_tasks), int(pred.n_classes) if row.metric == "multiclass" else 0


def _zero_safe(num: np.ndarray, den: np.ndarray) -> np.ndarray:
    """``num / den`` with 0 where ``den == 0``."""
    out = np.zeros_like(num, dtype=np.float64)
    np.divide(num, den, out=out, where=den != 0)
    return out


class MetricStats:
    """The epoch's statistics of one model: ``stats`` (float64, on ``device``), zero at the start of an epoch.

    ``update`` adds one batch: on device tensors it is ``dmpnn_metric_stats`` (two launches, bitwise reproducible), on CPU tensors a
    torch float64 restatement that writes the same layout.  ``merge`` adds another buffer of the same shape (another rank's: one
    ``all_reduce`` of ``stats`` does the same).  ``compute`` copies the buffer to the host once and applies the formulas."""

    def __init__(self, kind: str, n_tasks: int, n_classes: int = 0, threshold: float = 0.5, device="cpu"):
        self.kind, self.n_tasks, self.n_classes, self.threshold = kind, int(n_tasks), int(n_classes), float(threshold)
        self.per = per_task(kind, n_classes)
        if self.n_tasks < 0 or not math.isfinite(self.threshold):
            raise ValueError(f"n_tasks >= 0 and a finite threshold (got {n_tasks}, {threshold})")
        self.stats = torch.zeros(HEADER + (self.n_tasks * self.per if kind != "none" else 0), dtype=torch.float64, device=device)
        self._ws: Optional[Tensor] = None

    @classmethod
    def for_model(cls, model, threshold: float = 0.5, device=None) -> "MetricStats":
        """The statistics that fit ``model``'s predictor (:func:`kind_of_model`), on the device of its parameters."""
        kind, n_tasks, n_classes = kind_of_model(model)
        dev = device if device is not None else next(model.parameters()).device
        return cls(kind, n_tasks, n_classes, threshold, dev)

    @property
    def device(self):
        return self.stats.device

    def reset(self) -> None:
        self.stats.zero_()

    def merge(self, other: "MetricStats") -> None:
        if (other.kind, other.n_tasks, other.n_classes) != (self.kind, self.n_tasks, self.n_classes):
            raise ValueError("merge: statistics of another kind or shape")
        self.stats += other.stats.to(self.stats.device)

    # ---- one batch ---------------------------------------------------------------------------------------------------------------------
    def _rows(self, preds: Tensor, targets: Tensor) -> tuple:
        """``preds`` as ``[n, t, group | n_classes]`` and ``targets [n, t]`` in float32, shapes checked."""
        n, t = int(targets.shape[0]), self.n_tasks
        if targets.dim() != 2 or int(targets.shape[1]) != t:
            raise ValueError(f"targets must be [n, {t}], got {tuple(targets.shape)}")
        if preds.shape[0] != n or preds.device != targets.device:
            raise ValueError("preds and targets: one row per molecule, on one device")
        P = preds.detach().float().reshape(n, t, -1) if t else preds.detach().float().reshape(n, 0, 1)
        width = int(P.shape[2])
        if self.kind == "multiclass" and width != self.n_classes:
            raise ValueError(f"multiclass preds must be [n, {t}, {self.n_classes}], got {tuple(preds.shape)}")
        if self.kind in ("regression", "binary") and width not in (1, 2, 4):
            raise ValueError(f"preds must hold 1, 2 or 4 values per task, got {tuple(preds.shape)}")
        return P, targets.detach().float()

    def update(self, preds: Tensor, targets: Tensor, lt_mask: Optional[Tensor] = None, gt_mask: Optional[Tensor] = None,
               loss: Optional[Tensor] = None) -> None:
        """Add one batch: ``preds`` as the model returns them in eval mode (``[n, t]`` or ``[n, t, k]``: element 0 of a task's group
        is the prediction; multiclass: the class scores), ``targets [n, t]`` (NaN: missing), the bounds of a regression batch, and
        ``loss = [loss, n_finite]`` of the batch (``PredictResult.loss``).  ``n == 0`` leaves the buffer as it was."""
        n, dev = int(targets.shape[0]), targets.device
        if dev != self.stats.device:
            raise ValueError(f"these statistics live on {self.stats.device}, the batch on {dev}")
        if n == 0:
            return
        P, T = (None, None) if self.kind == "none" else self._rows(preds, targets)
        if dev.type == "cuda":
            self._device_update(P, T, n, lt_mask, gt_mask, loss)
        else:
            self._cpu_update(P, T, n, lt_mask, gt_mask, loss)

    def _device_update(self, P, T, n: int, lt_mask, gt_mask, loss) -> None:
        from . import engine

        lib, dev = _lib.load(), self.stats.device
        a = _lib.MetricArgs()
        a.kind, a.n_mols, a.n_tasks, a.n_classes, a.threshold = _lib.METRIC[self.kind], n, self.n_tasks, self.n_classes, self.threshold
        keep = []
        if P is not None:
            rows = lambda X: X if n > 1 and X.stride(1) == 1 and X.stride(0) >= X.shape[1] else X.contiguous()   # (views into wider tables stay views)
            P2, T = rows(P.reshape(n, -1)), rows(T)
            a.group = int(P.shape[2]) if self.kind != "multiclass" else 1
            a.preds, a.ld_p, a.targets, a.ld_t = P2.data_ptr(), int(P2.stride(0)), T.data_ptr(), int(T.stride(0))
            keep += [P2, T]
            if self.kind == "regression":
                for name, m in (("lt_mask", lt_mask), ("gt_mask", gt_mask)):
                    if m is not None:
                        m8 = m.to(device=dev, dtype=torch.uint8).reshape(n, self.n_tasks).contiguous()
                        setattr(a, name, m8.data_ptr())
                        keep.append(m8)
        if loss is not None:
            l2 = loss.detach().to(device=dev, dtype=torch.float32).reshape(2).contiguous()
            a.loss = l2.data_ptr()
            keep.append(l2)
        a.stats, a.stats_bytes = self.stats.data_ptr(), self.stats.numel() * 8
        nb = int(lib.dmpnn_metric_stats_ws_bytes(C.byref(a)))
        if nb:
            if self._ws is None or self._ws.device != dev or self._ws.numel() < nb:
                self._ws = torch.empty(nb, dtype=torch.uint8, device=dev)
            a.ws, a.ws_bytes = self._ws.data_ptr(), self._ws.numel()
        with engine._OnDevice(dev):
            _lib.check(lib.dmpnn_metric_stats(C.byref(a), engine._stream_ptr(dev)), "dmpnn_metric_stats")
        del keep

    def _cpu_update(self, P, T, n: int, lt_mask, gt_mask, loss) -> None:
        """The stage restated on torch ops in float64: the same layout, the same conventions."""
        s = self.stats
        if loss is not None:
            l, nf = float(loss[0]), float(loss[1])
            if nf > 0:
                s[0] += l * nf
                s[1] += nf
        s[2] += 1
        s[3] += n
        if self.kind == "none" or self.n_tasks == 0:
            return
        body = s[HEADER:].view(self.n_tasks, self.per)
        m = T.isfinite()
        if self.kind == "multiclass":
            nc = self.n_classes
            cls = T.nan_to_num(nan=-1.0, posinf=-1.0, neginf=-1.0).trunc()
            ok = m & (cls >= 0) & (cls < nc)
            idx = torch.arange(nc).expand_as(P)
            am = torch.where(P == P.max(-1, keepdim=True).values, idx, torch.full_like(idx, nc)).min(-1).values   # (lowest index among equal maxima)
            cell = cls.long().clamp(0, nc - 1) * nc + am.clamp(max=nc - 1)
            for j in range(self.n_tasks):
                body[j] += torch.bincount(cell[:, j][ok[:, j]], minlength=nc * nc).double()
            return
        p0 = P[:, :, 0]
        md = m.double()
        if self.kind == "binary":
            pp, tp = p0 > torch.tensor(self.threshold, dtype=torch.float32), T > 0.5
            cols = (md, (m & pp & tp).double(), (m & pp & ~tp).double(), (m & ~pp & ~tp).double(), (m & ~pp & tp).double())
        else:
            y = torch.where(m, T, torch.zeros_like(T)).double()
            e = torch.where(m, p0.double() - y, torch.zeros_like(y))
            clip = torch.zeros_like(m)
            if lt_mask is not None:
                clip = clip | (lt_mask.bool().reshape(m.shape) & (p0 < T))
            if gt_mask is not None:
                clip = clip | (gt_mask.bool().reshape(m.shape) & (p0 > T))
            eb = torch.where(clip, torch.zeros_like(e), e)
            cols = (md, e * e, e.abs(), y, y * y, eb * eb, eb.abs())
        for k, c in enumerate(cols):
            body[:, k] += c.sum(0)
        body[:, len(cols):] = 0   # (the reserved slots)

    # ---- the epoch's metrics -----------------------------------------------------------------------------------------------------------
    def compute(self) -> dict:
        """ONE copy of the buffer to the host, then float64 formulas.  Every kind: ``val_loss = stats[0] / stats[1]`` (the count-weighted
        mean of the batches' losses; NaN without a finite target), ``n_calls``, ``n_mols`` and ``per_task`` (arrays ``[n_tasks]``).

        ``regression`` — ``mse``, ``mae``, ``rmse = sqrt(mse)`` and ``bounded-mse`` / ``bounded-mae`` / ``bounded-rmse`` are POOLED over
        tasks as ``ChempropMetric.compute`` pools them (``nn/metrics.py:78-127``: the sum over all finite pairs over their count;
        ``BoundedMixin``, ``:157-163``, for the bounded forms).  ``r2 = 1 - sum e^2 / (sum t^2 - (sum t)^2 / n)`` per task
        (torchmetrics' ``R2Score``: ``1 - SS_res / SS_tot``), averaged over the tasks with ``n >= 2`` and a nonzero denominator (its
        ``uniform_average``; NaN when no task qualifies).  Deviation: the one-pass ``SS_tot`` cancels where ``mean^2 / var`` is large —
        the relative error is about ``2^-53 n mean^2 / var``.

        ``binary`` — per task ``accuracy = (TP + TN) / n``, ``f1 = 2 TP / (2 TP + FP + FN)``, ``binary-mcc = (TP TN - FP FN) /
        sqrt((TP + FP)(TP + FN)(TN + FP)(TN + FN))`` (torchmetrics' ``BinaryAccuracy`` / ``BinaryF1Score`` / ``BinaryMatthewsCorrCoef``
        at ``threshold``), each 0 where its denominator is 0, averaged over ALL tasks.  Deviation: the reference pools the classification
        metrics of a multi-task model over tasks; the per-task values are in ``per_task``.

        ``multiclass`` — from the confusion matrix ``C`` of a task: ``accuracy = tr C / sum C``; ``multiclass-mcc = (c s - sum_k p_k
        t_k) / sqrt((s^2 - sum p_k^2)(s^2 - sum t_k^2))`` with ``c = tr C``, ``s = sum C``, ``t_k`` / ``p_k`` the row / column sums
        (torchmetrics' ``MulticlassMatthewsCorrCoef``), 0 where a denominator is 0, averaged over all tasks.

        Unweighted throughout (the module docstring's declared deviation)."""
        s = self.stats.detach().cpu().numpy().astype(np.float64)
        out = {"val_loss": float(s[0] / s[1]) if s[1] > 0 else float("nan"), "n_calls": int(s[2]), "n_mols": int(s[3]), "per_task": {}}
        if self.kind == "none" or self.n_tasks == 0:
            return out
        A = s[HEADER:].reshape(self.n_tasks, self.per)
        per = out["per_task"]
        nan = float("nan")
        if self.kind == "regression":
            n, se2, sae, st, st2, sb2, sab = (A[:, k] for k in range(7))
            N = n.sum()
            for name, q in (("mse", se2), ("mae", sae), ("bounded-mse", sb2), ("bounded-mae", sab)):
                out[name] = float(q.sum() / N) if N > 0 else nan
                per[name] = np.where(n > 0, _zero_safe(q, n), np.nan)
            out["rmse"], out["bounded-rmse"] = math.sqrt(out["mse"]) if N > 0 else nan, math.sqrt(out["bounded-mse"]) if N > 0 else nan
            per["rmse"], per["bounded-rmse"] = np.sqrt(per["mse"]), np.sqrt(per["bounded-mse"])
            den = st2 - _zero_safe(st * st, n)
            ok = (n >= 2) & (den != 0)
            per["r2"] = np.where(ok, 1.0 - _zero_safe(se2, den), np.nan)
            out["r2"] = float(per["r2"][ok].mean()) if ok.any() else nan
            per["n"] = n
        elif self.kind == "binary":
            n, TP, FP, TN, FN = (A[:, k] for k in range(5))
            per["accuracy"] = _zero_safe(TP + TN, n)
            per["f1"] = _zero_safe(2 * TP, 2 * TP + FP + FN)
            per["binary-mcc"] = _zero_safe(TP * TN - FP * FN, np.sqrt((TP + FP) * (TP + FN) * (TN + FP) * (TN + FN)))
            per["n"] = n
            for name in ("accuracy", "f1", "binary-mcc"):
                out[name] = float(per[name].mean())
        else:
            Cm = A.reshape(self.n_tasks, self.n_classes, self.n_classes)
            tot, c = Cm.sum((1, 2)), np.trace(Cm, axis1=1, axis2=2)
            tk, pk = Cm.sum(2), Cm.sum(1)
            per["accuracy"] = _zero_safe(c, tot)
            per["multiclass-mcc"] = _zero_safe(c * tot - (pk * tk).sum(1), np.sqrt((tot * tot - (pk * pk).sum(1)) * (tot * tot - (tk * tk).sum(1))))
            per["n"] = tot
            for name in ("accuracy", "multiclass-mcc"):
                out[name] = float(per[name].mean())
        return out
