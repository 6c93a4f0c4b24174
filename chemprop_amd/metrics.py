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

ROC-AUC and PRC-AUC are functions of ranks, not of sums: :class:`RankStats` (below) keeps the epoch's (score, label) pairs on the
device and ranks them there at the epoch's end.
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


# ---- the epoch's rank metrics: ROC-AUC and PRC-AUC of a binary head ---------------------------------------------------------------------
RANK_MAX_ROWS = _lib.RANK_MAX_ROWS


def rank_keys(scores: Tensor, targets: Tensor) -> tuple:
    """``(keys, labels)`` of float32 ``scores`` / ``targets`` of one shape — ``k_rank_append``'s rules restated on torch ops.  ``keys``
    (int32 holding the uint32 bits): the order-preserving image of the score — ``-0.0`` becomes ``+0.0``, then sign bit set ``->
    ~bits``, else ``bits | 0x80000000`` — and 0 where the pair is not ranked.  ``labels`` (uint8): 0 negative, 1 positive (``t > 0.5``),
    2 the target is NaN / infinite, 3 the target is finite and the score is not (counted as ``n_skipped``).  Integer tests on the bits
    throughout: no denormal mode can merge or split ties."""
    b = scores.detach().float().contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    T = targets.detach().float()
    t_ok = T.isfinite()
    p_ok = (b & 0x7F800000) != 0x7F800000
    b = torch.where((b & 0x7FFFFFFF) == 0, torch.zeros_like(b), b)
    key = torch.where((b & 0x80000000) != 0, b ^ 0xFFFFFFFF, b | 0x80000000)
    ranked = t_ok & p_ok
    key = torch.where(ranked, key, torch.zeros_like(key))
    lab = torch.where(ranked, (T > 0.5).to(torch.uint8), torch.where(t_ok, torch.full_like(T, 3, dtype=torch.uint8), torch.full_like(T, 2, dtype=torch.uint8)))
    key = torch.where(key >= 1 << 31, key - (1 << 32), key).to(torch.int32)   # (the same 32 bits in int32)
    return key, lab


def rank_column(keys: np.ndarray, labels: np.ndarray) -> np.ndarray:
    """``dmpnn_rank_metrics``' 8 doubles of ONE column, restated in float64 numpy: ``n_pos, n_neg, n_skipped, n_thresholds, U2, roc,
    prc, 0``.  The five counts of every distinct key come from one sort of the distinct keys (the device counts all pairs; the
    integers are the same, the PRC sum is added in key order, not row order)."""
    keys, labels = np.asarray(keys).reshape(-1).view(np.uint32), np.asarray(labels).reshape(-1)
    out = np.zeros(8)
    ranked = labels < 2
    out[2] = float((labels == 3).sum())
    k, pos = keys[ranked], labels[ranked] == 1
    P, N = int(pos.sum()), int((~pos).sum())
    out[0], out[1] = P, N
    out[5] = out[6] = np.nan
    if k.size == 0:
        return out
    u, inv = np.unique(k, return_inverse=True)
    ep = np.bincount(inv, weights=pos, minlength=u.size).astype(np.int64)
    en = np.bincount(inv, minlength=u.size).astype(np.int64) - ep
    gp = ep[::-1].cumsum()[::-1] - ep      # positives / negatives with a strictly greater key
    gn = en[::-1].cumsum()[::-1] - en
    U2 = int((en * (2 * gp + ep)).sum())
    out[3], out[4] = u.size, U2
    if P > 0 and N > 0:
        above = (gp + gn).astype(np.float64)
        p_i = (gp + ep) / (above + ep + en)
        p_prev = np.where(above > 0, gp / np.where(above > 0, above, 1.0), 1.0)
        out[5] = U2 / (2.0 * P * N)
        out[6] = float((ep * (p_i + p_prev) * 0.5).sum()) / P
    return out


class RankStats:
    """The epoch's rank buffer of one binary model — ``keys`` (int32 holding ``uint32`` bits) and ``labels`` (uint8), ``[capacity,
    n_tasks]`` on ``device`` — and ``rows``, the molecules appended so far, counted on the host (``include/dmpnn.h``, "Epoch rank
    metrics").  ROC-AUC and PRC-AUC need every (score, label) pair of the epoch, not sums: the pairs stay on the device, and
    :meth:`compute` ranks them there by an all-pairs count and copies ``8 (n_tasks + 1)`` doubles to the host.

    ``update`` appends one batch: on device tensors it is ``dmpnn_rank_append`` (one launch), on CPU tensors :func:`rank_keys`.
    ``merge`` appends another buffer's used rows — unlike sums, ranks need every rank's rows: under ``--devices N`` this is what an
    ``all_gather`` of the buffers feeds.

    Declared deviations — restated from chemprop 2.3.1 (``BinaryAUROC`` / ``BinaryAUPRC``) and not run against it: unweighted; ``roc`` /
    ``prc`` are per-task values averaged over the tasks that have both classes, where the reference pools all tasks' pairs into one
    curve — that pooling is offered beside them as ``roc-pooled`` / ``prc-pooled``; a column without positives or without negatives
    gives NaN, not the reference's warning-and-zero; a pair whose target is finite and whose prediction is not is left out and counted
    (``n_skipped``) where the reference would rank it.  At most ``RANK_MAX_ROWS`` keys are ranked together (the cost is quadratic)."""

    def __init__(self, n_tasks: int, capacity: int, device="cpu"):
        self.n_tasks, self.capacity = int(n_tasks), int(capacity)
        if self.n_tasks < 1 or self.capacity < 0:
            raise ValueError(f"n_tasks >= 1 and capacity >= 0 (got {n_tasks}, {capacity})")
        self.keys = torch.zeros(self.capacity, self.n_tasks, dtype=torch.int32, device=device)
        self.labels = torch.full((self.capacity, self.n_tasks), 2, dtype=torch.uint8, device=device)
        self.rows = 0
        self._ws: Optional[Tensor] = None

    @classmethod
    def for_model(cls, model, capacity: int, device=None) -> "RankStats":
        """The buffer that fits ``model``'s binary predictor (a sigmoid or a binary Dirichlet head) and ``capacity`` molecules — the
        validation set's size — on the device of its parameters; ``NotImplementedError`` for every other predictor."""
        pred = model.predictor
        row = predictor_row(pred)
        if row is None or row.metric != "binary":
            raise NotImplementedError(f"rank metrics take a binary classification predictor (got {type(pred).__name__})")
        dev = device if device is not None else next(model.parameters()).device
        return cls(int(pred.n_tasks), capacity, dev)

    @property
    def device(self):
        return self.keys.device

    def reset(self) -> None:
        self.rows = 0

    def fits(self, n: int) -> bool:
        return self.rows + int(n) <= self.capacity

    def merge(self, other: "RankStats") -> None:
        if other.n_tasks != self.n_tasks:
            raise ValueError("merge: a buffer of another number of tasks")
        if not self.fits(other.rows):
            raise ValueError(f"merge: {other.rows} rows do not fit ({self.rows} of {self.capacity} used)")
        dev = self.keys.device
        self.keys[self.rows:self.rows + other.rows] = other.keys[:other.rows].to(dev)
        self.labels[self.rows:self.rows + other.rows] = other.labels[:other.rows].to(dev)
        self.rows += other.rows

    def update(self, preds: Tensor, targets: Tensor) -> None:
        """Append one batch: ``preds`` as the model returns them in eval mode (``[n, t]`` or ``[n, t, k]`` with ``k`` 1 or 2: element 0
        of a task's group is the score), ``targets [n, t]`` (NaN: missing).  ``ValueError`` when the batch does not fit or lives on
        another device."""
        n, t, dev = int(targets.shape[0]), self.n_tasks, targets.device
        if dev != self.keys.device or preds.device != dev:
            raise ValueError(f"this buffer lives on {self.keys.device}, the batch on {preds.device} / {dev}")
        if targets.dim() != 2 or int(targets.shape[1]) != t or int(preds.shape[0]) != n:
            raise ValueError(f"targets must be [n, {t}] with one row of preds each, got {tuple(targets.shape)} / {tuple(preds.shape)}")
        if not self.fits(n):
            raise ValueError(f"a batch of {n} rows does not fit ({self.rows} of {self.capacity} used)")
        if n == 0:
            return
        P, T = preds.detach().float().reshape(n, t, -1), targets.detach().float()
        group = int(P.shape[2])
        if group not in (1, 2):
            raise ValueError(f"preds must hold 1 or 2 values per task, got {tuple(preds.shape)}")
        if dev.type == "cuda":
            from . import engine

            lib = _lib.load()
            rows = lambda X: X if n > 1 and X.stride(1) == 1 and X.stride(0) >= X.shape[1] else X.contiguous()   # (views into wider tables stay views)
            P2, T = rows(P.reshape(n, -1)), rows(T)
            a = _lib.RankAppendArgs()
            a.n_mols, a.n_tasks, a.group = n, t, group
            a.preds, a.ld_p, a.targets, a.ld_t = P2.data_ptr(), int(P2.stride(0)), T.data_ptr(), int(T.stride(0))
            a.keys, a.labels, a.capacity, a.row0 = self.keys.data_ptr(), self.labels.data_ptr(), self.capacity, self.rows
            with engine._OnDevice(dev):
                _lib.check(lib.dmpnn_rank_append(C.byref(a), engine._stream_ptr(dev)), "dmpnn_rank_append")
            del P2, T
        else:
            k, l = rank_keys(P[:, :, 0], T)
            self.keys[self.rows:self.rows + n], self.labels[self.rows:self.rows + n] = k, l
        self.rows += n

    def _out(self, pooled: bool) -> np.ndarray:
        """``dmpnn_rank_metrics``' ``out`` on the host, ``[n_tasks + pooled, 8]``."""
        t, n, dev = self.n_tasks, self.rows, self.keys.device
        if dev.type != "cuda":
            K, L = self.keys[:n].numpy(), self.labels[:n].numpy()
            cols = [rank_column(K[:, j], L[:, j]) for j in range(t)]
            if pooled:
                cols.append(rank_column(K, L))
            return np.stack(cols)
        from . import engine

        lib = _lib.load()
        out = torch.empty(t + int(pooled), _lib.RANK_OUT, dtype=torch.float64, device=dev)
        a = _lib.RankArgs()
        a.keys, a.labels, a.rows, a.n_tasks, a.pooled, a.out = self.keys.data_ptr(), self.labels.data_ptr(), n, t, int(pooled), out.data_ptr()
        nb = int(lib.dmpnn_rank_metrics_ws_bytes(C.byref(a)))
        if nb:
            if self._ws is None or self._ws.device != dev or self._ws.numel() < nb:
                self._ws = torch.empty(nb, dtype=torch.uint8, device=dev)
            a.ws, a.ws_bytes = self._ws.data_ptr(), self._ws.numel()
        with engine._OnDevice(dev):
            _lib.check(lib.dmpnn_rank_metrics(C.byref(a), engine._stream_ptr(dev)), "dmpnn_rank_metrics")
        return out.cpu().numpy()   # (the ONE copy)

    def compute(self, pooled: bool = True) -> dict:
        """``roc`` / ``prc``: the mean of the per-task values over the tasks that have both classes (NaN if none); with ``pooled``
        also ``roc-pooled`` / ``prc-pooled``, all tasks' pairs ranked as one column (the reference's pooling); ``per_task``: arrays
        ``roc, prc, n_pos, n_neg, n_thresholds, n_skipped``.  On the device ONE ``dmpnn_rank_metrics`` call and one copy of ``8
        (n_tasks + pooled)`` doubles; on CPU buffers :func:`rank_column`.  ``ValueError`` when more than ``RANK_MAX_ROWS`` keys would
        be ranked together (beyond it for the pooled column alone: ``pooled=False``)."""
        together = self.rows * (self.n_tasks if pooled else 1)
        if together > RANK_MAX_ROWS:
            raise ValueError(f"{together} keys would be ranked together, the cap is RANK_MAX_ROWS = {RANK_MAX_ROWS}"
                             + (" (pooled=False ranks each task alone)" if pooled and self.rows <= RANK_MAX_ROWS else ""))
        A = self._out(bool(pooled))
        t = self.n_tasks
        per = dict(roc=A[:t, 5].copy(), prc=A[:t, 6].copy(), n_pos=A[:t, 0].copy(), n_neg=A[:t, 1].copy(), n_thresholds=A[:t, 3].copy(),
                   n_skipped=A[:t, 2].copy(), U2=A[:t, 4].copy())
        ok = (per["n_pos"] > 0) & (per["n_neg"] > 0)
        out = {"roc": float(per["roc"][ok].mean()) if ok.any() else float("nan"),
               "prc": float(per["prc"][ok].mean()) if ok.any() else float("nan"), "n_mols": self.rows, "per_task": per}
        if pooled:
            out["roc-pooled"], out["prc-pooled"] = float(A[t, 5]), float(A[t, 6])
            out["pooled"] = dict(n_pos=A[t, 0], n_neg=A[t, 1], n_thresholds=A[t, 3], n_skipped=A[t, 2], U2=A[t, 4])
        return out
