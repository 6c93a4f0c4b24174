"""``chemprop_amd.model.masked_loss`` as it stood on the commit before the head tables (``chemprop_amd/heads.py``): one function, an
``if kind in (...)`` chain — copied unchanged and never edited, so that ``tests/test_head_table.py`` can hold the per-kind functions
behind today's ``masked_loss`` to it bit for bit on whatever CPU the suite runs (the float records of
``tests/golden/head_table_parent.json`` are the bits of the CPU that wrote them).  A plain module: no fixtures."""
import math
from typing import Optional

import torch
from torch import Tensor


def masked_loss(preds: Tensor, targets: Tensor, weights: Optional[Tensor] = None, task_weights: Optional[Tensor] = None,
                lt_mask: Optional[Tensor] = None, gt_mask: Optional[Tensor] = None, kind: str = "mse", v_kl: float = 0.2, eps: float = 1e-8,
                alpha: float = 0.1, threshold: Optional[float] = None) -> Tensor:
    """``ChempropMetric.update`` + ``compute`` on one batch (``nn/metrics.py:78-127``) with the masking of
    ``MPNN.training_step`` (``models/model.py:152-156``): torch ops, differentiable — the module path's criterion."""
    mask = targets.isfinite()
    targets = targets.nan_to_num(nan=0.0)
    w = torch.ones(targets.shape[0], dtype=torch.float, device=targets.device) if weights is None else weights
    tw = 1.0 if task_weights is None else task_weights.view(1, -1)
    if kind in ("bce", "ce", "mve", "evidential", "quantile", "dirichlet", "sid", "wasserstein", "mcc"):
        lt_mask = gt_mask = None     # (only the Bounded* criteria apply the masks: metrics.py:157-177)
    if kind == "mcc":                # preds [b, t] logits (BinaryClassificationFFN.train_step): BinaryMCCLoss as include/dmpnn.h restates it
        a = w.view(-1, 1) * mask     # (the sigmoid always; 1 - p as sigmoid(-x); the mean over ALL tasks: no finite target anywhere is loss 1)
        p, q = preds.sigmoid(), (-preds).sigmoid()
        TP, FP = (a * targets * p).sum(0), (a * (1 - targets) * p).sum(0)
        TN, FN = (a * (1 - targets) * q).sum(0), (a * targets * q).sum(0)
        mcc = (TP * TN - FP * FN) / ((TP + FP) * (TP + FN) * (TN + FP) * (TN + FN) + 1e-8).sqrt()
        return 1 - (mcc * tw).sum() / targets.shape[1]
    if kind in ("sid", "wasserstein"):   # preds [b, t] = p (SpectralFFN.train_step): renormalised over the finite targets (include/dmpnn.h)
        c = preds if threshold is None else preds.clamp(min=threshold)
        q = c / (c * mask).sum(1, keepdim=True)
        if kind == "sid":            # (masked q and y filled with 1: a zero term)
            one = torch.ones_like(q)
            qm, ym = torch.where(mask, q, one), torch.where(mask, targets, one)
            L = qm * (qm / ym).log() + ym * (ym / qm).log()
        else:                        # (the running sum of q includes the masked columns; only y is 0 there)
            L = (targets.cumsum(1) - q.cumsum(1)).abs()
        return (L * w.view(-1, 1) * tw * mask).sum() / mask.sum()
    if kind == "dirichlet":          # preds [b, t, c] = alpha (the Dirichlet predictors' train_step), targets [b, t] class indices (DirichletLoss)
        y = torch.nn.functional.one_hot(targets.long(), preds.shape[-1]).to(preds.dtype)
        S = preds.sum(-1, keepdim=True)
        p = preds / S
        L_mse = ((y - p) ** 2).sum(-1) + (p * (1 - p) / (S + 1)).sum(-1)
        a_t = y + (1 - y) * preds    # (1 at the true class: the KL term leaves its evidence alone)
        S_t = a_t.sum(-1, keepdim=True)
        L_kl = (torch.lgamma(S_t).squeeze(-1) - torch.lgamma(a_t).sum(-1) - math.lgamma(preds.shape[-1])
                + ((a_t - 1) * (torch.digamma(a_t) - torch.digamma(S_t))).sum(-1))
        return ((L_mse + v_kl * L_kl) * w.view(-1, 1) * tw * mask).sum() / mask.sum()
    if kind in ("mve", "evidential", "quantile"):   # preds [b, t, 2 | 4]: what MveFFN / EvidentialFFN / QuantileFFN.train_step stack (predictors.py:173-232)
        if kind == "mve":               # MVELoss, metrics.py:203-219
            mean, var = torch.unbind(preds, dim=-1)
            L = (mean - targets) ** 2 / (2 * var) + (2 * torch.pi * var).log() / 2
        elif kind == "quantile":        # QuantileLoss, metrics.py:589-610
            mean, interval = torch.unbind(preds, dim=-1)
            bounds = torch.tensor([-0.5, 0.5], device=preds.device).view(-1, 1, 1)
            tau = torch.tensor([[alpha / 2, 1 - alpha / 2], [alpha / 2 - 1, -alpha / 2]], device=preds.device).view(2, 2, 1, 1)
            L = (tau * (targets - (mean + bounds * interval))).amax(0).sum(0)
        else:                           # EvidentialLoss, metrics.py:222-262
            mean, v, alpha, beta = torch.unbind(preds, dim=-1)
            residuals = targets - mean
            two_b_lambda = 2 * beta * (1 + v)
            L_nll = (0.5 * (torch.pi / v).log() - alpha * two_b_lambda.log() + (alpha + 0.5) * torch.log(v * residuals**2 + two_b_lambda)
                     + torch.lgamma(alpha) - torch.lgamma(alpha + 0.5))
            L = L_nll + v_kl * ((2 * v + alpha) * residuals.abs() - eps)
        return (L * w.view(-1, 1) * tw * mask).sum() / mask.sum()
    if kind == "ce":                 # preds [b, t, c] logits, targets [b, t] class indices (metrics.py:298-304)
        L = torch.nn.functional.cross_entropy(preds.transpose(1, 2), targets.long(), reduction="none")
        return (L * w.view(-1, 1) * tw * mask).sum() / mask.sum()
    if lt_mask is not None:
        preds = torch.where((preds < targets) & lt_mask, targets, preds)
    if gt_mask is not None:
        preds = torch.where((preds > targets) & gt_mask, targets, preds)
    if kind == "bce":     # nn/metrics.py:292-295 (on logits: the classification predictor's train_step, predictors.py:246-247)
        L = torch.nn.functional.binary_cross_entropy_with_logits(preds, targets, reduction="none")
    else:
        L = (preds - targets).abs() if kind == "mae" else torch.nn.functional.mse_loss(preds, targets, reduction="none")
    return (L * w.view(-1, 1) * tw * mask).sum() / mask.sum()
