"""Shared helpers of the metric-statistics tests (``dmpnn_metric_stats`` / ``chemprop_amd.metrics``): no fixtures, no pytest settings —
a plain module.

``make_inputs`` builds one batch with every element the conventions are about: 10 % NaN targets and one all-NaN column, predictions
exactly at the threshold and exactly equal to their target, both bounds, two equal maxima, targets outside the class range and
fractional ones.  ``ref_stats`` restates the statistics buffer in numpy float64 straight from the raw arrays — independently of
``MetricStats`` — and ``wrong`` switches ONE deliberate mistake on, for the tests that show the comparison would catch it.
``direct_metrics`` computes the epoch metrics from the raw arrays WITHOUT the sums: two-pass R2, MCC as a correlation coefficient.
"""
import numpy as np
import torch

HEADER = 4
WRONG = {"regression": "ignore_masks", "binary": "ge_threshold", "multiclass": "argmax_high"}


def per_task(kind, nc=0):
    return nc * nc if kind == "multiclass" else (0 if kind == "none" else 8)


def make_inputs(kind: str, n: int, t: int, width: int, seed: int = 0, thr: float = 0.5) -> dict:
    """``P [n, t, width]`` (``width``: the group of a regression / binary head, the classes of a multiclass one), ``T [n, t]`` float32
    CPU tensors, and for regression ``lt`` / ``gt`` bool masks."""
    g = torch.Generator().manual_seed(1000 + seed)
    r = lambda *s: torch.rand(*s, generator=g)
    out = {}
    if kind == "multiclass":
        P = torch.randn(n, t, width, generator=g)
        a = torch.randint(0, width - 1, (n, t), generator=g)
        b = a + 1 + (r(n, t) * (width - 1 - a)).long()   # a < b < width
        tie = r(n, t) < 0.15
        top = P.max(-1).values + 1
        for idx in (a, b):   # two equal maxima at a < b
            P.scatter_(2, idx.unsqueeze(-1), torch.where(tie, top, P.gather(2, idx.unsqueeze(-1)).squeeze(-1)).unsqueeze(-1))
        T = torch.randint(0, width, (n, t), generator=g).float()
        u = r(n, t)
        T = torch.where(u < 0.05, torch.full_like(T, float(width)), T)          # out of range above
        T = torch.where((u >= 0.05) & (u < 0.10), torch.full_like(T, -1.0), T)   # and below
        T = torch.where((u >= 0.10) & (u < 0.15), T + 0.7, T)                    # fractional: truncated (width - 1 + 0.7 stays inside)
        T = torch.where((u >= 0.15) & (u < 0.18), torch.full_like(T, -0.5), T)   # truncates to class 0
    elif kind == "binary":
        P = r(n, t, width)
        P[:, :, 0] = torch.where(r(n, t) < 0.15, torch.full((n, t), thr), P[:, :, 0])   # exactly at the threshold
        T = r(n, t).round()
    else:
        P = torch.randn(n, t, width, generator=g)
        T = 2 * torch.randn(n, t, generator=g) + 1
        P[:, :, 0] = torch.where(r(n, t) < 0.1, T, P[:, :, 0])                        # p == t
        out.update(lt=r(n, t) < 0.3, gt=r(n, t) < 0.3)
    T = torch.where(r(n, t) < 0.1, torch.full_like(T, float("nan")), T)
    if t >= 3:
        T[:, 1] = float("nan")   # one all-NaN column
    out.update(P=P.float().contiguous(), T=T.float().contiguous())
    return out


def ref_stats(kind, P, T, lt=None, gt=None, thr=0.5, nc=0, loss=None, wrong=None, abs_terms=False) -> np.ndarray:
    """The buffer one ``update`` leaves from zero, in numpy float64.  ``abs_terms``: every sum over the absolute values of its terms
    (the scale of the summation bound).  ``wrong``: ``ignore_masks | ge_threshold | argmax_high``."""
    P, T = np.asarray(P, np.float32), np.asarray(T, np.float32)
    n, t = T.shape
    per = per_task(kind, nc)
    s = np.zeros(HEADER + t * per)
    if n == 0:
        return s
    if loss is not None and float(loss[1]) > 0:
        s[0], s[1] = float(loss[0]) * float(loss[1]), float(loss[1])
        if abs_terms:
            s[0] = abs(s[0])
    s[2], s[3] = 1, n
    if kind == "none" or t == 0:
        return s
    body = s[HEADER:].reshape(t, per)
    P = P.reshape(n, t, -1)
    m = np.isfinite(T)
    p, y = P[:, :, 0].astype(np.float64), np.where(m, T, 0).astype(np.float64)
    if kind == "regression":
        e = np.where(m, p - y, 0.0)
        clip = np.zeros_like(m)
        if wrong != "ignore_masks":
            if lt is not None:
                clip |= np.asarray(lt, bool) & (p < y)
            if gt is not None:
                clip |= np.asarray(gt, bool) & (p > y)
        eb = np.where(clip, 0.0, e)
        cols = (m.astype(np.float64), e * e, np.abs(e), np.abs(y) if abs_terms else y, y * y, eb * eb, np.abs(eb))
        for k, c in enumerate(cols):
            body[:, k] = c.sum(0)
    elif kind == "binary":
        th = np.float32(thr)
        pp = (P[:, :, 0] >= th) if wrong == "ge_threshold" else (P[:, :, 0] > th)
        tp = np.where(m, T, 0) > 0.5
        for k, c in enumerate((m, m & pp & tp, m & pp & ~tp, m & ~pp & ~tp, m & ~pp & tp)):
            body[:, k] = c.sum(0)
    else:
        cls = np.trunc(np.where(m, T, -1.0))
        ok = m & (cls >= 0) & (cls < nc)
        am = (nc - 1 - np.argmax(P[:, :, ::-1], -1)) if wrong == "argmax_high" else np.argmax(P, -1)   # (numpy: the first maximum)
        for j in range(t):
            for i in np.nonzero(ok[:, j])[0]:
                body[j, int(cls[i, j]) * nc + int(am[i, j])] += 1
    return s


def _safe(num, den):
    return num / den if den != 0 else 0.0


def direct_metrics(kind, P, T, lt=None, gt=None, thr=0.5, nc=0) -> dict:
    """The epoch metrics straight from the raw arrays (no sums of squares, no confusion matrix)."""
    P, T = np.asarray(P, np.float32), np.asarray(T, np.float32)
    n, t = T.shape
    P = P.reshape(n, t, -1)
    m = np.isfinite(T)
    out = {}
    if kind == "regression":
        p, y = P[:, :, 0].astype(np.float64), T.astype(np.float64)
        clip = np.zeros_like(m)
        if lt is not None:
            clip |= np.asarray(lt, bool) & (p < y)
        if gt is not None:
            clip |= np.asarray(gt, bool) & (p > y)
        pb = np.where(clip, y, p)
        out["mse"], out["mae"] = float(np.mean((p - y)[m] ** 2)), float(np.mean(np.abs(p - y)[m]))
        out["bounded-mse"], out["bounded-mae"] = float(np.mean((pb - y)[m] ** 2)), float(np.mean(np.abs(pb - y)[m]))
        out["rmse"], out["bounded-rmse"] = out["mse"] ** 0.5, out["bounded-mse"] ** 0.5
        r2 = []
        for j in range(t):
            yj, pj = y[m[:, j], j], p[m[:, j], j]
            if yj.size >= 2 and np.sum((yj - yj.mean()) ** 2) != 0:
                r2.append(1.0 - np.sum((pj - yj) ** 2) / np.sum((yj - yj.mean()) ** 2))   # two passes
        out["r2"] = float(np.mean(r2)) if r2 else float("nan")
    elif kind == "binary":
        acc, f1, mcc = [], [], []
        for j in range(t):
            pr, tg = (P[m[:, j], j, 0] > np.float32(thr)).astype(np.float64), (T[m[:, j], j] > 0.5).astype(np.float64)
            acc.append(float(np.mean(pr == tg)) if pr.size else 0.0)
            prec, rec = _safe(np.sum(pr * tg), np.sum(pr)), _safe(np.sum(pr * tg), np.sum(tg))
            f1.append(_safe(2 * prec * rec, prec + rec))
            mcc.append(float(np.corrcoef(pr, tg)[0, 1]) if pr.size and pr.std() > 0 and tg.std() > 0 else 0.0)   # MCC IS Pearson's r of the two indicators
        out.update({"accuracy": float(np.mean(acc)), "f1": float(np.mean(f1)), "binary-mcc": float(np.mean(mcc))})
    else:
        acc, mcc = [], []
        for j in range(t):
            cls = np.trunc(np.where(m[:, j], T[:, j], -1.0))
            ok = m[:, j] & (cls >= 0) & (cls < nc)
            c, a = cls[ok].astype(int), np.argmax(P[ok, j], -1)
            acc.append(float(np.mean(c == a)) if c.size else 0.0)
            X, Y = np.eye(nc)[a], np.eye(nc)[c]   # Gorodkin's R_K: cov(X, Y) / sqrt(cov(X, X) cov(Y, Y)) over the one-hot rows
            cov = lambda A, B: float(np.sum((A - A.mean(0)) * (B - B.mean(0)))) if A.size else 0.0
            den = (cov(X, X) * cov(Y, Y)) ** 0.5
            mcc.append(cov(X, Y) / den if den > 1e-12 else 0.0)
        out.update({"accuracy": float(np.mean(acc)), "multiclass-mcc": float(np.mean(mcc))})
    return out


def close(a: float, b: float, rel: float = 1e-9) -> bool:
    return (a != a and b != b) or abs(a - b) <= rel * max(abs(a), abs(b), 1e-300) or abs(a - b) <= 1e-15
