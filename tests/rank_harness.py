"""The yardstick of the rank-metric tests (``tests/test_rank_stats.py``, ``tests/test_rank_stats_gpu.py``): float64 numpy references of
ROC-AUC and PRC-AUC and the inputs they are held against.  Nothing here imports the code under test.

``ref_curves``  one column, sort-based: a transcription of torchmetrics' ``_binary_clf_curve`` (sort descending, one threshold per
                distinct score, ``tps`` / ``fps`` cumulative), ``roc`` (a leading (0, 0), rates, trapezoid) and
                ``precision_recall_curve`` (reversed, the appended point recall 0 / precision 1) with ``auc(recall, precision)`` as
                chemprop 2.3.1's ``BinaryAUPRC`` forms it — restated, not run.  Also ``P``, ``N``, ``n_thresholds``, ``n_skipped`` and
                ``U2`` in exact integers from the same sort.
``ref_u2``      the integer ``U2`` again, from ALL PAIRS by numpy broadcasting (in row chunks): twice the Mann-Whitney count, ties half.
``make_inputs`` scores and targets ``[n, t]`` whose columns rotate through ten patterns (see the function).

A pair is ranked where its target and its score are both finite; a finite target with a score that is not is left out and counted
(``n_skipped`` — the declared deviation of ``include/dmpnn.h``); positive means ``t > 0.5``."""
import numpy as np

EPS = 2.0 ** -52
N_PATTERNS = 10


def bar(n_ranked: int) -> float:
    """The absolute bar on ``roc`` / ``prc``: each is a sum of at most ``n_ranked`` non-negative terms that totals at most 1, each term
    formed with a handful of roundings — ``(n_ranked + 8) 2^-52``, derived, not measured."""
    return (n_ranked + 8) * EPS


def _ranked(scores, targets):
    s32, t = np.asarray(scores, dtype=np.float32).reshape(-1), np.asarray(targets, dtype=np.float32).reshape(-1)
    t_ok = np.isfinite(t)
    ok = t_ok & np.isfinite(s32)
    return s32[ok].astype(np.float64), (t[ok] > 0.5), int((t_ok & ~ok).sum())


def ref_curves(scores_f32, targets) -> dict:
    s, y, skipped = _ranked(scores_f32, targets)
    P, N = int(y.sum()), int((~y).sum())
    out = dict(P=P, N=N, n_skipped=skipped, n_ranked=int(s.size), n_thresholds=0, U2=0, roc=float("nan"), prc=float("nan"))
    if s.size == 0:
        return out
    order = np.argsort(-s, kind="stable")
    s, y = s[order], y[order]
    distinct = np.nonzero(s[1:] != s[:-1])[0]              # (-0.0 == +0.0; two denormals differ)
    idx = np.concatenate([distinct, [s.size - 1]])
    tps = np.cumsum(y.astype(np.int64))[idx]
    fps = 1 + idx - tps
    out["n_thresholds"] = int(idx.size)
    ep, en = np.diff(np.concatenate([[0], tps])), np.diff(np.concatenate([[0], fps]))
    gp = tps - ep
    out["U2"] = int((en * (2 * gp + ep)).sum())
    if P == 0 or N == 0:
        return out
    # roc: (0, 0) in front, rates, trapezoid over fpr
    tpr, fpr = np.concatenate([[0], tps]) / float(P), np.concatenate([[0], fps]) / float(N)
    out["roc"] = float(np.sum(np.diff(fpr) * (tpr[1:] + tpr[:-1]) * 0.5))
    # precision_recall_curve: reversed, then (recall 0, precision 1); auc(recall, precision) with recall descending
    precision, recall = tps / (tps + fps).astype(np.float64), tps / float(P)
    precision, recall = np.concatenate([precision[::-1], [1.0]]), np.concatenate([recall[::-1], [0.0]])
    out["prc"] = float(-np.sum(np.diff(recall) * (precision[1:] + precision[:-1]) * 0.5))
    return out


def ref_u2(scores_f32, targets, chunk: int = 512) -> int:
    s, y, _ = _ranked(scores_f32, targets)
    pos, neg = s[y], s[~y]
    total = 0
    for a in range(0, neg.size, chunk):
        blk = neg[a:a + chunk, None]
        total += 2 * int((pos[None, :] > blk).sum()) + int((pos[None, :] == blk).sum())
    return total


def pattern_of(j: int, seed: int) -> int:
    return (j + seed) % N_PATTERNS


def make_inputs(n: int, t: int, seed: int):
    """``(scores, targets)`` float32 ``[n, t]``.  Column ``j`` follows pattern ``(j + seed) % 10``: 0 uniform scores; 1 scores quantised to
    4 levels (heavy ties); 2 all scores equal; 3 only the denormals 1e-40 and 2e-40, ``+0.0`` and ``-0.0`` (the zeros must tie, the
    denormals must not); 4 saturated 0.0 / 1.0 scores; 5 uniform with 10 % NaN targets; 6 every target NaN; 7 no positive; 8 no negative;
    9 targets exactly 0.5 (negative) or 1.  With ``n >= 4`` two predictions of the first column that is not all-NaN are made ``inf`` and
    NaN over finite targets (``n_skipped``)."""
    rng = np.random.default_rng(1000 + seed)
    S = rng.random((n, t), dtype=np.float32)
    T = (rng.random((n, t)) < 0.4).astype(np.float32)
    for j in range(t):
        p = pattern_of(j, seed)
        if p == 1:
            S[:, j] = np.floor(S[:, j] * 4) / 4
        elif p == 2:
            S[:, j] = np.float32(0.3)
        elif p == 3:
            S[:, j] = np.array([1e-40, 2e-40, 0.0, -0.0], dtype=np.float32)[rng.integers(0, 4, n)]
        elif p == 4:
            S[:, j] = (S[:, j] > 0.5).astype(np.float32)
        elif p == 5:
            T[rng.random(n) < 0.1, j] = np.nan
        elif p == 6:
            T[:, j] = np.nan
        elif p == 7:
            T[:, j] = 0.0
        elif p == 8:
            T[:, j] = 1.0
        elif p == 9:
            T[:, j] = np.where(T[:, j] > 0.5, 1.0, 0.5).astype(np.float32)
    if n >= 4:
        for j in range(t):
            if pattern_of(j, seed) != 6:
                S[1, j], S[n - 2, j] = np.inf, np.nan
                T[1, j], T[n - 2, j] = 1.0, 0.0 if pattern_of(j, seed) != 8 else 1.0
                break
    return S, T
