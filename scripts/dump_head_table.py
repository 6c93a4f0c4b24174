"""What the package says about every prediction head, as one JSON document: ``python scripts/dump_head_table.py TREE OUT.json``.

``records()`` asks the ``chemprop_amd`` it can import — ``main`` puts ``TREE`` and ``TREE/tests`` in front of ``sys.path`` first — for
``HeadSpec`` / ``PredictSpec`` / ``metrics.kind_of_model`` on every pair of predictor and criterion (values or the complete refusal),
``criterion_kind`` on classes that merely carry the reference's names, the message a model with two faults gets, and ``masked_loss``
with its gradient for every kind as ``float.hex()``.  ``tests/golden/head_table_parent.json`` is this script's output on the commit
before the head tables (``chemprop_amd/heads.py``) went in; ``tests/test_head_table.py`` holds the working tree to it, string by string (the floats: to a few ulp, and bit for bit to the parent's function).
"""
import json
import sys

import torch
from torch import nn

D = 8   # the block's width and the predictors' input_dim


def _outcome(fn):
    try:
        return fn()
    except NotImplementedError as e:
        return str(e)


def _head_spec(model, M):
    s = M.HeadSpec(model)
    return [s.kind, s.bounded, s.n_tasks, s.n_out, s.n_classes, s.n_targets, s.spectral_act, s.spectral_threshold, s.v_kl, s.eps, s.q_alpha]


def _predict_spec(model, flag):
    from chemprop_amd.predict import PredictSpec

    s = PredictSpec(model, dirichlet=flag)
    return [s.transform, list(s.out_shape(5)), s.unscale is None]


def outcomes(model) -> dict:
    from chemprop_amd import metrics
    from chemprop_amd import model as M

    return {"head": _outcome(lambda: _head_spec(model, M)), "predict": _outcome(lambda: _predict_spec(model, False)),
            "predict_dirichlet": _outcome(lambda: _predict_spec(model, True)), "metric": _outcome(lambda: list(metrics.kind_of_model(model)))}


def _mpnn(pred, agg=None, **kw):
    from chemprop_amd import agg as cagg
    from chemprop_amd.model import MPNN
    from chemprop_amd.nn import BondMessagePassing

    return MPNN(BondMessagePassing(d_h=D), cagg.MeanAggregation() if agg is None else agg, pred, **kw)


def grid() -> dict:
    import step_harness as sh

    out = {}
    for p in sh.HEADS:
        for c in sh.HEADS:
            out[f"{p}|{c}"] = outcomes(_mpnn(sh.make_predictor(p, c, sh.StepCase(head=p).tasks, D, (6,), "relu")))
    return out


def _named(name, *bases, **attrs):
    return type(name, bases or (nn.Module,), attrs)


def stand_ins() -> dict:
    """Criteria that are nothing but the reference's class names, alone, on the predictor of their kind and on ``RegressionFFN``."""
    from chemprop_amd import model as M

    mixin = type("BoundedMixin", (), {})
    mse, mae, quantile, sid = _named("MSE"), _named("MAE"), _named("QuantileLoss"), _named("SID")
    crits = [mse, mae, _named("BoundedMSE", mixin, mse), _named("BoundedMAE", mixin, mae), _named("RMSE", mse), _named("MVELoss"),
             _named("EvidentialLoss"), quantile, _named("PointQuantileLoss", quantile), _named("BCELoss"), _named("CrossEntropyLoss"),
             _named("DirichletLoss"), sid, _named("Wasserstein", sid), _named("BinaryMCCLoss"), _named("MulticlassMCCLoss"), _named("Huber")]
    kw = dict(n_tasks=2, input_dim=D, hidden_dim=6)
    home = {"mve": [M.MveFFN], "evidential": [M.EvidentialFFN], "quantile": [M.QuantileFFN], "bce": [M.BinaryClassificationFFN],
            "mcc": [M.BinaryClassificationFFN], "ce": [M.MulticlassClassificationFFN], "dirichlet": [M.BinaryDirichletFFN, M.MulticlassDirichletFFN],
            "sid": [M.SpectralFFN], "wasserstein": [M.SpectralFFN]}
    out = {}
    for cls in crits:
        kind = M.criterion_kind(cls())
        rec = {"criterion_kind": list(kind)}
        for p in home.get(kind[0], []) + [M.RegressionFFN] + ([M.MulticlassClassificationFFN] if cls.__name__ == "MulticlassMCCLoss" else []):
            pred = p(3, criterion=cls(), **kw) if p.__name__.startswith("Multiclass") else p(criterion=cls(), **kw)
            rec[p.__name__] = outcomes(_mpnn(pred))
        out[cls.__name__] = rec
    return out


def two_faults() -> dict:
    """Models with two faults at once, one for every adjacent pair of refusals in ``HeadSpec.__init__`` and ``PredictSpec.__init__``: the
    message that wins is the one tested first."""
    from chemprop_amd import model as M

    kw = dict(n_tasks=2, input_dim=D, hidden_dim=6)
    mcmcc, unknown = _named("MulticlassMCCLoss"), _named("Huber")

    def unscale(n):
        t = _named("UnscaleTransform")()
        t.register_buffer("mean", torch.zeros(1, n)), t.register_buffer("scale", torch.ones(1, n))
        return t

    def with_(pred, **attrs):
        for k, v in attrs.items():
            setattr(pred, k, v)
        return pred

    def spectral(act=None, **k):
        pred = M.SpectralFFN(**{**kw, **k})
        if act is not None:
            pred.ffn.spectral_activation = act
        return pred

    models = {
        "aggregation|prelu": _mpnn(M.RegressionFFN(activation="prelu", **kw), agg=nn.Identity()),
        "prelu|multiclass-mcc": _mpnn(M.RegressionFFN(activation="prelu", criterion=mcmcc(), **kw)),
        "dropout|transform": _mpnn(with_(M.RegressionFFN(dropout=0.1, **kw), output_transform=nn.Tanh())),
        "transform|multiclass-mcc": _mpnn(with_(M.RegressionFFN(criterion=mcmcc(), **kw), output_transform=nn.Tanh())),
        "multiclass-mcc|dirichlet-predictor": _mpnn(M.BinaryDirichletFFN(criterion=mcmcc(), **kw)),
        "unknown|spectral-activation": _mpnn(spectral(nn.Tanh(), criterion=unknown())),
        "dirichlet-criterion|spectral-activation": _mpnn(spectral(nn.Tanh(), criterion=M.Dirichlet(1.0))),
        "dirichlet-predictor|spectral-criterion": _mpnn(M.BinaryDirichletFFN(criterion=M.SID(1.0), **kw)),
        "dirichlet-criterion|spectral-predictor": _mpnn(spectral(criterion=M.Dirichlet(1.0))),
        "spectral-criterion|chunked-predictor": _mpnn(M.MveFFN(criterion=M.Wasserstein(1.0), **kw)),
        "spectral-predictor|mcc": _mpnn(spectral(criterion=M.BinaryMCC(1.0))),
        "mcc|chunked-predictor": _mpnn(M.EvidentialFFN(criterion=M.BinaryMCC(1.0), **kw)),
        "mcc|class-dimension": _mpnn(M.MulticlassClassificationFFN(3, criterion=M.BinaryMCC(1.0), **kw)),
        "spectral-activation|threshold": _mpnn(spectral(nn.Tanh(), criterion=M.SID(1.0, threshold=-1.0))),
        "threshold|n-targets": _mpnn(with_(spectral(criterion=M.SID(1.0, threshold=float("inf"))), n_targets=2)),
        "n-targets|class-dimension": _mpnn(with_(M.RegressionFFN(criterion=M.MVE(1.0), **kw), n_classes=3)),
        "chunked-criterion|class-dimension": _mpnn(M.MulticlassClassificationFFN(3, criterion=M.Quantile(1.0), **kw)),
        "class-dimension|width": _mpnn(with_(M.RegressionFFN(criterion=M.CE(1.0), n_tasks=3, input_dim=D, hidden_dim=6), n_classes=1)),
        "width|batch-norm": with_(_mpnn(with_(M.MulticlassClassificationFFN(3, **kw), n_classes=4), batch_norm=True), bn=nn.BatchNorm1d(D, momentum=None)),
        "dirichlet-opt-in|transform": _mpnn(with_(M.BinaryDirichletFFN(**kw), output_transform=unscale(2))),
        "spectral|unscale": _mpnn(with_(spectral(), output_transform=unscale(2))),
        "classification|unscale-width": _mpnn(with_(M.BinaryClassificationFFN(**kw), output_transform=unscale(5))),
        "multiclass|unscale": _mpnn(with_(M.MulticlassClassificationFFN(3, **kw), output_transform=unscale(2))),
        "unscale-width": _mpnn(with_(M.MveFFN(**kw), output_transform=unscale(5))),
        "unscale": _mpnn(with_(M.QuantileFFN(**kw), output_transform=unscale(2))),
    }
    return {k: outcomes(m) for k, m in models.items()}


def losses(masked_loss=None) -> dict:
    """``masked_loss`` (the package's, or the one given) and its gradient w.r.t. ``preds`` for every kind, in float32 and float64, as
    ``float.hex()``."""
    from chemprop_amd import _lib
    from chemprop_amd import model as M
    from chemprop_amd.ffn import MLP

    t, kw = 4, dict(n_tasks=4, input_dim=D, hidden_dim=6)
    preds_of = {"mse": M.RegressionFFN, "mae": M.RegressionFFN, "bce": M.BinaryClassificationFFN, "mcc": M.BinaryClassificationFFN,
                "ce": M.MulticlassClassificationFFN, "mve": M.MveFFN, "evidential": M.EvidentialFFN, "quantile": M.QuantileFFN,
                "dirichlet": M.MulticlassDirichletFFN, "sid": M.SpectralFFN, "wasserstein": M.SpectralFFN}
    out = {}
    forward, MLP.forward = MLP.forward, nn.Sequential.forward   # (the mirror MLP runs on the device only: it IS an nn.Sequential)
    try:
        for kind in _lib.LOSS:
            for dtype in (torch.float32, torch.float64):
                gen = torch.Generator().manual_seed(11)
                torch.manual_seed(5)
                cls = preds_of[kind]
                pred = (cls(3, **kw) if cls.__name__.startswith("Multiclass") else cls(**kw)).to(dtype)
                Z = torch.randn(6, D, generator=gen, dtype=torch.float64).to(dtype)
                if kind in ("ce", "dirichlet"):
                    T = torch.randint(0, 3, (6, t), generator=gen).to(dtype)
                elif kind in ("bce", "mcc"):
                    T = (torch.rand(6, t, generator=gen) < 0.5).to(dtype)
                elif kind in ("sid", "wasserstein"):
                    T = (0.05 + torch.rand(6, t, generator=gen, dtype=torch.float64)).to(dtype)
                else:
                    T = torch.randn(6, t, generator=gen, dtype=torch.float64).to(dtype)
                T[torch.arange(3), torch.arange(3)] = float("nan")   # one NaN in each of three columns,
                T[:, 3] = float("nan")                               # and one column without a finite target
                w = (0.5 + torch.rand(6, generator=gen)).to(dtype)
                tw = (0.5 + torch.rand(t, generator=gen)).to(dtype)
                lt, gt = torch.rand(6, t, generator=gen) < 0.4, torch.rand(6, t, generator=gen) < 0.4
                # (1e-3 lies under every p of these four tasks; 0.3 lies over some: the clamp bites)
                for threshold in ((None, 1e-3, 0.3) if kind in ("sid", "wasserstein") else (None,)):
                    P = pred.train_step(Z).detach().requires_grad_(True)
                    extra = dict(lt_mask=lt, gt_mask=gt) if kind in ("mse", "mae") else {}
                    loss = (masked_loss or M.masked_loss)(P, T, w, tw, kind=kind, v_kl=0.3, eps=1e-6, alpha=0.2, threshold=threshold, **extra)
                    loss.backward()
                    name = f"{kind}|{str(dtype).split('.')[1]}" + ("" if threshold is None else "|threshold" if threshold == 1e-3 else f"|threshold{threshold}")
                    out[name] = {"loss": float(loss.detach()).hex(), "grad": [float(g).hex() for g in P.grad.double().reshape(-1)]}
    finally:
        MLP.forward = forward
    return out


def records() -> dict:
    from chemprop_amd import model as M

    return {"grid": grid(), "stand_ins": stand_ins(), "two_faults": two_faults(), "masked_loss": losses(), "model_all": list(M.__all__)}


def main(tree: str, out: str) -> None:
    sys.path[:0] = [tree, tree + "/tests"]
    with open(out, "w") as f:
        json.dump(records(), f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main(*sys.argv[1:3])
