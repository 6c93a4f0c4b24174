"""``fused_validate`` / ``MPNN.validate`` on the MI355X: one validation step behind the block as ONE ``dmpnn_validate_head`` call, on the tiny
models of ``tests/test_dirichlet_predict_gpu.py`` (17 molecules, ``d_h`` 16, hidden 12) — a regression head behind an ``UnscaleTransform``
(with both bounds), MVE, binary, 3-class, binary Dirichlet and spectral (statistics of kind ``none``) heads, one variant each with ``X_d``,
attentive aggregation and two components, and a head wider than ``DMPNN_PREDICT_MAX_OUT``.

Conditions: ``preds`` / ``raw`` / ``loss`` / ``fingerprint`` bit-equal to ``fused_predict``'s on the same inputs; ``stats`` bit-equal to
``MetricStats.update(result.preds, ..., loss=result.loss)`` from a zeroed buffer; the launches of ``fused_predict`` with targets plus at
most 2; a three-batch epoch's ``compute()`` equal to the metrics computed directly from the concatenated fused predictions
(``metric_harness.direct_metrics``; 1e-9 relative, ``tests/test_metric_stats.py``'s bar); ``metric_targets`` honoured; ``MPNN.validate`` on a
model the inference head refuses (a PReLU predictor) gives the same dictionary."""
import numpy as np
import pytest
import torch

import metric_harness as mh
from chemprop_amd import _lib
from predict_harness import same_bits

pytestmark = pytest.mark.gpu
N_MOLS, D_H, HIDDEN, D_XD = 17, 16, 12, 8


class UnscaleTransform(torch.nn.Module):
    """``chemprop.nn.transforms.UnscaleTransform`` restated: the identity while training, ``X * scale + mean`` in eval mode."""

    def __init__(self, mean, scale):
        super().__init__()
        self.register_buffer("mean", mean.reshape(1, -1))
        self.register_buffer("scale", scale.reshape(1, -1))

    def forward(self, X):
        return X if self.training else X * self.scale + self.mean

    def transform_variance(self, var):
        return var if self.training else var * self.scale ** 2


# head -> (metric kind, tasks, classes)
HEADS = {"regression": ("regression", 3, 0), "mve": ("regression", 2, 0), "binary": ("binary", 3, 0), "multiclass": ("multiclass", 2, 3),
         "dirichlet-binary": ("binary", 2, 0), "spectral": ("none", 5, 0), "wide": ("regression", 65, 0)}
CASES = [(h, None) for h in HEADS] + [("regression", "xd"), ("binary", "attentive"), ("multiclass", "two-component")]
IDS = [h + ("-" + v if v else "") for h, v in CASES]


def _model(head, variant, dev, activation="tanh"):
    from chemprop_amd import agg as cagg
    from chemprop_amd import model as cm
    from chemprop_amd.nn import BondMessagePassing, MulticomponentMessagePassing

    torch.manual_seed(11)
    n_comp = 2 if variant == "two-component" else 1
    blocks = [BondMessagePassing(d_h=D_H, depth=2) for _ in range(n_comp)]
    mp = MulticomponentMessagePassing(blocks, n_comp) if n_comp > 1 else blocks[0]
    _, t, nc = HEADS[head]
    tw = 0.5 + torch.rand(t, generator=torch.Generator().manual_seed(2))
    kw = dict(n_tasks=t, input_dim=n_comp * D_H + (D_XD if variant == "xd" else 0), hidden_dim=HIDDEN, activation=activation)
    pred = {"regression": lambda: cm.RegressionFFN(criterion=cm.MSE(tw), **kw), "wide": lambda: cm.RegressionFFN(criterion=cm.MAE(tw), **kw),
            "mve": lambda: cm.MveFFN(criterion=cm.MVE(tw), **kw), "binary": lambda: cm.BinaryClassificationFFN(criterion=cm.BCE(tw), **kw),
            "multiclass": lambda: cm.MulticlassClassificationFFN(nc, criterion=cm.CE(tw), **kw),
            "dirichlet-binary": lambda: cm.BinaryDirichletFFN(criterion=cm.Dirichlet(tw, v_kl=0.35), **kw),
            "spectral": lambda: cm.SpectralFFN(criterion=cm.SID(tw), **kw)}[head]()
    if head in ("regression", "mve"):
        g = torch.Generator().manual_seed(4)
        pred.output_transform = UnscaleTransform(torch.randn(t, generator=g), 0.5 + torch.rand(t, generator=g))
    ag = cagg.AttentiveAggregation(output_size=D_H) if variant == "attentive" else cagg.MeanAggregation()
    model = (cm.MulticomponentMPNN if n_comp > 1 else cm.MPNN)(mp, ag, pred, batch_norm=True).to(dev).eval()
    with torch.no_grad():
        model.bn.weight.uniform_(0.5, 1.5), model.bn.bias.uniform_(-0.5, 0.5)
        model.bn.running_mean.uniform_(-0.1, 0.1), model.bn.running_var.uniform_(0.5, 2.0)
    return model


def _batch(head, variant, seed, dev):
    """One validation batch: the graphs, ``X_d``, targets with 20 % missing, weights, and the bounds of the regression head."""
    from chemprop_amd import synth

    kind, t, nc = HEADS[head]
    multi = variant == "two-component"
    bmgs = [synth.random_batch(N_MOLS, "qm9", seed=21 + 7 * seed + c) for c in range(2 if multi else 1)]
    for b in bmgs:
        b.to(dev)
    g = torch.Generator().manual_seed(100 + seed)
    if head == "spectral":
        T = torch.rand(N_MOLS, t, generator=g) + 0.05
    elif kind == "regression":
        T = torch.randn(N_MOLS, t, generator=g)
    else:
        T = torch.randint(0, max(nc, 2), (N_MOLS, t), generator=g).float()
    T[torch.rand(N_MOLS, t, generator=g) < 0.2] = float("nan")
    kw = dict(targets=T.to(dev), weights=(0.5 + torch.rand(N_MOLS, generator=g)).to(dev))
    if head == "regression":
        kw.update(lt_mask=(torch.rand(N_MOLS, t, generator=g) < 0.3).to(dev), gt_mask=(torch.rand(N_MOLS, t, generator=g) < 0.3).to(dev))
    if variant == "xd":
        kw["X_d"] = torch.randn(N_MOLS, D_XD, generator=g).to(dev)
    return (bmgs if multi else bmgs[0]), kw


class _FixedBlock:
    """The block's output computed once per batch: every path reads THIS tensor — the block is not part of the comparison."""

    def __init__(self, model, bmg):
        with torch.no_grad():
            out = model.message_passing(bmg, None)
        self.model, self.out = model, out

    def __enter__(self):
        self.model.message_passing.forward = lambda *a, **k: self.out

    def __exit__(self, *exc):
        del self.model.message_passing.forward


def _result_dict(r):
    return dict(preds=r.preds, raw=r.raw, loss=r.loss, fingerprint=r.fingerprint)


def _stats_kw(head, kw):
    return {k: kw[k] for k in ("lt_mask", "gt_mask") if k in kw}


@pytest.mark.parametrize("head,variant", CASES, ids=IDS)
def test_fused_validate_is_fused_predict_plus_the_statistics(head, variant, gpu_device):
    from chemprop_amd.metrics import MetricStats
    from chemprop_amd.predict import fused_predict, fused_validate

    dev, lib = gpu_device, _lib.load()
    kind, t, nc = HEADS[head]
    model = _model(head, variant, dev)
    stats = MetricStats.for_model(model)
    assert (stats.kind, stats.n_tasks, stats.n_classes, stats.device.type) == (kind, t, nc, "cuda")
    epoch, preds_all, T_all, masks_all, losses = MetricStats.for_model(model), [], [], [], []
    with torch.no_grad():
        for seed in range(3):
            bmg, kw = _batch(head, variant, seed, dev)
            with _FixedBlock(model, bmg):
                fused_predict(model, bmg, fingerprint=True, **kw)
                ref = fused_predict(model, bmg, fingerprint=True, **kw)   # (the split images are ready now)
                n_pred = int(lib.dmpnn_last_launch_count())
                stats.reset()
                got = fused_validate(model, bmg, stats=stats, fingerprint=True, **kw)
                n_val = int(lib.dmpnn_last_launch_count())
                assert ref is not None and got is not None
                torch.cuda.synchronize()
                assert same_bits(_result_dict(got), _result_dict(ref)) == [], (seed, same_bits(_result_dict(got), _result_dict(ref)))
                print(f"VALIDATE {head}-{variant} batch {seed}: launches predict {n_pred} validate {n_val}")
                assert n_val == n_pred + (1 if kind == "none" else 2)   # (the stage: the column reduction and the finish; `none`: the finish)
                again = MetricStats.for_model(model)
                again.update(got.preds, kw["targets"], loss=got.loss, **_stats_kw(head, kw))
                assert torch.equal(stats.stats.view(torch.int64), again.stats.view(torch.int64)), seed
                assert float(stats.stats[2]) == 1 and float(stats.stats[3]) == N_MOLS and float(stats.stats[1]) == float(got.loss[1])
                # the epoch: the same batches accumulated by further calls (MPNN.validate: the entry a caller uses)
                r = model.validate(bmg, kw["targets"], epoch, None, kw.get("X_d"), **{k: v for k, v in kw.items() if k not in ("targets", "X_d")})
                assert int(lib.dmpnn_last_launch_count()) == n_val and torch.equal(r.preds, got.preds)
            preds_all.append(got.preds.cpu()), T_all.append(kw["targets"].cpu()), losses.append(got.loss.cpu().double())
            masks_all.append(tuple(kw[k].cpu() for k in ("lt_mask", "gt_mask")) if "lt_mask" in kw else None)
    torch.cuda.synchronize()
    out = epoch.compute()
    L = torch.stack(losses)
    assert out["n_calls"] == 3 and out["n_mols"] == 3 * N_MOLS
    assert mh.close(out["val_loss"], float((L[:, 0] * L[:, 1]).sum() / L[:, 1].sum()), 1e-12)
    if kind == "none":
        assert out["per_task"] == {} and epoch.stats.numel() == 4
        return
    P, T = torch.cat(preds_all).numpy(), torch.cat(T_all).numpy()
    lt, gt = (torch.cat([m[i] for m in masks_all]).numpy() for i in (0, 1)) if masks_all[0] is not None else (None, None)
    ref = mh.direct_metrics(kind, P.reshape(3 * N_MOLS, t, -1), T, lt, gt, nc=nc)
    for k, v in ref.items():
        print(f"VALIDATE {head}-{variant} epoch {k}: stats {out[k]!r} direct {v!r}")
        assert mh.close(out[k], v), (k, out[k], v)
    if head == "regression":
        assert out["bounded-mse"] < out["mse"]   # (the bounds reached the statistics)


def test_metric_targets_are_honoured_and_misfit_statistics_are_refused(gpu_device):
    from chemprop_amd.metrics import MetricStats
    from chemprop_amd.predict import fused_validate

    dev = gpu_device
    model = _model("regression", None, dev)
    bmg, kw = _batch("regression", None, 0, dev)
    M = (3 * kw["targets"] + 1).contiguous()   # (the metrics' targets unscaled, the criterion's scaled)
    M[0, 0], M[1, 0] = float("nan"), 0.25    # (its own missing entries)
    stats, plain = MetricStats.for_model(model), MetricStats.for_model(model)
    with torch.no_grad(), _FixedBlock(model, bmg):
        got = fused_validate(model, bmg, stats=stats, metric_targets=M, **kw)
        ref = fused_validate(model, bmg, stats=plain, **kw)
        wide = torch.full((N_MOLS, 7), 9.0, device=dev)
        wide[:, :3] = M
        viewed = MetricStats.for_model(model)
        fused_validate(model, bmg, stats=viewed, metric_targets=wide[:, :3], **kw)   # (a view: ld_mt > n_tasks)
    assert same_bits(dict(preds=got.preds, raw=got.raw, loss=got.loss), dict(preds=ref.preds, raw=ref.raw, loss=ref.loss)) == []   # (the criterion saw `targets`)
    want = MetricStats.for_model(model)
    want.update(got.preds, M, kw["lt_mask"], kw["gt_mask"], loss=got.loss)
    assert torch.equal(stats.stats.view(torch.int64), want.stats.view(torch.int64))
    assert torch.equal(viewed.stats.view(torch.int64), want.stats.view(torch.int64))
    assert not torch.equal(stats.stats, plain.stats) and float(stats.stats[1]) == float(plain.stats[1])
    with torch.no_grad():
        assert fused_validate(model, bmg, stats=MetricStats.for_model(model, device="cpu"), **kw) is None        # statistics on another device
        assert fused_validate(model, bmg, stats=MetricStats.for_model(model), metric_targets=M[:, :2], **kw) is None
        with pytest.raises(ValueError):
            fused_validate(model, bmg, stats=MetricStats("binary", 3, device=dev), **kw)
        with pytest.raises(ValueError):
            fused_validate(model, bmg, stats=MetricStats("regression", 2, device=dev), **kw)


@pytest.mark.parametrize("head", ["regression", "binary", "multiclass"])
def test_validate_on_a_model_the_inference_head_refuses(head, gpu_device):
    """A PReLU predictor: ``PredictSpec`` refuses it, ``MPNN.validate`` forms the fingerprint once on the modules and ``stats.update`` adds
    the sums — the same dictionary as the statistics of the module path's own predictions on the CPU."""
    from chemprop_amd.metrics import MetricStats
    from chemprop_amd.predict import predict_spec

    dev, lib = gpu_device, _lib.load()
    kind, t, nc = HEADS[head]
    model = _model(head, None, dev, activation="prelu")
    assert predict_spec(model, dirichlet=True) is None
    epoch, cpu = MetricStats.for_model(model), MetricStats(kind, t, nc)
    losses = []
    for seed in range(3):
        bmg, kw = _batch(head, None, seed, dev)
        T = kw.pop("targets")
        with _FixedBlock(model, bmg):
            r = model.validate(bmg, T, epoch, **kw)
            with torch.no_grad():
                mod = model(bmg)
                l = model.loss(bmg, T, kw["weights"], kw.get("lt_mask"), kw.get("gt_mask"))
        assert torch.equal(r.preds, mod) and r.fingerprint is None and not r.preds.requires_grad
        assert abs(float(r.loss[0]) - float(l)) <= 1e-6 * abs(float(l)) and float(r.loss[1]) == float(T.isfinite().sum())
        cpu.update(mod.cpu(), T.cpu(), *(kw[k].cpu() for k in ("lt_mask", "gt_mask") if k in kw), loss=r.loss.cpu())
        losses.append(r.loss.cpu().double())
    got, want = epoch.compute(), cpu.compute()
    assert got["n_calls"] == 3 and got["n_mols"] == 3 * N_MOLS
    for k, v in want.items():
        if k != "per_task":
            print(f"VALIDATE prelu-{head} {k}: device {got[k]!r} cpu {v!r}")
            assert mh.close(got[k], v), (k, got[k], v)
    if kind != "regression":
        assert np.array_equal(epoch.stats.cpu().numpy(), cpu.stats.numpy())   # (counts, and the header's products in the same order: exact)
