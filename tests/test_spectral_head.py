"""Spectral heads (``SpectralFFN`` with ``SID`` / ``Wasserstein``) without a GPU: the contract of ``include/dmpnn.h`` ("The spectral
criteria") restated op by op in torch — ``spectral_p`` / ``spectral_criterion``, which the GPU files of this feature import as their
float64 reference and float32 yardstick — against the mirrors of ``chemprop_amd.model``, closed forms worked by hand, and what
``HeadSpec`` / ``PredictSpec`` / ``_lib`` make of such a model.

The restatement forms ``exp`` as ``exp(x - max_row x)``: the same ``p`` in exact arithmetic (the header declares that the kernels do
so), and finite in float32 where ``exp(x)`` alone overflows.
"""
import ctypes as C
import re
from pathlib import Path

import pytest
import torch

from chemprop_amd import _lib
from chemprop_amd import agg as cagg
from chemprop_amd.model import (MPNN, MSE, SID, HeadSpec, RegressionFFN, SpectralFFN, Wasserstein, criterion_kind, criterion_loss,
                                masked_loss)
from chemprop_amd.nn import BondMessagePassing

F = torch.nn.functional
ROOT = Path(__file__).resolve().parents[1]


# ---- the contract, op by op ----------------------------------------------------------------------------------------------------------
def spectral_p(x, act="softplus"):
    """``SpectralFFN.forward`` on the raw outputs ``x [B, t]``: ``a / sum_j a``."""
    a = F.softplus(x) if act == "softplus" else (x - x.detach().amax(1, keepdim=True)).exp()
    return a / a.sum(1, keepdim=True)


def spectral_loss_of_p(kind, p, T, w, tw, thr=None):
    """Both criteria on ``p``: clamp, renormalise over the finite targets, ``sum L w_i tw_j m / sum m``."""
    m = T.isfinite()
    y = torch.where(m, T, torch.zeros_like(T))
    c = p if thr is None else p.clamp(min=thr)
    q = c / torch.where(m, c, torch.zeros_like(c)).sum(1, keepdim=True)
    if kind == "sid":
        one = torch.ones_like(q)
        qm, ym = torch.where(m, q, one), torch.where(m, y, one)   # (masked q and y filled with 1)
        # q log(q / y) + y log(y / q), written as (q - y) (log q - log y): the same number (held to 1e-14 in float64 by
        # test_the_sid_term_is_the_contracts_formula), but float32 autograd gets through it where q is tiny — the quotient's own
        # derivative y / q**2 overflows float32 below q ~ 1e-19, the product form's 1 / q only below 3e-39
        L = (qm - ym) * (qm.log() - ym.log())
    else:
        assert kind == "wasserstein", kind
        L = (y.cumsum(1) - q.cumsum(1)).abs()                       # (the running sum of q includes the masked columns)
    return (L * w.view(-1, 1) * tw.view(1, -1) * m).sum() / m.sum()   # (a product, not a select: a row without targets is NaN * 0)


def spectral_criterion(kind, x, T, w, tw, act="softplus", thr=None):
    return spectral_loss_of_p(kind, spectral_p(x, act), T, w, tw, thr)


def spectral_targets(B, t, missing, seed):
    """Strictly positive target spectra ``[B, t]`` (float32), renormalised over their finite entries.  ``missing``: ``none``; ``some``
    (20 %, every row keeps a finite entry); ``first`` / ``last`` / ``task`` (column 0 / t - 1 / t // 2 in every row); ``all``."""
    g = torch.Generator().manual_seed(9000 + seed)
    Y = 0.05 + torch.rand(B, t, generator=g, dtype=torch.float64)
    gone = torch.zeros(B, t, dtype=torch.bool)
    if missing == "some" and t > 1:
        gone = torch.rand(B, t, generator=g) < 0.2
        gone[torch.arange(B), torch.arange(B) % t] = False
    elif missing in ("first", "last", "task"):
        assert t > 1
        gone[:, dict(first=0, last=t - 1, task=t // 2)[missing]] = True
    elif missing == "all":
        gone[:] = True
    else:
        assert missing in ("none", "some"), missing
    Y = Y / torch.where(gone, torch.zeros_like(Y), Y).sum(1, keepdim=True).clamp(min=1e-300)
    Y[gone] = float("nan")
    return Y.float()


def _model(t=7, act="softplus", crit=None, hidden=11, n_layers=1, d_h=8):
    torch.manual_seed(3)
    mp = BondMessagePassing(d_h=d_h, depth=2, activation="tanh")
    pred = SpectralFFN(n_tasks=t, input_dim=d_h, hidden_dim=hidden, n_layers=n_layers, activation="tanh", criterion=crit,
                       spectral_activation=act)
    return MPNN(mp, cagg.MeanAggregation(), pred, batch_norm=True)


def _inputs(B=6, t=7, seed=0, missing="some"):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, t, generator=g, dtype=torch.float64)
    T = spectral_targets(B, t, missing, seed).double()
    # (weights that float32 holds exactly: the criterion modules keep task_weights as a float32 buffer)
    return x, T, (0.5 + torch.rand(B, generator=g)).double(), (0.5 + torch.rand(t, generator=g)).double()


# ---- the mirrors against the restatement ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("act", ["softplus", "exp"])
def test_mirror_forward_is_train_step_is_p(act, monkeypatch):
    import chemprop_amd.ffn as cffn

    # (the MLP mirror runs on the HIP kernels: here its layers are restated with F.linear, on the CPU in float64)
    def cpu_layers(blocks, seq, X):
        H = blocks[0][-1](X)
        for b in blocks[1:]:
            H = b[2](b[1](b[0](H)))
        return H

    monkeypatch.setattr(cffn, "_mlp_forward", cpu_layers)
    pred = _model(act=act).predictor.double().eval()
    Z = torch.randn(5, 8, dtype=torch.float64, generator=torch.Generator().manual_seed(1))
    blocks = [m for n, m in pred.ffn.named_children() if n != "spectral_activation"]
    x = blocks[1][2](torch.tanh(blocks[0][0](Z)))
    want = spectral_p(x, act).detach()
    for got in (pred(Z).detach(), pred.train_step(Z).detach()):
        assert got.shape == (5, 7) and float((got - want).abs().max()) <= 1e-14 * float(want.abs().max())
    assert float((pred(Z).sum(1) - 1).abs().max()) <= 1e-14
    assert SpectralFFN.train_step is SpectralFFN.forward


@pytest.mark.parametrize("kind", ["sid", "wasserstein"])
@pytest.mark.parametrize("thr", [None, 0.07])
@pytest.mark.parametrize("missing", ["none", "some", "first", "last"])
def test_masked_loss_is_the_restatement(kind, thr, missing):
    x, T, w, tw = _inputs(missing=missing)
    p = spectral_p(x).requires_grad_()
    got = masked_loss(p, T, w, tw, kind=kind, threshold=thr)
    want = spectral_loss_of_p(kind, p, T, w, tw, thr)
    assert abs(float(got) - float(want)) <= 1e-14 * abs(float(want))
    crit = (SID if kind == "sid" else Wasserstein)(tw, threshold=thr).double()
    for v in (criterion_loss(crit, p, T, w), crit(p, T, weights=w)):
        assert abs(float(v) - float(want)) <= 1e-14 * abs(float(want))
    (gg,), (gw,) = torch.autograd.grad(got, p), torch.autograd.grad(want, p)
    assert float((gg - gw).abs().max()) <= 1e-14 * float(gw.abs().max())


def test_the_sid_term_is_the_contracts_formula():
    """The restatement's ``(q - y)(log q - log y)`` against the header's ``q log(q / y) + y log(y / q)``, loss and gradient, float64."""
    for missing in ("none", "some"):
        x, T, w, tw = _inputs(B=9, t=33, missing=missing)
        x.requires_grad_()
        m = T.isfinite()
        p = spectral_p(x)
        q = p / (p * m).sum(1, keepdim=True)
        one = torch.ones_like(q)
        qm, ym = torch.where(m, q, one), torch.where(m, T, one)
        want = ((qm * (qm / ym).log() + ym * (ym / qm).log()) * w.view(-1, 1) * tw.view(1, -1) * m).sum() / m.sum()
        got = spectral_criterion("sid", x, T, w, tw)
        assert abs(float(got) - float(want)) <= 1e-14 * abs(float(want))
        (gg,), (gw,) = torch.autograd.grad(got, x, retain_graph=True), torch.autograd.grad(want, x)
        assert float((gg - gw).abs().max()) <= 1e-14 * float(gw.abs().max())


def test_masked_columns_get_a_gradient_from_wasserstein_and_none_from_sid():
    x, T, w, tw = _inputs(missing="task")
    x.requires_grad_()
    col = T.shape[1] // 2
    (g,) = torch.autograd.grad(spectral_criterion("wasserstein", x, T, w, tw), x)
    assert float(g[:, col].abs().min()) > 1e-4
    (g,) = torch.autograd.grad(spectral_criterion("sid", x, T, w, tw), x)
    assert float(g[:, col].abs().max()) <= 1e-15 and float(g.abs().max()) > 1e-3


def test_edges_no_target_and_a_row_without_targets():
    x, T, w, tw = _inputs(missing="all")
    for kind in ("sid", "wasserstein"):
        assert bool(torch.isnan(spectral_criterion(kind, x, T, w, tw)))
    x, T, w, tw = _inputs(missing="none")
    T[2] = float("nan")
    assert bool(torch.isnan(spectral_criterion("wasserstein", x, T, w, tw)))   # (the reference's own; the kernels declare NaN for SID too)


# ---- closed forms ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["sid", "wasserstein"])
@pytest.mark.parametrize("act", ["softplus", "exp"])
def test_one_task_is_loss_zero_and_gradient_zero(kind, act):
    x = torch.tensor([[0.3], [-2.0], [5.0]], dtype=torch.float64, requires_grad=True)
    loss = spectral_criterion(kind, x, torch.ones(3, 1, dtype=torch.float64), torch.tensor([1.0, 2.0, 0.5]).double(), torch.tensor([1.5]).double(), act)
    (g,) = torch.autograd.grad(loss, x)
    assert float(loss) == 0.0 and float(g.abs().max()) == 0.0


def test_wasserstein_of_two_tasks_by_hand():
    """``t = 2``, no missing target: ``q = p``, ``D_1 = y_1 - p_1``, ``D_2 = 0``: ``L = tw_1 |y_1 - p_1|``; with ``exp``, ``p_1 =
    sigmoid(x_1 - x_2)`` and ``dL/dx_1 = -sign(D_1) tw_1 p_1 (1 - p_1) = -dL/dx_2``."""
    x = torch.tensor([[0.4, -0.3], [-1.0, 0.5]], dtype=torch.float64, requires_grad=True)
    T = torch.tensor([[0.25, 0.75], [0.6, 0.4]], dtype=torch.float64)
    w, tw = torch.tensor([2.0, 0.5]).double(), torch.tensor([1.5, 3.0]).double()
    loss = spectral_criterion("wasserstein", x, T, w, tw, "exp")
    p1 = torch.sigmoid(x[:, 0] - x[:, 1]).detach()
    D1 = T[:, 0] - p1
    want = float((w * 1.5 * D1.abs()).sum() / 4)
    assert abs(float(loss) - want) <= 1e-15
    (g,) = torch.autograd.grad(loss, x)
    g1 = -torch.sign(D1) * 1.5 * p1 * (1 - p1) * w / 4
    assert float((g[:, 0] - g1).abs().max()) <= 1e-15 and float((g[:, 1] + g1).abs().max()) <= 1e-15
    # one target missing: q_1 = 1, D_1 = y_1 - 1 = 0 (y renormalised over the finite entries), and the masked column's q_2 = p_2 / p_1
    # only enters D_2, which the mask drops: loss 0
    T2 = torch.tensor([[1.0, float("nan")], [1.0, float("nan")]], dtype=torch.float64)
    assert float(spectral_criterion("wasserstein", x, T2, w, tw, "exp")) == 0.0


# ---- HeadSpec / PredictSpec / _lib -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("crit_cls,kind", [(SID, "sid"), (Wasserstein, "wasserstein")])
@pytest.mark.parametrize("act", ["softplus", "exp"])
def test_headspec_accepts_the_two_pairs(crit_cls, kind, act):
    model = _model(t=7, act=act, crit=crit_cls(torch.ones(7), threshold=0.01))
    spec = HeadSpec(model)
    assert (spec.kind, spec.n_tasks, spec.n_out, spec.n_classes, spec.n_targets) == (kind, 7, 7, 0, 1)
    assert (spec.spectral_act, spec.spectral_threshold) == (act, 0.01)
    assert len(spec.layers) == 2 and all(isinstance(l, torch.nn.Linear) for l in spec.layers)   # (the spectral_activation child is no layer)
    assert list(dict(model.predictor.ffn.named_children()))[-1] == "spectral_activation"
    assert criterion_kind(model.predictor.criterion) == (kind, False)
    assert HeadSpec(_model(crit=crit_cls(torch.ones(7)))).spectral_threshold == 0.0
    h = _lib.HeadArgs()
    T = torch.zeros(4, 7)
    spec.fill(h, 9, 4, 8, torch.zeros(9, dtype=torch.int64), T, None, None, None, lambda p: None)
    assert (h.loss, h.spectral_act, h.n_classes, h.n_layers, h.dims[2]) == (_lib.LOSS[kind], _lib.SPECTRAL_ACT[act], 0, 2, 7)
    assert abs(h.spectral_threshold - 0.01) < 1e-9


def test_default_criterion_and_reference_class_names():
    assert _model().predictor.criterion.kind == "sid"

    class Wasserstein_(torch.nn.Module):   # (the reference's classes are told by MRO name)
        pass

    Wasserstein_.__name__ = "Wasserstein"
    assert criterion_kind(Wasserstein_()) == ("wasserstein", False)
    Wasserstein_.__name__ = "SID"
    assert criterion_kind(Wasserstein_()) == ("sid", False)


def test_headspec_refuses_mixed_pairs_and_an_unknown_activation():
    with pytest.raises(NotImplementedError, match="SpectralFFN with a criterion other than SID"):
        HeadSpec(_model(crit=MSE(torch.ones(7))))
    torch.manual_seed(0)
    reg = MPNN(BondMessagePassing(d_h=8, depth=2), cagg.MeanAggregation(), RegressionFFN(n_tasks=7, input_dim=8, hidden_dim=11, criterion=SID(torch.ones(7))))
    with pytest.raises(NotImplementedError, match="not a SpectralFFN"):
        HeadSpec(reg)
    model = _model()
    model.predictor.ffn.spectral_activation = torch.nn.Sigmoid()
    with pytest.raises(NotImplementedError, match="softplus or exp"):
        HeadSpec(model)
    with pytest.raises(ValueError):
        SpectralFFN(n_tasks=3, input_dim=8, spectral_activation="relu")
    with pytest.raises(NotImplementedError, match="threshold"):
        HeadSpec(_model(crit=SID(torch.ones(7), threshold=-0.1)))


def test_predictspec_maps_to_the_spectral_transform():
    from chemprop_amd.predict import PredictSpec

    spec = PredictSpec(_model(t=7, act="exp"))
    assert spec.transform == "spectral" and spec.out_shape(5) == (5, 7) and spec.unscale is None
    assert _lib.PT_SPECTRAL == 8 and "spectral" not in _lib.PREDICT_TRANSFORM
    model = _model()
    model.predictor.output_transform = torch.nn.Softplus()
    with pytest.raises(NotImplementedError):
        PredictSpec(model)


def test_lib_mirrors_follow_the_header():
    """The enum values and the two appended fields, in the header's order (``tests/test_abi.py`` holds the offsets to a C compiler)."""
    text = (ROOT / "include" / "dmpnn.h").read_text()
    assert re.search(r"DMPNN_LOSS_SID\s*=\s*8\b", text) and re.search(r"DMPNN_LOSS_WASSERSTEIN\s*=\s*9\b", text)
    assert (_lib.LOSS["sid"], _lib.LOSS["wasserstein"]) == (8, 9) and _lib.SPECTRAL_ACT == {"softplus": 0, "exp": 1}
    assert int(re.search(r"#define DMPNN_PT_SPECTRAL (\d+)", text).group(1)) == _lib.PT_SPECTRAL
    body = re.search(r"typedef struct dmpnn_head_args \{(.*?)\} dmpnn_head_args;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert re.search(r"g_att_b;\s*int32_t spectral_act;\s*float spectral_threshold;\s*$", body)
    fields = [f[0] for f in _lib.HeadArgs._fields_]
    assert fields[-3:] == ["g_att_b", "spectral_act", "spectral_threshold"]
    assert _lib.HeadArgs.spectral_threshold.offset == _lib.HeadArgs.spectral_act.offset + 4
    h = _lib.HeadArgs()
    assert (h.spectral_act, h.spectral_threshold) == (0, 0.0) and C.sizeof(h) % 8 == 0


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
    ("sid, valid", 8, {}, ENOSPC, "workspace"),
    ("wasserstein, valid, exp, threshold", 9, dict(spectral_act=1, spectral_threshold=0.01), ENOSPC, "workspace"),
    ("loss 10", 10, {}, EINVAL, "unknown criterion"),
    ("sid with a class dimension", 8, dict(n_classes=2), EINVAL, "unknown criterion"),
    ("wasserstein with a class dimension", 9, dict(n_classes=3), EINVAL, "unknown criterion"),
    ("unknown activation", 8, dict(spectral_act=2), EINVAL, "spectral_act"),
    ("negative threshold", 9, dict(spectral_threshold=-0.5), EINVAL, "spectral_threshold"),
    ("infinite threshold", 9, dict(spectral_threshold=float("inf")), EINVAL, "spectral_threshold"),
    ("nan threshold", 8, dict(spectral_threshold=float("nan")), EINVAL, "spectral_threshold"),
    ("sid, lt_mask", 8, dict(lt_mask=PTR), EINVAL, "bounds"),
    ("wasserstein, gt_mask", 9, dict(gt_mask=PTR), EINVAL, "bounds"),
]


@pytest.mark.parametrize("rule,loss,extra,code,names", HEAD_RULES, ids=[r[0] for r in HEAD_RULES])
def test_head_argument_rules(rule, loss, extra, code, names):
    lib = _lib.load()
    h = _head(loss, **extra)
    rc = lib.dmpnn_head(C.byref(h), PTR, 8, None)
    msg = lib.dmpnn_last_error_string().decode()
    assert rc == code and names in msg, (rule, rc, msg)


def _predict(transform, **head):
    p = _lib.PredictArgs()
    h = _head(head.pop("loss", 0), **head)
    C.memmove(C.byref(p.head), C.byref(h), C.sizeof(h))
    p.transform, p.preds = transform, PTR
    return p


def test_predict_head_argument_rules():
    lib = _lib.load()

    def call(p):
        rc = lib.dmpnn_predict_head(C.byref(p), PTR, 8, None)
        return rc, lib.dmpnn_last_error_string().decode()

    rc, msg = call(_predict(_lib.PT_SPECTRAL, loss=8))
    assert rc == ENOSPC and "workspace" in msg, (rc, msg)
    rc, msg = call(_predict(7, loss=8))                      # (the value between the enum's last and DMPNN_PT_SPECTRAL stays unknown)
    assert rc == EINVAL and "unknown transform" in msg, (rc, msg)
    rc, msg = call(_predict(9, loss=8))
    assert rc == EINVAL and "unknown transform" in msg, (rc, msg)
    p = _predict(_lib.PT_SPECTRAL, loss=9)
    p.out_mean = p.out_scale = PTR
    rc, msg = call(p)
    assert rc == EINVAL and "spectral transform" in msg, (rc, msg)
    rc, msg = call(_predict(_lib.PT_SPECTRAL, loss=8, spectral_act=3))
    assert rc == EINVAL and "spectral" in msg, (rc, msg)
    rc, msg = call(_predict(_lib.PT_SPECTRAL, loss=_lib.LOSS["mve"]))   # (two outputs per task against the transform's one)
    assert rc == EINVAL and "disagree" in msg, (rc, msg)
    rc, msg = call(_predict(_lib.PREDICT_TRANSFORM["mve"], loss=9))
    assert rc == EINVAL and "disagree" in msg, (rc, msg)
    assert lib.dmpnn_predict_head_ws_bytes(C.byref(_predict(_lib.PT_SPECTRAL, loss=8))) > 0
    assert lib.dmpnn_predict_head_ws_bytes(C.byref(_predict(7, loss=8))) == 0
