"""Shared helpers of the head tests (``csrc/dmpnn_head.hip`` through the C ABI): no fixtures, no pytest settings — a plain module.

Two layers:

* ``make_model`` / ``descriptors`` / ``case_inputs`` / ``run_head`` / ``restate``: a mirror model, one ``dmpnn_head`` call on its
  parameters (NaN-prefilled outputs) and the float64 restatement op by op (``tests/test_head_descriptors.py``);
* ``HeadCase`` / ``build_inputs`` / ``reference`` / ``run_case`` / ``compare``: the head on plain tensors, without a model in
  between — any widths, any criterion, any batch vector, NULL gradient pointers, inference — for the boundary sweep of
  ``tests/test_head_boundaries.py``.  ``reference`` runs in float64 (the reference) and in float32 (the yardstick: what plain fp32
  PyTorch does on the very same inputs); ``build_inputs`` moves the inputs away from every kink (ReLU masks, ``|y - p|``, bounds)
  and asserts it, on the CPU, before a GPU is touched.
"""
import ctypes as C
import dataclasses
import math
from typing import Optional

import numpy as np
import torch

from chemprop_amd import _lib
from conftest import parity_err_unfloored

F = torch.nn.functional


# ---- the model layer (moved from tests/test_head_descriptors.py) ---------------------------------------------------------------------
def make_model(d_h, d_xd, hidden, tasks, bn=True, agg="norm", kind="mse", act="relu", n_layers=1, n_classes=3, X_d_transform=None,
               depth=3):
    from chemprop_amd import agg as cagg
    from chemprop_amd.model import (BCE, CE, MAE, MPNN, MSE, MVE, BinaryClassificationFFN, MulticlassClassificationFFN, MveFFN,
                                    RegressionFFN)
    from chemprop_amd.nn import BondMessagePassing

    mp = BondMessagePassing(d_h=d_h, depth=depth, activation=act)
    ag = dict(norm=cagg.NormAggregation, mean=cagg.MeanAggregation, sum=cagg.SumAggregation)[agg]()
    ffn = dict(n_tasks=tasks, input_dim=d_h + d_xd, hidden_dim=hidden, n_layers=n_layers, activation=act)
    if kind == "bce":
        pred = BinaryClassificationFFN(criterion=BCE(1.0), **ffn)
    elif kind == "ce":
        pred = MulticlassClassificationFFN(n_classes, criterion=CE(1.0), **ffn)
    elif kind == "mve":
        pred = MveFFN(criterion=MVE(1.0), **ffn)
    else:
        pred = RegressionFFN(criterion=(MAE if kind.endswith("mae") else MSE)(1.0), **ffn)
    return MPNN(mp, ag, pred, batch_norm=bn, X_d_transform=X_d_transform)


def descriptors(n, d_xd, seed, how="normal"):
    """``normal``: N(0, 1); ``binary``: 0 / 1 bits (Morgan); ``mixed``: every row spans ~1e-3 .. 1e3 (raw rdkit values beside counts)."""
    gen = torch.Generator().manual_seed(seed)
    if how == "binary":
        return (torch.rand(n, d_xd, generator=gen) < 0.1).float()
    x = torch.randn(n, d_xd, generator=gen)
    if how == "mixed":
        x = x.sign() * 10.0 ** (6.0 * torch.rand(n, d_xd, generator=gen) - 3.0)
        x[:, 0], x[:, -1] = 1e3, -1e-3   # (both ends in every row)
    return x


def run_head(model, Hv, batch, n_mols, T, w, lt, gt, X=None):
    """One ``dmpnn_head`` call (forward + backward, ``bn_training``) with descriptors ``X`` (or none) handed over as they are
    (``ld_xd`` = the view's row stride); returns (loss, preds, {param id: grad}, gH_v)."""
    from chemprop_amd import engine
    from chemprop_amd.model import HeadSpec

    lib = _lib.load()
    spec = HeadSpec(model)
    dev = Hv.device
    grads = {id(p): torch.zeros_like(p) for p in spec.params()}
    h = _lib.HeadArgs()
    nV, d = int(Hv.shape[0]), int(Hv.shape[1])
    keep = spec.fill(h, nV, n_mols, d, batch, T, w, lt if spec.bounded else None, gt if spec.bounded else None,
                     lambda p: None if p is None else grads[id(p)].data_ptr(), X_d=X)
    preds = torch.full((n_mols, spec.n_out), float("nan"), device=dev)
    loss = torch.empty(2, device=dev)
    gH = torch.full((nV, d), float("nan"), device=dev)
    h.preds, h.loss_out, h.gHv, h.ldg = preds.data_ptr(), loss.data_ptr(), gH.data_ptr(), d
    nb = int(lib.dmpnn_head_ws_bytes(C.byref(h)))
    ws = torch.empty(nb, dtype=torch.uint8, device=dev)
    h.ws, h.ws_bytes = ws.data_ptr(), nb
    with engine._OnDevice(dev):
        _lib.check(lib.dmpnn_head(C.byref(h), Hv.data_ptr(), Hv.stride(0), engine._stream_ptr(dev)), "dmpnn_head")
    torch.cuda.synchronize()
    del keep
    return float(loss[0]), preds.cpu(), {k: g.cpu() for k, g in grads.items()}, gH.cpu()


def restate(model, Hv, batch, n_mols, T, w, lt, gt, X=None):
    """The head in float64 on the CPU, op by op: agg, BatchNorm1d (training), cat(., X_d) when there are descriptors, the MLP, the
    criterion; returns (loss, raw outputs, {param id: grad}, gH_v, {running_mean, running_var})."""
    from chemprop_amd.model import MODES, HeadSpec, masked_loss

    spec = HeadSpec(model)
    f = lambda t: t.detach().cpu().double()
    Hv64 = f(Hv).requires_grad_()
    b = batch.cpu()
    d = Hv64.shape[1]
    H = torch.zeros(n_mols, d, dtype=torch.float64).index_add(0, b, Hv64)
    mode = {v: k for k, v in MODES.items()}[spec.agg_mode]
    if mode == "mean":
        H = H / torch.bincount(b, minlength=n_mols).clamp(min=1).double().view(-1, 1)
    elif mode == "norm":
        H = H / spec.agg_norm
    leaves, bufs = {}, {}
    if spec.bn is not None:
        bw, bb = f(spec.bn.weight).requires_grad_(), f(spec.bn.bias).requires_grad_()
        rm, rv = f(spec.bn.running_mean).clone(), f(spec.bn.running_var).clone()
        H = torch.nn.functional.batch_norm(H, rm, rv, bw, bb, training=True, momentum=spec.bn.momentum, eps=spec.bn.eps)
        leaves[id(spec.bn.weight)], leaves[id(spec.bn.bias)] = bw, bb
        bufs = dict(running_mean=rm, running_var=rv)
    Z = H if X is None else torch.cat((H, f(X)), 1)
    for i, blk in enumerate(model.predictor.ffn):
        lin = blk[-1]
        if i > 0:
            Z = blk[0](Z)
        W = f(lin.weight).requires_grad_()
        leaves[id(lin.weight)] = W
        bias = None
        if lin.bias is not None:
            bias = f(lin.bias).requires_grad_()
            leaves[id(lin.bias)] = bias
        Z = torch.nn.functional.linear(Z, W, bias)
    Y = Z
    if spec.kind == "ce":
        P = Y.reshape(n_mols, -1, spec.n_classes)
    elif spec.kind == "mve":
        mean, var = torch.chunk(Y, 2, 1)
        P = torch.stack((mean, torch.nn.functional.softplus(var)), 2)
    else:
        P = Y
    T64 = f(T)
    l = masked_loss(P, T64, None if w is None else f(w), None, f(lt) > 0 if (lt is not None and spec.bounded) else None,
                    f(gt) > 0 if (gt is not None and spec.bounded) else None, spec.kind)
    l.backward()
    return float(l.detach()), Y.detach(), {k: v.grad for k, v in leaves.items()}, Hv64.grad, bufs


def case_inputs(case, dev, seed=0):
    """``case``: (form, n_mols, d_h, d_xd, hidden, tasks, n_layers, bn, agg, kind, act, X_d kind, strided view); ``d_xd == 0``: no
    descriptors (``X`` is ``None``)."""
    from chemprop_amd import synth

    form, n, d_h, d_xd, hidden, tasks, n_layers, bn, agg, kind, act, xk, strided = case
    torch.manual_seed(seed + 5)
    model = make_model(d_h, d_xd, hidden, tasks, bn, agg, kind, act, n_layers).to(dev).train()
    if bn:   # (non-trivial batch-norm parameters and running statistics)
        with torch.no_grad():
            model.bn.weight.uniform_(0.5, 1.5), model.bn.bias.uniform_(-0.5, 0.5)
            model.bn.running_mean.uniform_(-0.1, 0.1), model.bn.running_var.uniform_(0.5, 2.0)
    bmg = synth.random_batch(n, "qm9", seed=seed + 9)
    gen = torch.Generator().manual_seed(seed + 2)
    Hv = torch.randn(int(bmg.V.shape[0]), d_h, generator=gen).to(dev)
    batch = bmg.batch.to(dev)
    if kind == "bce":
        T = torch.rand(n, tasks, generator=gen).round()
    elif kind == "ce":
        T = torch.randint(0, 3, (n, tasks), generator=gen).float()
    else:
        T = torch.randn(n, tasks, generator=gen)
    if tasks > 1:
        T[torch.rand(n, tasks, generator=gen) < 0.2] = float("nan")
    w = 0.5 + torch.rand(n, 1, generator=gen)
    lt = (torch.rand(n, tasks, generator=gen) < 0.3) if kind.startswith("bounded") else None
    gt = (torch.rand(n, tasks, generator=gen) < 0.3) if kind.startswith("bounded") else None
    if d_xd == 0:
        X = None
    else:
        X = descriptors(n, d_xd, seed + 4, xk)
        if strided:   # a view into a wider table: row stride > d_xd, an address that is not 16-byte aligned
            big = torch.randn(n, d_xd + 7, generator=gen)
            big[:, 3:3 + d_xd] = X
            X = big.to(dev)[:, 3:3 + d_xd]
            assert X.stride(0) == d_xd + 7 and X.data_ptr() % 16 != 0
        else:
            X = X.to(dev)
    to = lambda t: None if t is None else t.to(dev)
    return model, Hv, batch, n, to(T), to(w), to(lt), to(gt), X


# ---- the tensor layer ----------------------------------------------------------------------------------------------------------------
EPS32 = 2.0 ** -23
# the floored bars the suite already holds (tests/test_head_descriptors.py, tests/test_model.py): the unfloored bar of a tensor never exceeds them
CAP = dict(loss=1e-5, preds=2e-5, grad=2e-5, stat=1e-6)
PER_TASK = dict(mse=1, mae=1, bce=1, ce=None, mve=2, evidential=4, quantile=2)
KINKED_ACT = ("relu", "leakyrelu")
LEAKY_SLOPE = 0.1


@dataclasses.dataclass(frozen=True)
class HeadCase:
    """One ``dmpnn_head`` call.  ``form``: ``rows`` / ``chain`` (``DMPNN_HEAD``) or ``default`` (no variable: the size rules decide).
    ``hidden``: widths of the predictor's hidden layers (``()``: one linear layer).  ``kind``: ``mse | mae | bce | ce | mve |
    evidential | quantile``; ``bounded``: ``lt_mask`` / ``gt_mask`` (MSE / MAE).  ``layout``: the batch vector (``make_batch``).
    ``missing``: ``some`` (20 % NaN targets when there is more than one task) / ``dead`` (and task column 1 without any finite
    target) / ``all`` (no finite target in the batch) / ``none``.  ``mode``: ``train`` (forward + backward), ``infer`` (no targets,
    batch norm on its running statistics), ``eval-loss`` (targets and loss, no gradients, batch norm in training mode).
    ``frozen``: ``gW[0]`` and ``g_bn_weight`` NULL.  ``const_col``: columns 1 and 2 of ``H_v`` are constant (variance 0 behind a mean
    aggregation).  ``env``: ``DMPNN_HEAD_QPW`` / ``DMPNN_HEAD_AGG``."""
    id: str
    form: str
    B: int
    d_h: int
    hidden: tuple
    tasks: int
    kind: str = "mse"
    act: str = "relu"
    agg: str = "mean"
    bn: bool = True
    bounded: bool = False
    n_classes: int = 0
    d_xd: int = 0
    layout: str = "mols"
    missing: str = "some"
    mode: str = "train"
    frozen: bool = False
    const_col: bool = False
    env: tuple = ()
    seed: int = 0

    @property
    def per_task(self):
        return self.n_classes if self.kind == "ce" else PER_TASK[self.kind]

    @property
    def dims(self):
        return (self.d_h + self.d_xd,) + tuple(self.hidden) + (self.tasks * self.per_task,)


def make_batch(layout: str, B: int, seed: int) -> torch.Tensor:
    """A sorted batch vector (int64) of ``B`` molecules.
    ``mols``: 1 .. 27 atoms per molecule;  ``ragged``: molecules without atoms at the start, in the middle and the last two (behind
    ``batch[-1]``), a run of single-atom molecules, and one molecule holding more than half of all atoms;  ``one-each``: ``n_atoms ==
    n_mols``;  ``huge``: more than 32 768 atoms (the multi-block bounds kernel)."""
    gen = torch.Generator().manual_seed(1000 + seed)
    if layout == "one-each":
        counts = torch.ones(B, dtype=torch.int64)
    elif layout == "huge":
        counts = torch.randint(20, 60, (B,), generator=gen)
        counts[0] += max(0, 32769 + 64 - int(counts.sum()))
    else:
        counts = torch.randint(1, 28, (B,), generator=gen)
        if layout == "ragged":
            assert B >= 12
            counts[0] = 0
            counts[B // 2] = counts[B // 2 + 1] = 0
            counts[-2:] = 0
            counts[3:3 + min(40, B // 3)] = 1
            counts[2] = int(counts.sum()) + 33   # (more than half of the atoms; many rounds of 16 rows)
        else:
            assert layout == "mols", layout
    return torch.repeat_interleave(torch.arange(B), counts)


def _act(name, x):
    if name == "relu":
        return F.relu(x)
    if name == "leakyrelu":
        return F.leaky_relu(x, LEAKY_SLOPE)
    if name == "tanh":
        return torch.tanh(x)
    if name == "elu":
        return F.elu(x)
    assert name == "none", name
    return x


def criterion(case: HeadCase, Y, T, w, tw, lt, gt, v_kl=0.2, eps=1e-8, alpha=0.1):
    """The seven criteria on the RAW outputs ``Y [B, t * per_task]`` as the predictors and metrics of the reference define them:
    ``sum(L w_row w_task [target finite]) / #finite`` (NaN without a finite target)."""
    t = case.tasks
    mask = T.isfinite()
    y = torch.where(mask, T, torch.zeros_like(T))
    sp = F.softplus
    if case.kind == "ce":
        x = Y.reshape(Y.shape[0], t, case.n_classes)
        L = torch.logsumexp(x, 2) - torch.gather(x, 2, y.long().unsqueeze(2)).squeeze(2)
    elif case.kind == "mve":        # chunked outputs: column k t + j is value k of task j
        var = sp(Y[:, t:])
        L = (Y[:, :t] - y) ** 2 / (2 * var) + torch.log(2 * math.pi * var) / 2
    elif case.kind == "quantile":   # pinball loss of the lower and of the upper bound
        L = 0
        for bound, tau in ((Y[:, :t], alpha / 2), (Y[:, t:], 1 - alpha / 2)):
            e = y - bound
            L = L + torch.maximum(tau * e, (tau - 1) * e)
    elif case.kind == "evidential":
        mean, v, al, be = Y[:, :t], sp(Y[:, t:2 * t]), sp(Y[:, 2 * t:3 * t]) + 1, sp(Y[:, 3 * t:])
        res = y - mean
        tbl = 2 * be * (1 + v)
        L = (0.5 * torch.log(math.pi / v) - al * torch.log(tbl) + (al + 0.5) * torch.log(v * res ** 2 + tbl) + torch.lgamma(al)
             - torch.lgamma(al + 0.5)) + v_kl * ((2 * v + al) * res.abs() - eps)
    else:
        p = Y
        if lt is not None:
            p = torch.where((p < y) & lt, y, p)
        if gt is not None:
            p = torch.where((p > y) & gt, y, p)
        if case.kind == "bce":
            L = F.softplus(p) - y * p
        elif case.kind == "mae":
            L = (p - y).abs()
        else:
            L = (p - y) ** 2
    L = L * w.view(-1, 1) * tw.view(1, -1)
    return torch.where(mask, L, torch.zeros_like(L)).sum() / mask.sum()


def reference(case: HeadCase, inp: dict, dtype=torch.float64) -> dict:
    """The head op by op on the CPU in ``dtype``: aggregation by ``index_add``, ``F.batch_norm``, ``cat(., X_d)``, ``F.linear`` and
    the activation per layer, the criterion, autograd.  Returns every output of the call by name — ``loss``, ``preds``, ``gHv``,
    ``gW{l}``, ``gb{l}``, ``g_bn_weight``, ``g_bn_bias``, ``running_mean``, ``running_var`` — and ``z``: the pre-activations of the
    hidden layers."""
    f = lambda k: None if inp.get(k) is None else inp[k].to(dtype)
    train = case.mode != "infer"
    grad = case.mode == "train"
    Hv = f("Hv").requires_grad_(grad)
    b, B = inp["batch"], case.B
    H = torch.zeros(B, case.d_h, dtype=dtype).index_add(0, b, Hv)
    if case.agg == "mean":
        H = H / torch.bincount(b, minlength=B).clamp(min=1).to(dtype).view(-1, 1)
    elif case.agg == "norm":
        H = H / inp["agg_norm"]
    out, leaves = {}, {}
    if case.bn:
        bw, bb = f("bn_weight").requires_grad_(grad), f("bn_bias").requires_grad_(grad)
        rm, rv = f("running_mean").clone(), f("running_var").clone()
        H = F.batch_norm(H, rm, rv, bw, bb, training=train, momentum=inp["bn_momentum"], eps=inp["bn_eps"])
        leaves.update(g_bn_weight=bw, g_bn_bias=bb)
        out.update(running_mean=rm, running_var=rv)
    Z = H if inp.get("X") is None else torch.cat((H, f("X")), 1)
    zs = []
    n_lin = len(case.dims) - 1
    for l in range(n_lin):
        W, bias = inp[f"W{l}"].to(dtype).requires_grad_(grad), inp[f"b{l}"].to(dtype).requires_grad_(grad)
        leaves[f"gW{l}"], leaves[f"gb{l}"] = W, bias
        Z = F.linear(Z, W, bias)
        if l + 1 < n_lin:
            zs.append(Z.detach())
            Z = _act(case.act, Z)
    out.update(preds=Z.detach(), z=zs)
    if case.mode == "infer":
        return out
    lt, gt = (inp.get("lt"), inp.get("gt")) if case.bounded else (None, None)
    loss = criterion(case, Z, f("T"), f("w"), f("tw"), lt, gt)
    out["loss"] = loss.detach()
    if grad:
        loss.backward()
        out["gHv"] = Hv.grad
        for k, v in leaves.items():
            out[k] = v.grad
    return out


def _unkink_bias(z: torch.Tensor, delta: float) -> torch.Tensor:
    """Per column j of the pre-activations ``z [B, N]`` the shift ``s_j`` of smallest magnitude with ``min_i |z_ij + s_j| >= delta``
    (0 where the column is already clear).  The forbidden set of a column is the union of the intervals ``(-z_ij - delta, -z_ij +
    delta)``: from 0 the walk goes to the end of the interval it stands in, in either direction, until it stands in none."""
    s = torch.zeros(z.shape[1], dtype=torch.float64)
    bad = (z.abs().min(0).values < delta).nonzero().flatten().tolist()
    zn = z.double().numpy()
    for j in bad:
        c = np.sort(-zn[:, j])
        best = None
        for sign in (1.0, -1.0):
            x = 0.0
            if sign > 0:
                i = int(np.searchsorted(c, x - delta, side="right"))   # (the first centre above x - delta)
                while i < len(c) and c[i] < x + delta:
                    x, i = c[i] + delta, i + 1
            else:
                i = int(np.searchsorted(c, x + delta, side="left")) - 1   # (the last centre below x + delta)
                while i >= 0 and c[i] > x - delta:
                    x, i = c[i] - delta, i - 1
            if best is None or abs(x) < abs(best):
                best = x
        s[j] = best
    return s


def build_inputs(case: HeadCase) -> dict:
    """The call's inputs as float32 CPU tensors (``batch`` int64, masks bool), away from every kink:
    * ReLU / LeakyReLU: layer by layer the hidden biases are shifted per unit (``_unkink_bias``, with a margin of 2 for the bias's own
      fp32 rounding) until ``min |z| >= delta = 1e-4 max|z|`` holds for the float64 pre-activations of the FINAL fp32 inputs — asserted;
    * MAE / quantile / evidential and the bounded criteria: ``min |y - p| >= 1e-4 max|p|`` over the finite targets (the masked ones for
      bounded MSE) — asserted; the target seed advances until it holds (``inp["target_seed"]``).
    No element is ever excluded from a comparison."""
    gen = torch.Generator().manual_seed(77 + case.seed)
    rn = lambda *s: torch.randn(*s, generator=gen)
    B, d, dims = case.B, case.d_h, case.dims
    batch = make_batch(case.layout, B, case.seed)
    inp = dict(batch=batch, Hv=rn(int(batch.numel()), d), agg_norm=100.0 if case.agg == "norm" else 1.0, bn_eps=1e-5, bn_momentum=0.1)
    if case.const_col:
        assert d >= 4 and case.layout != "ragged"
        inp["Hv"][:, 1], inp["Hv"][:, 2] = 0.0, 1.0
    if case.bn:
        u = lambda lo, hi: lo + (hi - lo) * torch.rand(d, generator=gen)
        inp.update(bn_weight=u(0.5, 1.5), bn_bias=u(-0.5, 0.5), running_mean=u(-0.1, 0.1), running_var=u(0.5, 2.0))
    if case.d_xd:
        inp["X"] = rn(B, case.d_xd)
    for l in range(len(dims) - 1):   # (nn.Linear's default range)
        k = 1.0 / math.sqrt(dims[l])
        inp[f"W{l}"] = (2 * torch.rand(dims[l + 1], dims[l], generator=gen) - 1) * k
        inp[f"b{l}"] = (2 * torch.rand(dims[l + 1], generator=gen) - 1) * k
    inp["w"] = 0.5 + torch.rand(B, generator=gen)
    inp["tw"] = 0.5 + torch.rand(case.tasks, generator=gen)   # (non-unit task weights)
    fwd = dataclasses.replace(case, mode="infer")
    deltas = []
    if case.act in KINKED_ACT:
        for l in range(len(case.hidden)):
            z = reference(fwd, inp)["z"][l]
            delta = 1e-4 * float(z.abs().max())
            b64 = inp[f"b{l}"].double() + _unkink_bias(z, 2 * delta)
            inp[f"b{l}"] = b64.float()
        for l, z in enumerate(reference(fwd, inp)["z"]):
            delta = 1e-4 * float(z.abs().max())
            assert float(z.abs().min()) >= delta, (case.id, l, float(z.abs().min()), delta)
            deltas.append(delta)
    inp["z_delta"] = deltas
    if case.mode == "infer":
        return inp
    P = reference(fwd, inp)["preds"]
    t = case.tasks
    for seed in range(case.seed, case.seed + 20):
        g = torch.Generator().manual_seed(4242 + seed)
        if case.kind == "bce":
            T = torch.rand(B, t, generator=g).round()
        elif case.kind == "ce":
            T = torch.randint(0, case.n_classes, (B, t), generator=g).float()
        else:
            T = torch.randn(B, t, generator=g)
        if case.missing in ("some", "dead") and t > 1:
            T[torch.rand(B, t, generator=g) < 0.2] = float("nan")
        if case.missing == "dead":
            assert t > 1
            T[:, 1] = float("nan")
        if case.missing == "all":
            T[:] = float("nan")
        lt = gt = None
        if case.bounded:
            lt, gt = torch.rand(B, t, generator=g) < 0.3, torch.rand(B, t, generator=g) < 0.3
        fin = T.isfinite()
        gaps = []
        if case.kind in ("mae", "evidential"):
            gaps.append((T.double() - P[:, :t]).abs()[fin])
        if case.kind == "quantile":
            gaps += [(T.double() - P[:, :t]).abs()[fin], (T.double() - P[:, t:]).abs()[fin]]
        if case.bounded:
            gaps.append((T.double() - P).abs()[fin & (lt | gt)])
        gap = min([float(x.min()) for x in gaps if x.numel()], default=float("inf"))
        if gap >= 1e-4 * float(P.abs().max()):
            break
    else:
        raise AssertionError(f"{case.id}: no target seed keeps |y - p| away from 0")
    inp.update(T=T, lt=lt, gt=gt, target_seed=seed, yp_gap=gap)
    return inp


def output_names(case: HeadCase) -> list:
    """The outputs of the call a test compares (by the names ``reference`` and ``run_case`` use)."""
    names = ["preds"]
    if case.mode != "infer":
        names.append("loss")
    if case.bn and case.mode != "infer":
        names += ["running_mean", "running_var"]
    if case.mode == "train":
        names.append("gHv")
        for l in range(len(case.dims) - 1):
            names += ([] if (case.frozen and l == 0) else [f"gW{l}"]) + [f"gb{l}"]
        if case.bn:
            names += ([] if case.frozen else ["g_bn_weight"]) + ["g_bn_bias"]
    return names


def cap_of(name: str) -> float:
    return CAP["loss" if name == "loss" else "preds" if name == "preds" else "stat" if name.startswith("running") else "grad"]


def run_case(case: HeadCase, inp: dict, dev, env: Optional[dict] = None) -> dict:
    """One ``dmpnn_head`` call on the device: every output prefilled with NaN.  The environment switches (``DMPNN_HEAD`` from
    ``case.form``, ``case.env``, then ``env``) are set for the call and restored.  Returns the outputs on the CPU by name, with
    ``running_mean`` / ``running_var`` / ``num_batches_tracked`` after the call."""
    import os

    from chemprop_amd import engine
    from chemprop_amd.agg import MODES

    lib = _lib.load()
    to = lambda k: None if inp.get(k) is None else inp[k].to(dev).contiguous()
    Hv, batch = to("Hv"), to("batch")
    dims, n_lin = case.dims, len(case.dims) - 1
    h = _lib.HeadArgs()
    h.n_atoms, h.n_mols, h.d_h, h.batch = int(Hv.shape[0]), case.B, case.d_h, batch.data_ptr()
    h.agg_mode, h.agg_norm = MODES[case.agg], float(inp["agg_norm"])
    keep, out = [Hv, batch], {}
    nan = lambda *s: torch.full(s, float("nan"), device=dev)
    train, grad = case.mode != "infer", case.mode == "train"
    if case.bn:
        bw, bb, rm, rv = to("bn_weight"), to("bn_bias"), to("running_mean"), to("running_var")
        nbt = torch.tensor(5, dtype=torch.int64, device=dev)
        h.bn_weight, h.bn_bias, h.bn_running_mean, h.bn_running_var = bw.data_ptr(), bb.data_ptr(), rm.data_ptr(), rv.data_ptr()
        h.bn_eps, h.bn_momentum, h.bn_training = float(inp["bn_eps"]), float(inp["bn_momentum"]), 1 if train else 0
        if train:
            h.bn_num_batches_tracked = nbt.data_ptr()
        out.update(running_mean=rm, running_var=rv, num_batches_tracked=nbt)
        keep += [bw, bb]
        if grad:
            out["g_bn_bias"] = nan(case.d_h)
            h.g_bn_bias = out["g_bn_bias"].data_ptr()
            if not case.frozen:
                out["g_bn_weight"] = nan(case.d_h)
                h.g_bn_weight = out["g_bn_weight"].data_ptr()
    h.n_layers, h.act, h.act_slope = n_lin, _lib.ACT[case.act if case.hidden else "none"], LEAKY_SLOPE if case.act == "leakyrelu" else 0.0
    for l in range(n_lin + 1):
        h.dims[l] = dims[l]
    for l in range(n_lin):
        W, b = to(f"W{l}"), to(f"b{l}")
        keep += [W, b]
        h.W[l], h.b[l] = W.data_ptr(), b.data_ptr()
        if grad:
            out[f"gb{l}"] = nan(dims[l + 1])
            h.gb[l] = out[f"gb{l}"].data_ptr()
            if not (case.frozen and l == 0):
                out[f"gW{l}"] = nan(dims[l + 1], dims[l])
                h.gW[l] = out[f"gW{l}"].data_ptr()
    if case.d_xd:
        X = to("X")
        keep.append(X)
        h.X_d, h.ld_xd = X.data_ptr(), X.stride(0)
    h.loss, h.n_classes = _lib.LOSS[case.kind], case.n_classes
    h.evid_v_kl, h.evid_eps, h.quantile_alpha = 0.2, 1e-8, 0.1
    out["preds"] = nan(case.B, dims[-1])
    h.preds = out["preds"].data_ptr()
    if train:
        T, w, tw = to("T"), to("w"), to("tw")
        keep += [T, w, tw]
        h.targets, h.weights, h.task_weights = T.data_ptr(), w.data_ptr(), tw.data_ptr()
        if case.bounded:
            lt, gt = inp["lt"].to(torch.uint8).to(dev).contiguous(), inp["gt"].to(torch.uint8).to(dev).contiguous()
            keep += [lt, gt]
            h.lt_mask, h.gt_mask = lt.data_ptr(), gt.data_ptr()
        loss2 = nan(2)
        h.loss_out = loss2.data_ptr()
    if grad:
        out["gHv"] = nan(int(Hv.shape[0]), case.d_h)
        h.gHv, h.ldg = out["gHv"].data_ptr(), case.d_h
    want = dict(DMPNN_HEAD=None if case.form == "default" else case.form, DMPNN_HEAD_QPW=None, DMPNN_HEAD_AGG=None)
    want.update(dict(case.env))
    want.update(env or {})
    saved = {k: os.environ.get(k) for k in want}
    try:
        for k, v in want.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        nb = int(lib.dmpnn_head_ws_bytes(C.byref(h)))
        ws = torch.empty(max(nb, 16), dtype=torch.uint8, device=dev)
        h.ws, h.ws_bytes = ws.data_ptr(), nb
        with engine._OnDevice(dev):
            _lib.check(lib.dmpnn_head(C.byref(h), Hv.data_ptr(), Hv.stride(0), engine._stream_ptr(dev)), "dmpnn_head")
        torch.cuda.synchronize()
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    del keep
    res = {k: v.cpu() for k, v in out.items()}
    if train:
        res["loss"], res["n_finite"] = loss2[0].cpu(), float(loss2[1])
    return res


def yardstick(case: HeadCase, inp: dict):
    """(ref64, e32): the float64 reference and, per output, the unfloored error of the float32 restatement against it."""
    r64, r32 = reference(case, inp, torch.float64), reference(case, inp, torch.float32)
    e32 = {k: parity_err_unfloored(r32[k].double().numpy(), r64[k].numpy()) for k in output_names(case)}
    return r64, e32


def compare(case: HeadCase, got: dict, ref: dict, e32: dict, margin: float, report=print) -> list:
    """Every output of ``got`` against ``ref``: finite wherever the reference is, ``err = max|got - ref| / max|ref|`` (exactly 0
    where ``max|ref|`` is 0) within ``min(margin max(e32, 2**-23), cap)``.  Reports one line per tensor BEFORE judging; returns the
    list of failures (empty: all held)."""
    fails = []
    for k in output_names(case):
        g, r = got[k].double().reshape(-1), ref[k].double().reshape(-1)
        assert g.shape == r.shape, (case.id, k, tuple(got[k].shape), tuple(ref[k].shape))
        if not bool(torch.isfinite(g[torch.isfinite(r)]).all()):
            fails.append(f"{k}: not finite where the reference is")
            report(f"HEADBAR {case.id} {k} nonfinite")
            continue
        if not bool(torch.isfinite(r).all()):   # (no finite target in the batch: a NaN loss on both sides; its gradients are not compared)
            if k == "loss" and not bool(torch.isnan(g).all()):
                fails.append("loss: the reference is NaN (no finite target), the kernel's is not")
            continue
        last = len(case.dims) - 2
        if case.missing == "dead" and k in (f"gW{last}", f"gb{last}"):   # (outputs of a task without targets: exactly 0)
            dead = (ref[k].reshape(ref[k].shape[0], -1) == 0).all(1)
            assert int(dead.sum()) >= case.per_task, (case.id, k)
            if not bool((got[k].reshape(got[k].shape[0], -1)[dead] == 0).all()):
                fails.append(f"{k}: rows of a task without targets are not exactly 0")
        err = parity_err_unfloored(g.numpy(), r.numpy())
        scale = float(r.abs().max())
        bar = 0.0 if scale == 0.0 else min(margin * max(e32[k], EPS32), cap_of(k))
        ratio = err / max(e32[k], EPS32)
        report(f"HEADBAR {case.id} {k} err={err:.3e} e32={e32[k]:.3e} ratio={ratio:.2f} bar={bar:.3e} maxref={scale:.3e}")
        if not err <= bar:
            fails.append(f"{k}: err {err:.3e} > bar {bar:.3e} (fp32 yardstick {e32[k]:.3e}, ratio {ratio:.1f}, max|ref| {scale:.3e})")
    return fails
