"""Shared helpers of the inference-head tests (``dmpnn_predict_head`` through the C ABI): no fixtures, no pytest settings — a plain module.

``PredictCase`` / ``build_inputs`` / ``predict_ref`` / ``run_case`` / ``compare``: the inference head on plain tensors, without a model
in between — any widths, any of the seven transforms, any batch vector.  ``predict_ref`` restates the call op by op on the CPU in
float64 (the reference) or float32 (the yardstick: what plain fp32 PyTorch does on the very same inputs); ``wrong`` switches ONE
deliberate mistake on, for the tests that show the bar would catch it.
"""
import ctypes as C
import dataclasses
import math

import torch

from chemprop_amd import _lib
from conftest import parity_err_unfloored
from head_harness import CAP, EPS32, LEAKY_SLOPE, _act, criterion, make_batch

F = torch.nn.functional
GROUP = dict(none=1, unscale=1, sigmoid=1, softmax=None, mve=2, evidential=4, quantile=2)   # outputs per task of a transform
NAMES = ("fingerprint", "raw", "preds", "loss")
GUARD = 3          # NaN rows behind every output
FP_PAD = 3         # columns of the fingerprint's rows beyond dims[0]


@dataclasses.dataclass(frozen=True)
class PredictCase:
    """One ``dmpnn_predict_head`` call.  ``hidden``: widths of the predictor's hidden layers (``()``: one linear layer); ``tasks`` and
    ``transform`` (``nc`` classes per task for the softmax) give the output width, unless ``n_out`` names it (transform ``none``);
    ``unscale``: ``out_mean`` / ``out_scale`` given; ``kind``: the criterion when targets are given (``None``: predictions only);
    ``agg``: ``sum | mean | norm | attentive``; ``pad_xd``: ``ld_xd - d_xd``."""
    id: str
    B: int = 5
    d_h: int = 8
    hidden: tuple = (8,)
    tasks: int = 1
    transform: str = "unscale"
    nc: int = 0
    n_out: int = 0
    unscale: bool = True
    kind: str = None
    bounded: bool = False
    missing: str = "some"
    act: str = "relu"
    agg: str = "mean"
    bn: bool = True
    d_xd: int = 0
    pad_xd: int = 5
    layout: str = "mols"
    n_components: int = 1
    seed: int = 0

    @property
    def per_task(self):
        return self.nc if self.transform == "softmax" else GROUP[self.transform]

    @property
    def width(self):
        return self.n_out if self.n_out else self.tasks * self.per_task

    @property
    def n_tasks(self):
        return self.width // self.per_task

    @property
    def n_classes(self):   # (what head_harness.criterion reads)
        return self.nc

    @property
    def dims(self):
        return (self.n_components * self.d_h + self.d_xd,) + tuple(self.hidden) + (self.width,)

    @property
    def usual(self):
        """The model whose call with a ready split is three launches (four with targets): dmpnn.h."""
        return (self.agg != "attentive" and self.bn and len(self.hidden) == 1 and self.width <= _lib.PREDICT_MAX_OUT and self.B <= 1024
                and self.d_h % 4 == 0 and self.dims[0] % 4 == 0 and self.hidden[0] % 4 == 0)


def build_inputs(case: PredictCase) -> dict:
    """The call's inputs as float32 CPU tensors (``batch`` int64, masks bool): batch norm with non-trivial running statistics."""
    gen = torch.Generator().manual_seed(177 + case.seed)
    rn = lambda *s: torch.randn(*s, generator=gen)
    B, d, dims, nc = case.B, case.d_h, case.dims, case.n_components
    batch = make_batch(case.layout, nc * B, case.seed)
    inp = dict(batch=batch, Hv=rn(int(batch.numel()), d), agg_norm=100.0 if case.agg == "norm" else 1.0, bn_eps=1e-5, bn_momentum=0.1)
    u = lambda n, lo, hi: lo + (hi - lo) * torch.rand(n, generator=gen)
    if case.bn:
        inp.update(bn_weight=u(nc * d, 0.5, 1.5), bn_bias=u(nc * d, -0.5, 0.5), running_mean=u(nc * d, -0.1, 0.1), running_var=u(nc * d, 0.5, 2.0))
    if case.agg == "attentive":
        inp.update(att_W=rn(1, d) / math.sqrt(d), att_b=rn(1))
    if case.d_xd:
        inp["X"] = rn(B, case.d_xd)
    for l in range(len(dims) - 1):   # (nn.Linear's default range)
        k = 1.0 / math.sqrt(dims[l])
        inp[f"W{l}"] = (2 * torch.rand(dims[l + 1], dims[l], generator=gen) - 1) * k
        inp[f"b{l}"] = (2 * torch.rand(dims[l + 1], generator=gen) - 1) * k
    t = case.n_tasks
    if case.unscale:
        inp.update(out_mean=u(t, -3.0, 3.0), out_scale=u(t, 0.5, 4.0))
    if case.kind is not None:
        if case.kind == "bce":
            T = torch.rand(B, t, generator=gen).round()
        elif case.kind == "ce":
            T = torch.randint(0, case.nc, (B, t), generator=gen).float()
        else:
            T = rn(B, t)
        if case.missing == "some" and B * t > 1:
            T[torch.rand(B, t, generator=gen) < 0.2] = float("nan")
            if not bool(T.isfinite().any()):
                T[0, 0] = 0.0
        inp.update(T=T, w=u(B, 0.5, 1.5), tw=u(t, 0.5, 1.5))
        if case.bounded:
            inp.update(lt=torch.rand(B, t, generator=gen) < 0.3, gt=torch.rand(B, t, generator=gen) < 0.3)
    return inp


def transform_ref(name: str, Y, t: int, nc: int, s, m, wrong: str = None):
    """The eval-mode ``forward`` of the reference's predictors on the raw outputs ``Y [B, n_out]`` (``nn/predictors.py`` with
    ``UnscaleTransform`` / ``transform_variance``); ``s`` / ``m``: ``[t]`` scales and means."""
    sp = F.softplus
    s2 = s if wrong == "s_not_squared" else s * s
    if wrong == "stacked":     # column j G + k instead of k t + j
        chunk = lambda k, G: Y[:, k::G]
    else:
        chunk = lambda k, G: Y[:, k * t:(k + 1) * t]
    if name == "none":
        return Y
    if name == "unscale":
        return Y * s + m
    if name == "sigmoid":
        return Y.sigmoid()
    if name == "softmax":
        return Y.reshape(Y.shape[0], t, nc).softmax(-1)
    if name == "mve":
        return torch.stack((chunk(0, 2) * s + m, sp(chunk(1, 2)) * s2), 2)
    if name == "evidential":
        return torch.stack((chunk(0, 4) * s + m, sp(chunk(1, 4)), sp(chunk(2, 4)) + 1, sp(chunk(3, 4)) * s2), 2)
    assert name == "quantile", name
    lo, up = chunk(0, 2) * s + m, chunk(1, 2) * s + m
    return torch.stack(((lo + up) / 2, up - lo), 2)


def predict_ref(case: PredictCase, inp: dict, dtype=torch.float64, wrong: str = None) -> dict:
    """The inference head op by op on the CPU in ``dtype``: aggregation by ``index_add`` (the attention's softmax per molecule),
    ``F.batch_norm`` on the running statistics, ``cat(., X_d)``, ``F.linear`` and the activation per layer, the output transform, the
    criterion on the raw outputs.  Returns ``fingerprint``, ``raw``, ``preds`` and — with targets — ``loss`` / ``n_finite``.
    ``wrong``: ``s_not_squared`` | ``stacked`` | ``batch_stats``, one deliberate mistake."""
    f = lambda k: None if inp.get(k) is None else inp[k].to(dtype)
    Hv, b, B, nc = f("Hv"), inp["batch"], case.B, case.n_components
    if case.agg == "attentive":
        logit = (Hv @ f("att_W").t() + f("att_b")).reshape(-1)
        mx = torch.full((nc * B,), -float("inf"), dtype=dtype).scatter_reduce(0, b, logit, "amax")
        e = torch.exp(logit - mx[b])
        alpha = e / torch.zeros(nc * B, dtype=dtype).index_add(0, b, e)[b]
        Hv = Hv * alpha.view(-1, 1)
    H = torch.zeros(nc * B, case.d_h, dtype=dtype).index_add(0, b, Hv)
    if case.agg == "mean":
        H = H / torch.bincount(b, minlength=nc * B).clamp(min=1).to(dtype).view(-1, 1)
    elif case.agg == "norm":
        H = H / inp["agg_norm"]
    H = torch.cat([H[c * B:(c + 1) * B] for c in range(nc)], 1)
    if case.bn:
        H = F.batch_norm(H, f("running_mean").clone(), f("running_var").clone(), f("bn_weight"), f("bn_bias"), training=wrong == "batch_stats",
                         momentum=inp["bn_momentum"], eps=inp["bn_eps"])
    Z = H if inp.get("X") is None else torch.cat((H, f("X")), 1)
    out = dict(fingerprint=Z)
    n_lin = len(case.dims) - 1
    for l in range(n_lin):
        Z = F.linear(Z, f(f"W{l}"), f(f"b{l}"))
        if l + 1 < n_lin:
            Z = _act(case.act, Z)
    t = case.n_tasks
    s = f("out_scale") if case.unscale else torch.ones(t, dtype=dtype)
    m = f("out_mean") if case.unscale else torch.zeros(t, dtype=dtype)
    out.update(raw=Z, preds=transform_ref(case.transform, Z, t, case.nc, s, m, wrong))
    if case.kind is not None:
        lt, gt = (inp.get("lt"), inp.get("gt")) if case.bounded else (None, None)
        out["loss"] = criterion(case, Z, f("T"), f("w"), f("tw"), lt, gt)
        out["n_finite"] = float(inp["T"].isfinite().sum())
    return out


def output_names(case: PredictCase) -> list:
    return [n for n in NAMES if n != "loss" or case.kind is not None]


def yardstick(case: PredictCase, inp: dict):
    """(ref64, e32): the float64 reference and, per output, the unfloored error of the float32 restatement against it."""
    r64, r32 = predict_ref(case, inp, torch.float64), predict_ref(case, inp, torch.float32)
    e32 = {k: parity_err_unfloored(r32[k].double().numpy(), r64[k].numpy()) for k in output_names(case)}
    return r64, e32


def bar_of(name: str, e32: float, margin: float) -> float:
    return min(margin * max(e32, EPS32), CAP["loss" if name == "loss" else "preds"])


def compare(case: PredictCase, got: dict, ref: dict, e32: dict, margin: float, report=print, tag: str = "") -> list:
    """Every output of ``got`` against ``ref``: finite wherever the reference is, ``err = max|got - ref| / max|ref|`` within
    ``min(margin max(e32, 2**-23), cap)``.  Reports one line per tensor BEFORE judging; returns the list of failures."""
    fails = []
    for k in output_names(case):
        if got.get(k) is None:
            continue
        g, r = got[k].double().reshape(-1), ref[k].double().reshape(-1)
        assert g.shape == r.shape, (case.id, k, tuple(got[k].shape), tuple(ref[k].shape))
        if not bool(torch.isfinite(g[torch.isfinite(r)]).all()):
            fails.append(f"{k}: not finite where the reference is")
            report(f"PREDBAR {case.id}{tag} {k} nonfinite")
            continue
        err = parity_err_unfloored(g.numpy(), r.numpy())
        scale = float(r.abs().max())
        bar = 0.0 if scale == 0.0 else bar_of(k, e32[k], margin)
        ratio = err / max(e32[k], EPS32)
        report(f"PREDBAR {case.id}{tag} {k} err={err:.3e} e32={e32[k]:.3e} ratio={ratio:.2f} bar={bar:.3e} maxref={scale:.3e}")
        if not err <= bar:
            fails.append(f"{k}: err {err:.3e} > bar {bar:.3e} (fp32 yardstick {e32[k]:.3e}, ratio {ratio:.1f}, max|ref| {scale:.3e})")
    return fails


class Call:
    """The device side of one case: the inputs uploaded once, ``dmpnn_predict_args`` filled, every output NaN-prefilled with ``GUARD``
    rows behind it (the fingerprint's rows ``FP_PAD`` columns longer than ``dims[0]``).  ``run(ready)`` makes one call and returns the
    outputs on the CPU, ``launches`` beside them; ``untouched()`` says whether every guard and every batch-norm buffer is as it was."""

    def __init__(self, case: PredictCase, inp: dict, dev, wsplit: bool = True):
        from chemprop_amd.agg import MODES

        self.case, self.dev, self.lib = case, dev, _lib.load()
        to = lambda k: None if inp.get(k) is None else inp[k].to(dev).contiguous()
        self.keep = keep = {}
        p = self.p = _lib.PredictArgs()
        h = p.head
        Hv, batch = keep.setdefault("Hv", to("Hv")), keep.setdefault("batch", to("batch"))
        dims, n_lin = case.dims, len(case.dims) - 1
        h.n_atoms, h.n_mols, h.d_h, h.batch = int(Hv.shape[0]), case.B, case.d_h, batch.data_ptr()
        h.n_components = case.n_components if case.n_components > 1 else 0
        if case.agg == "attentive":
            keep["att_W"], keep["att_b"] = to("att_W"), to("att_b")
            h.agg_mode, h.att_W, h.att_b = _lib.MOLAGG_ATTENTIVE, keep["att_W"].data_ptr(), keep["att_b"].data_ptr()
        else:
            h.agg_mode, h.agg_norm = MODES[case.agg], float(inp["agg_norm"])
        self.stats = {}
        if case.bn:
            for k in ("bn_weight", "bn_bias", "running_mean", "running_var"):
                keep[k] = to(k)
            keep["nbt"] = torch.tensor(5, dtype=torch.int64, device=dev)
            h.bn_weight, h.bn_bias = keep["bn_weight"].data_ptr(), keep["bn_bias"].data_ptr()
            h.bn_running_mean, h.bn_running_var = keep["running_mean"].data_ptr(), keep["running_var"].data_ptr()
            h.bn_eps, h.bn_momentum, h.bn_num_batches_tracked = float(inp["bn_eps"]), float(inp["bn_momentum"]), keep["nbt"].data_ptr()
            self.stats = {k: keep[k].clone() for k in ("running_mean", "running_var", "nbt")}
        h.n_layers, h.act, h.act_slope = n_lin, _lib.ACT[case.act if case.hidden else "none"], LEAKY_SLOPE if case.act == "leakyrelu" else 0.0
        for l in range(n_lin + 1):
            h.dims[l] = dims[l]
        for l in range(n_lin):
            keep[f"W{l}"], keep[f"b{l}"] = to(f"W{l}"), to(f"b{l}")
            h.W[l], h.b[l] = keep[f"W{l}"].data_ptr(), keep[f"b{l}"].data_ptr()
        if case.d_xd:   # (a view into a wider table: ld_xd > d_xd)
            big = torch.full((case.B, case.d_xd + case.pad_xd), float("nan"), device=dev)
            big[:, :case.d_xd] = inp["X"].to(dev)
            keep["X"] = big
            h.X_d, h.ld_xd = big.data_ptr(), big.stride(0)
        h.n_classes = case.nc
        h.evid_v_kl, h.evid_eps, h.quantile_alpha = 0.2, 1e-8, 0.1
        nan = lambda *s: torch.full(s, float("nan"), device=dev)
        B, w = case.B, case.width
        self.out = dict(raw=nan(B + GUARD, w), preds=nan(B + GUARD, w), fingerprint=nan(B + GUARD, dims[0] + FP_PAD))
        h.preds, p.preds = self.out["raw"].data_ptr(), self.out["preds"].data_ptr()
        p.fingerprint, p.ld_fp = self.out["fingerprint"].data_ptr(), dims[0] + FP_PAD
        p.transform = _lib.PREDICT_TRANSFORM[case.transform]
        if case.unscale:
            keep["out_mean"], keep["out_scale"] = to("out_mean"), to("out_scale")
            p.out_mean, p.out_scale = keep["out_mean"].data_ptr(), keep["out_scale"].data_ptr()
        if case.kind is not None:
            h.loss = _lib.LOSS[case.kind]
            for k in ("T", "w", "tw"):
                keep[k] = to(k)
            h.targets, h.weights, h.task_weights = keep["T"].data_ptr(), keep["w"].data_ptr(), keep["tw"].data_ptr()
            if case.bounded:
                keep["lt"], keep["gt"] = (inp[k].to(torch.uint8).to(dev).contiguous() for k in ("lt", "gt"))
                h.lt_mask, h.gt_mask = keep["lt"].data_ptr(), keep["gt"].data_ptr()
            self.out["loss2"] = nan(2 + GUARD)
            h.loss_out = self.out["loss2"].data_ptr()
        nb = int(self.lib.dmpnn_predict_head_ws_bytes(C.byref(p)))
        assert nb > 0, case.id
        keep["ws"] = torch.empty(nb, dtype=torch.uint8, device=dev)
        h.ws, h.ws_bytes = keep["ws"].data_ptr(), nb
        self.wsplit_bytes = int(self.lib.dmpnn_predict_head_wsplit_bytes(C.byref(p)))
        if wsplit and self.wsplit_bytes:
            keep["wsplit"] = torch.zeros(self.wsplit_bytes + 256, dtype=torch.uint8, device=dev)
            keep["wsplit"][self.wsplit_bytes:] = 0xA5
            p.wsplit, p.wsplit_bytes = keep["wsplit"].data_ptr(), self.wsplit_bytes
        self.launches = None

    def run(self, ready: int = 0) -> dict:
        from chemprop_amd import engine

        c, B = self.case, self.case.B
        self.p.wsplit_ready = ready
        for v in self.out.values():
            v.fill_(float("nan"))
        Hv = self.keep["Hv"]
        with engine._OnDevice(self.dev):
            rc = self.lib.dmpnn_predict_head(C.byref(self.p), Hv.data_ptr(), Hv.stride(0), engine._stream_ptr(self.dev))
        self.launches = int(self.lib.dmpnn_last_launch_count())
        _lib.check(rc, "dmpnn_predict_head")
        torch.cuda.synchronize()
        res = dict(raw=self.out["raw"][:B].cpu(), fingerprint=self.out["fingerprint"][:B, :c.dims[0]].cpu())
        res["preds"] = self.out["preds"][:B].cpu().reshape((B, c.n_tasks) + ((c.per_task,) if c.per_task > 1 else ()))
        if c.kind is not None:
            res["loss"], res["n_finite"] = self.out["loss2"][0].cpu(), float(self.out["loss2"][1])
        return res

    def untouched(self) -> list:
        """What a call must leave alone, as a list of complaints: the guard rows, the pad columns of the fingerprint, the bytes behind
        ``wsplit``, the running statistics and ``num_batches_tracked`` (bit for bit)."""
        B, bad = self.case.B, []
        for k, v in self.out.items():
            if not bool(torch.isnan(v[B:] if k != "loss2" else v[2:]).all()):
                bad.append(f"{k}: guard rows written")
        if not bool(torch.isnan(self.out["fingerprint"][:, self.case.dims[0]:]).all()):
            bad.append("fingerprint: columns beyond dims[0] written")
        if "wsplit" in self.keep and not bool((self.keep["wsplit"][self.wsplit_bytes:] == 0xA5).all()):
            bad.append("wsplit: bytes beyond dmpnn_predict_head_wsplit_bytes written")
        for k, v in self.stats.items():
            same = torch.equal(v, self.keep[k]) if v.dtype == torch.int64 else torch.equal(v.view(torch.int32), self.keep[k].view(torch.int32))
            if not same:
                bad.append(f"{k}: changed")
        return bad


def same_bits(a: dict, b: dict) -> list:
    """Names of the outputs of two calls that differ in any bit (NaN payloads included)."""
    out = []
    for k in a:
        x, y = a[k], b[k]
        if torch.is_tensor(x):
            if not torch.equal(x.reshape(-1).view(torch.int32), y.reshape(-1).view(torch.int32)):
                out.append(k)
        elif not (x == y or (x != x and y != y)):
            out.append(k)
    return out
