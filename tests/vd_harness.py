"""Shared helpers of the atom-descriptor layer's tests (``csrc/dmpnn_vd.hip`` through the C ABI): no fixtures, no pytest settings —
a plain module.

``build_inputs`` makes the layer's inputs as float32 CPU tensors, ``reference`` restates the layer op by op on the CPU in float64
(the reference) or float32 (the yardstick: what plain fp32 PyTorch does on the very same inputs), ``run_layer`` is one
``dmpnn_vd_forward`` + one ``dmpnn_vd_backward`` on the device with every output prefilled with NaN, ``compare`` is the metric and
the bar of ``tests/head_harness.py``: ``max|got - ref| / max|ref|`` within ``min(margin max(e32, 2**-23), cap)``."""
import ctypes as C
import dataclasses

import torch

from chemprop_amd import _lib
from conftest import parity_err_unfloored
from head_harness import CAP, EPS32

OUTPUTS = ("out", "gHv", "gW_d", "gb_d")


@dataclasses.dataclass(frozen=True)
class VdCase:
    n_atoms: int
    d_h: int
    d_vd: int
    pad: int = 0            # every leading dimension = its width + pad
    want_gW: bool = True    # False: gW_d is NULL
    want_gb: bool = True    # False: gb_d is NULL
    mixed: bool = False     # rows of H_v, V_d and gout span ~1e-3 .. 1e3
    seed: int = 0

    @property
    def id(self) -> str:
        return (f"n{self.n_atoms}-h{self.d_h}-vd{self.d_vd}-pad{self.pad}" + ("" if self.want_gW else "-nogW") + ("" if self.want_gb else "-nogb")
                + ("-mixed" if self.mixed else ""))


def build_inputs(case: VdCase) -> dict:
    gen = torch.Generator().manual_seed(1000 + case.seed)
    n, h, v = case.n_atoms, case.d_h, case.d_vd
    D = h + v
    Hv, Vd, gout = torch.randn(n, h, generator=gen), torch.randn(n, v, generator=gen), torch.randn(n, D, generator=gen)
    if case.mixed:
        for t in (Hv, Vd, gout):
            t *= 10.0 ** (6.0 * torch.rand(n, 1, generator=gen) - 3.0)
    # (nn.Linear's own initialisation range, asymmetric on purpose: a kernel that swapped rows and columns of W_d would not pass)
    W = (torch.rand(D, D, generator=gen) * 2 - 1) / D ** 0.5
    b = (torch.rand(D, generator=gen) * 2 - 1) / D ** 0.5
    return dict(Hv=Hv, Vd=Vd, gout=gout, W=W, b=b)


def reference(case: VdCase, inp: dict, dtype=torch.float64) -> dict:
    """``out = cat(Hv, V_d) W_d^T + b_d``, ``gHv = gout W_d[:, :d_h]``, ``gW_d = gout^T cat(Hv, V_d)``, ``gb_d = colsum(gout)``."""
    f = lambda t: t.to(dtype)
    X = torch.cat((f(inp["Hv"]), f(inp["Vd"])), 1)
    W, g = f(inp["W"]), f(inp["gout"])
    return dict(out=X @ W.t() + f(inp["b"]), gHv=g @ W[:, :case.d_h], gW_d=g.t() @ X, gb_d=g.sum(0))


def yardstick(case: VdCase, inp: dict):
    r64, r32 = reference(case, inp, torch.float64), reference(case, inp, torch.float32)
    return r64, {k: parity_err_unfloored(r32[k].double().numpy(), r64[k].numpy()) for k in OUTPUTS}


def _padded(t: torch.Tensor, pad: int, dev, fill=None) -> torch.Tensor:
    """``t`` as a view of a device matrix whose rows are ``pad`` elements longer (the padding holds NaN: a kernel that reads it shows)."""
    buf = torch.full((t.shape[0], t.shape[1] + pad), float("nan"), dtype=torch.float32, device=dev)
    view = buf[:, :t.shape[1]]
    if fill is None:
        view.copy_(t)
    return view


def vd_args(case: VdCase, inp: dict, dev):
    """The filled ``dmpnn_vd_args`` and the tensors it points into (outputs NaN-prefilled)."""
    lib = _lib.load()
    n, h, v = case.n_atoms, case.d_h, case.d_vd
    D = h + v
    t = dict(Hv=_padded(inp["Hv"], case.pad, dev), Vd=_padded(inp["Vd"], case.pad, dev), gout=_padded(inp["gout"], case.pad, dev),
             W=inp["W"].to(dev).contiguous(), b=inp["b"].to(dev).contiguous(),
             out=_padded(torch.empty(n, D), case.pad, dev, fill="nan"), gHv=_padded(torch.empty(n, h), case.pad, dev, fill="nan"),
             gW_d=torch.full((D, D), float("nan"), device=dev), gb_d=torch.full((D,), float("nan"), device=dev))
    a = _lib.VdArgs()
    a.n_atoms, a.d_h, a.d_vd = n, h, v
    a.Hv, a.ldhv = t["Hv"].data_ptr(), h + case.pad
    a.V_d, a.ldvd = t["Vd"].data_ptr(), v + case.pad
    a.W_d, a.b_d = t["W"].data_ptr(), t["b"].data_ptr()
    a.out, a.ldout = t["out"].data_ptr(), D + case.pad
    a.gout, a.ldgout = t["gout"].data_ptr(), D + case.pad
    a.gHv, a.ldghv = t["gHv"].data_ptr(), h + case.pad
    a.gW_d = t["gW_d"].data_ptr() if case.want_gW else None
    a.gb_d = t["gb_d"].data_ptr() if case.want_gb else None
    nb = int(lib.dmpnn_vd_ws_bytes(C.byref(a)))
    assert nb > 0
    t["ws"] = torch.empty(nb, dtype=torch.uint8, device=dev)
    a.ws, a.ws_bytes = t["ws"].data_ptr(), nb
    return a, t


def run_layer(case: VdCase, inp: dict, dev) -> dict:
    """``dmpnn_vd_forward`` then ``dmpnn_vd_backward`` (each on its own: the backward rebuilds the image of ``W_d``); the outputs on
    the CPU by name — a gradient that was not asked for comes back as the NaN it was prefilled with."""
    from chemprop_amd import engine

    lib = _lib.load()
    a, t = vd_args(case, inp, dev)
    with engine._OnDevice(dev):
        _lib.check(lib.dmpnn_vd_forward(C.byref(a), engine._stream_ptr(dev)), "dmpnn_vd_forward")
        t["ws"].fill_(0xFF)   # (nothing of the forward's workspace may be relied on)
        _lib.check(lib.dmpnn_vd_backward(C.byref(a), engine._stream_ptr(dev)), "dmpnn_vd_backward")
    torch.cuda.synchronize()
    return {k: t[k].cpu() for k in OUTPUTS}


def compare(case: VdCase, got: dict, ref: dict, e32: dict, margin: float, report=print) -> list:
    """``head_harness.compare``'s rule per output: finite, ``err = max|got - ref| / max|ref|`` within ``min(margin max(e32, 2**-23),
    cap)`` (``out``: the cap of predictions, the others: of gradients).  One report line per tensor BEFORE judging; returns the
    failures and, last, the worst ``err / max(e32, 2**-23)`` of the case."""
    fails, worst = [], 0.0
    for k in OUTPUTS:
        if (k == "gW_d" and not case.want_gW) or (k == "gb_d" and not case.want_gb):
            if not bool(torch.isnan(got[k]).all()):
                fails.append(f"{k}: written although its pointer was NULL")
            continue
        g, r = got[k].double().reshape(-1), ref[k].double().reshape(-1)
        assert g.shape == r.shape, (case.id, k, tuple(got[k].shape), tuple(ref[k].shape))
        if not bool(torch.isfinite(g).all()):
            fails.append(f"{k}: not finite")
            report(f"VDBAR {case.id} {k} nonfinite")
            continue
        err = parity_err_unfloored(g.numpy(), r.numpy())
        scale = float(r.abs().max()) if r.numel() else 0.0
        bar = 0.0 if scale == 0.0 else min(margin * max(e32[k], EPS32), CAP["preds" if k == "out" else "grad"])
        ratio = err / max(e32[k], EPS32)
        worst = max(worst, ratio)
        report(f"VDBAR {case.id} {k} err={err:.3e} e32={e32[k]:.3e} ratio={ratio:.2f} bar={bar:.3e} maxref={scale:.3e}")
        if not err <= bar:
            fails.append(f"{k}: err {err:.3e} > bar {bar:.3e} (fp32 yardstick {e32[k]:.3e}, ratio {ratio:.1f}, max|ref| {scale:.3e})")
    return fails, worst
