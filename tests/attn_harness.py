"""Shared by the attentive-aggregation tests (plain helpers: no fixtures, no pytest settings).

The kernels through the C ABI (``dmpnn_molagg_attn_fwd`` / ``_bwd``) and ``dmpnn_head`` in attentive mode against float64 restatements
on the CPU: ``oracle.agg_torch.attentive`` (it follows the dtype of ``H``) with gradients from autograd.

Bars (the suite's convention, ``head_harness.compare``): per tensor ``err = max|got - ref64| / max|ref64|`` within ``min(MARGIN max(e32,
2**-23), cap)``, ``e32`` the same quantity for the float32 run of the restatement, caps 1e-5 (outputs) / 2e-5 (gradients).  ``gb`` is
analytically zero (the softmax is shift invariant); its bar is absolute: ``|gb| <= MARGIN 2**-23 sum_v |dl_v|``, the sum from float64.
"""
import ctypes as C
import dataclasses
import math
import os

import torch

import head_harness as hh
from chemprop_amd import _lib
from conftest import parity_err_unfloored

F = torch.nn.functional
MARGIN = 32.0
EPS32 = 2.0 ** -23
CAP_OUT, CAP_GRAD = 1e-5, 2e-5
MAX_LOGIT = 30.0

# capacities of the kernels (dmpnn_attn.hip): a row of up to NARROW_VEC columns as 16-byte quads (NARROW_SCALAR as single floats) stays in
# registers; wider rows take column passes, on which the first STAGE_ATOMS atoms of a molecule keep their logit term in LDS
STAGE_ATOMS = 128
NARROW_VEC, NARROW_SCALAR = 1024, 256
PARTIAL_ROWS = 1024   # partial rows of gW | gb: beyond that many molecules a wave walks several

BASE_SIZES = (1, 2, 9, 0, 31, 64, 65, 3)
BEYOND_STAGE = (3, STAGE_ATOMS + 1, 0, 2)


@dataclasses.dataclass(frozen=True)
class AggCase:
    """One forward + backward of the kernels.  ``sizes``: atoms per molecule; ``extra_mols``: molecules without atoms behind
    ``batch.max()``; ``pad``: columns of NaN padding behind every row of H / out / gout / gH (row stride ``d + pad``); ``offset``: floats
    the base pointers of H / out / gout / gH are shifted by (unaligned rows); ``scale``: factor on the ``randn`` rows."""
    id: str
    sizes: tuple
    d: int
    extra_mols: int = 0
    pad: int = 0
    offset: int = 0
    scale: float = 1.0
    seed: int = 0

    @property
    def n_mols(self):
        return len(self.sizes) + self.extra_mols

    @property
    def vector(self):
        return self.d % 4 == 0 and self.pad % 4 == 0 and self.offset % 4 == 0


def agg_cases():
    cs = [AggCase(f"d{d}", BASE_SIZES, d) for d in (1, 4, 6, 301, 44, 256, 300, 1024, 2400)]
    cs += [AggCase("d300-x4", BASE_SIZES, 300, scale=4.0), AggCase("d44-x4", BASE_SIZES, 44, scale=4.0),
           AggCase("one-mol", (7,), 300), AggCase("extra-mols", BASE_SIZES, 44, extra_mols=3),
           AggCase("pad4-d300", BASE_SIZES, 300, pad=4), AggCase("pad1-d300", BASE_SIZES, 300, pad=1), AggCase("pad3-d6", BASE_SIZES, 6, pad=3),
           AggCase("offset1-d300", BASE_SIZES, 300, offset=1),
           # one atom beyond the LDS stage on both column-pass forms (quads: d > NARROW_VEC; single floats: d > NARROW_SCALAR)
           AggCase("stage+1-vec", BEYOND_STAGE, NARROW_VEC + 4), AggCase("stage+1-scalar", BEYOND_STAGE, NARROW_SCALAR + 1),
           AggCase("stage+1-narrow", BEYOND_STAGE, 300)]
    return cs


def batch_of(sizes) -> torch.Tensor:
    return torch.repeat_interleave(torch.arange(len(sizes)), torch.tensor(sizes, dtype=torch.int64))


def build(case: AggCase) -> dict:
    """float32 CPU inputs: ``H = scale randn``, ``W`` / ``b`` in ``nn.Linear``'s default range, ``gout = randn``.  Asserts the
    harness's precondition: ``max|logit| <= MAX_LOGIT`` in float64 (exp stays far inside fp32)."""
    gen = torch.Generator().manual_seed(500 + case.seed)
    batch = batch_of(case.sizes)
    nV, d = int(batch.numel()), case.d
    k = 1.0 / math.sqrt(d)
    inp = dict(batch=batch, n_mols=case.n_mols, H=case.scale * torch.randn(nV, d, generator=gen),
               W=(2 * torch.rand(1, d, generator=gen) - 1) * k, b=(2 * torch.rand(1, generator=gen) - 1) * k,
               gout=torch.randn(case.n_mols, d, generator=gen))
    logit = F.linear(inp["H"].double(), inp["W"].double(), inp["b"].double())
    inp["max_logit"] = float(logit.abs().max()) if nV else 0.0
    assert inp["max_logit"] <= MAX_LOGIT, (case.id, inp["max_logit"])
    assert nV > 0 and batch.numel() == sum(case.sizes)
    return inp


def attentive(H, batch, W, b, n_mols):
    """``oracle.agg_torch.attentive`` with the rows of the molecules behind ``batch.max()`` (zero, like every molecule without atoms)."""
    from oracle import agg_torch as oa

    out = oa.attentive(H, batch, W, b)
    if out.shape[0] < n_mols:
        out = torch.cat((out, torch.zeros(n_mols - out.shape[0], H.shape[1], dtype=H.dtype)))
    return out


def reference(inp: dict, dtype=torch.float64) -> dict:
    H, W, b = (inp[k].detach().to(dtype).clone().requires_grad_(True) for k in ("H", "W", "b"))   # (copies: the inputs stay as they are)
    out = attentive(H, inp["batch"], W, b, inp["n_mols"])
    (out * inp["gout"].to(dtype)).sum().backward()
    r = dict(out=out.detach(), gH=H.grad, gW=W.grad.reshape(-1), gb=b.grad.reshape(-1))
    # sum_v |dl_v| (the scale of gb's rounding): dl_v = alpha_v (a_v - c_m)
    with torch.no_grad():
        s = F.linear(H, W, b).exp().reshape(-1)
        Z = torch.zeros(inp["n_mols"], dtype=dtype).index_add(0, inp["batch"], s)
        al = s / Z[inp["batch"]]
        a = (inp["gout"].to(dtype)[inp["batch"]] * H).sum(1)
        c = torch.zeros(inp["n_mols"], dtype=dtype).index_add(0, inp["batch"], al * a)
        r["sum_abs_dl"] = float((al * (a - c[inp["batch"]])).abs().sum())
    return r


def yardstick(inp: dict):
    """(ref64, e32): the float64 restatement and, per tensor, the error of its float32 run."""
    r64, r32 = reference(inp, torch.float64), reference(inp, torch.float32)
    e32 = {k: parity_err_unfloored(r32[k].double().numpy(), r64[k].numpy()) for k in ("out", "gH", "gW")}
    e32["gb_abs"] = abs(float(r32["gb"])) / max(r64["sum_abs_dl"], 1e-300)
    return r64, e32


def _strided(t: torch.Tensor, pad: int, offset: int, dev):
    """``t`` on the device inside a NaN-filled buffer: rows ``pad`` columns apart, the first one ``offset`` floats into the buffer.
    Returns ``(view [n, d], buffer)``."""
    n, d = t.shape
    ld = d + pad
    buf = torch.full((offset + max(n, 1) * ld,), float("nan"), dtype=torch.float32, device=dev)
    view = buf[offset:offset + n * ld].view(n, ld)[:, :d] if n else buf[offset:offset].view(0, d)
    view.copy_(t.to(dev))
    return view, buf


def padding_untouched(view: torch.Tensor, buf: torch.Tensor) -> bool:
    """Everything of ``buf`` outside ``view`` is still NaN."""
    mask = torch.ones_like(buf, dtype=torch.bool)
    n, d = view.shape
    if n:
        off = view.storage_offset() - buf.storage_offset()
        idx = (off + torch.arange(n, device=buf.device).view(-1, 1) * view.stride(0) + torch.arange(d, device=buf.device).view(1, -1)).reshape(-1)
        mask[idx] = False
    return bool(torch.isnan(buf[mask]).all())


def bounds_table(batch_dev: torch.Tensor, n_mols: int):
    from chemprop_amd import engine

    lib = _lib.load()
    nb = int(lib.dmpnn_molagg_ws_bytes(n_mols))
    ws = torch.empty(max(nb, 16), dtype=torch.uint8, device=batch_dev.device)
    with engine._OnDevice(batch_dev.device):
        _lib.check(lib.dmpnn_molagg_bounds(batch_dev.data_ptr(), int(batch_dev.numel()), n_mols, ws.data_ptr(), nb,
                                           engine._stream_ptr(batch_dev.device)), "dmpnn_molagg_bounds")
    return ws


def run(inp: dict, dev, pad: int = 0, offset: int = 0, keep: bool = True, backward: bool = True, want_gW: bool = True, want_gb: bool = True,
        own_bounds: bool = False) -> dict:
    """Forward (+ backward) through the C ABI, every output prefilled with NaN.  Returns the outputs on the CPU and ``padding_ok``
    (the NaN padding of every strided buffer came back untouched).  ``own_bounds``: ``bounds == NULL`` — the table is built from
    ``batch`` at the head of ``ws``."""
    from chemprop_amd import engine

    lib = _lib.load()
    n_mols, (nV, d) = inp["n_mols"], inp["H"].shape
    batch = inp["batch"].to(dev)
    H, Hbuf = _strided(inp["H"], pad, offset, dev)
    gout, gobuf = _strided(inp["gout"], pad, offset, dev)
    out, obuf = _strided(torch.full((n_mols, d), float("nan")), pad, offset, dev)
    gH, gHbuf = _strided(torch.full((nV, d), float("nan")), pad, offset, dev)
    W, b = inp["W"].reshape(-1).to(dev).contiguous(), inp["b"].reshape(-1).to(dev).contiguous()
    gW, gb = torch.full((d,), float("nan"), device=dev), torch.full((1,), float("nan"), device=dev)
    s, Z = torch.full((max(nV, 1),), float("nan"), device=dev), torch.full((max(n_mols, 1),), float("nan"), device=dev)
    a = _lib.MolAggAttnArgs()
    a.n_atoms, a.n_mols, a.d_h = nV, n_mols, d
    a.H, a.ldh, a.batch = H.data_ptr(), d + pad, batch.data_ptr()
    table = None if own_bounds else bounds_table(batch, n_mols)
    a.bounds = None if own_bounds else table.data_ptr()
    a.W, a.b = W.data_ptr(), b.data_ptr()
    a.out, a.ldo = out.data_ptr(), d + pad
    if keep:
        a.keep_s, a.keep_Z = s.data_ptr(), Z.data_ptr()
    a.gout, a.ldgo, a.gH, a.ldgh = gout.data_ptr(), d + pad, gH.data_ptr(), d + pad
    a.gW, a.gb = (gW.data_ptr() if want_gW else None), (gb.data_ptr() if want_gb else None)
    nb = int(lib.dmpnn_molagg_attn_ws_bytes(C.byref(a)))
    ws = torch.empty(max(nb, 16), dtype=torch.uint8, device=dev)
    a.ws, a.ws_bytes = ws.data_ptr(), nb
    with engine._OnDevice(dev):
        st = engine._stream_ptr(dev)
        n0 = int(lib.dmpnn_last_launch_count())
        _lib.check(lib.dmpnn_molagg_attn_fwd(C.byref(a), st), "dmpnn_molagg_attn_fwd")
        n_fwd = int(lib.dmpnn_last_launch_count()) - n0   # (launches of the forward call itself)
        if backward:
            assert keep
            _lib.check(lib.dmpnn_molagg_attn_bwd(C.byref(a), st), "dmpnn_molagg_attn_bwd")
    torch.cuda.synchronize()
    res = dict(out=out.cpu().contiguous(), s=s.cpu(), Z=Z.cpu(), n_fwd=n_fwd,
               padding_ok=padding_untouched(out, obuf) and padding_untouched(H, Hbuf) and padding_untouched(gout, gobuf))
    if backward:
        res.update(gH=gH.cpu().contiguous(), gW=gW.cpu(), gb=gb.cpu())
        res["padding_ok"] = res["padding_ok"] and padding_untouched(gH, gHbuf)
    return res


def compare(cid: str, got: dict, ref: dict, e32: dict, names=("out", "gH", "gW", "gb"), report=print) -> list:
    """One line per tensor BEFORE judging; returns the failures (empty: all held)."""
    fails = []
    for k in names:
        if k == "gb":
            v, scale = abs(float(got["gb"])), ref["sum_abs_dl"]
            bar = MARGIN * EPS32 * scale
            report(f"ATTNBAR {cid} gb |gb|={v:.3e} bar={bar:.3e} sum|dl|={scale:.3e} fp32-restatement={e32['gb_abs'] / EPS32:.2f} eps sum|dl|")
            if not v <= bar:
                fails.append(f"gb: |gb| {v:.3e} > {bar:.3e}")
            continue
        g, r = got[k].double().reshape(-1), ref[k].double().reshape(-1)
        assert g.shape == r.shape, (cid, k, tuple(got[k].shape), tuple(ref[k].shape))
        if not bool(torch.isfinite(g).all()):
            report(f"ATTNBAR {cid} {k} nonfinite")
            fails.append(f"{k}: not finite")
            continue
        err = parity_err_unfloored(g.numpy(), r.numpy())
        scale = float(r.abs().max())
        bar = 0.0 if scale == 0.0 else min(MARGIN * max(e32[k], EPS32), CAP_OUT if k == "out" else CAP_GRAD)
        report(f"ATTNBAR {cid} {k} err={err:.3e} e32={e32[k]:.3e} bar={bar:.3e} maxref={scale:.3e}")
        if not err <= bar:
            fails.append(f"{k}: err {err:.3e} > bar {bar:.3e} (fp32 yardstick {e32[k]:.3e})")
    return fails


# ---- dmpnn_head in attentive mode ---------------------------------------------------------------------------------------------
def head_case(cid, B, d_h, bn=True, d_xd=0, mode="train", hidden=(16,), tasks=2, seed=0) -> hh.HeadCase:
    """Molecules of 1 .. 3 atoms, a tanh predictor (no kink can flip), MSE with some targets missing."""
    return hh.HeadCase(cid, "default", B, d_h, hidden, tasks, kind="mse", act="tanh", agg="sum", bn=bn, d_xd=d_xd, mode=mode, seed=seed)


def head_cases():
    # B = 2 runs WITHOUT batch norm in training mode: over two molecules batch norm's output is gamma * (+1 | -1) + beta whatever
    # its input, so every gradient behind it is the remainder eps / (var + eps) of a cancellation (max|gHv| 6e-5 under weight
    # gradients of 1e-1), and the float32 run of the restatement itself stands 1.1e-4 (gHv) and 7.1e-5 (g_att_W) from float64 —
    # beyond the 2e-5 cap before any kernel is involved.  Batch norm at B = 2 is held on its running statistics ("B2-bn-infer").
    cs = [head_case("B2", 2, 8, bn=False), head_case("B2-bn-infer", 2, 8, mode="infer")]
    cs += [head_case(f"B{B}", B, 8) for B in (64, 513, 1025)]
    cs += [head_case("d300", 64, 300), head_case("d37", 64, 37), head_case("no-bn", 64, 8, bn=False), head_case("d300-no-bn", 33, 300, bn=False),
           head_case("xd3", 64, 8, d_xd=3), head_case("infer", 64, 8, mode="infer"), head_case("d300-B513", 513, 300)]
    return cs


MIN_BN_VAR = 1e-2   # (1 000 times batch norm's eps)


def head_inputs(case: hh.HeadCase) -> dict:
    """``head_harness.build_inputs`` on a batch of 1 .. 3 atoms per molecule, plus the attention's ``att_W`` / ``att_b``.
    Preconditions, asserted in float64: ``max|logit| <= MAX_LOGIT``; with batch norm, every column of the aggregate has a batch
    variance of at least ``MIN_BN_VAR`` — batch norm's backward pass forms ``1 - xhat**2 var / (var + eps)``-like differences whose
    condition number grows like ``1 / var``, so on a column whose aggregates nearly coincide (two molecules: a difference of 0.04
    gives var 3e-4) half an ulp on ``H_v`` already moves ``gHv`` by 8e-6 of its maximum in float64 arithmetic, and the case would
    measure batch norm's conditioning instead of the attention.  The input seed advances until both hold (``inp["input_seed"]``)."""
    base = hh.build_inputs(case)
    k = 1.0 / math.sqrt(case.d_h)
    for seed in range(case.seed, case.seed + 50):
        gen = torch.Generator().manual_seed(900 + seed)
        inp = dict(base)
        counts = torch.randint(1, 4, (case.B,), generator=gen)
        inp["batch"] = torch.repeat_interleave(torch.arange(case.B), counts)
        inp["Hv"] = torch.randn(int(counts.sum()), case.d_h, generator=gen)
        inp["att_W"] = (2 * torch.rand(1, case.d_h, generator=gen) - 1) * k
        inp["att_b"] = (2 * torch.rand(1, generator=gen) - 1) * k
        logit = F.linear(inp["Hv"].double(), inp["att_W"].double(), inp["att_b"].double())
        A = attentive(inp["Hv"].double(), inp["batch"], inp["att_W"].double(), inp["att_b"].double(), case.B)
        if float(logit.abs().max()) <= MAX_LOGIT and (not case.bn or float(A.var(0, unbiased=False).min()) >= MIN_BN_VAR):
            break
    else:
        raise AssertionError(f"{case.id}: no input seed meets the preconditions")
    inp["input_seed"], inp["min_var"] = seed, float(A.var(0, unbiased=False).min())
    return inp


def head_reference(case: hh.HeadCase, inp: dict, dtype=torch.float64) -> dict:
    """``head_harness.reference`` with the aggregation swapped: the attentive aggregate is handed to it as a batch of one-atom
    molecules under SUM (an exact identity), inside one autograd graph."""
    grad = case.mode == "train"
    Hv, W, b = (inp[k].detach().to(dtype).clone().requires_grad_(grad) for k in ("Hv", "att_W", "att_b"))   # (copies)
    A = attentive(Hv, inp["batch"], W, b, case.B)
    if not grad:
        A = A.detach()

    sub = dict(inp)
    sub["batch"] = torch.arange(case.B)
    holder = _Leaf(A)
    sub["Hv"] = holder
    out = hh.reference(case, sub, dtype)
    if grad:
        A.backward(holder.leaf.grad)   # (the head's gradient of the aggregate, on through the attention)
        out["gHv"] = Hv.grad
        out["g_att_W"], out["g_att_b"] = W.grad.reshape(-1), b.grad.reshape(-1)
        with torch.no_grad():
            gA = holder.leaf.grad
            s = F.linear(Hv, W, b).exp().reshape(-1)
            Z = torch.zeros(case.B, dtype=dtype).index_add(0, inp["batch"], s)
            al = s / Z[inp["batch"]]
            a = (gA[inp["batch"]] * Hv).sum(1)
            c = torch.zeros(case.B, dtype=dtype).index_add(0, inp["batch"], al * a)
            out["sum_abs_dl"] = float((al * (a - c[inp["batch"]])).abs().sum())
    return out


class _Leaf:
    """Stands in for ``inp["Hv"]`` in ``head_harness.reference``: ``.to(dtype).requires_grad_(grad)`` gives a leaf holding the
    aggregate's values, whose gradient ``head_reference`` pushes on through the attention's graph."""

    def __init__(self, A):
        self.A, self.leaf = A, None

    def to(self, dtype):
        return self

    def requires_grad_(self, grad):
        self.leaf = self.A.detach().clone().requires_grad_(grad)
        return self.leaf


def head_output_names(case: hh.HeadCase) -> list:
    return hh.output_names(case) + (["g_att_W"] if case.mode == "train" else [])


def head_yardstick(case, inp):
    r64, r32 = head_reference(case, inp, torch.float64), head_reference(case, inp, torch.float32)
    e32 = {k: parity_err_unfloored(r32[k].double().numpy(), r64[k].numpy()) for k in head_output_names(case)}
    return r64, e32


def run_head(case: hh.HeadCase, inp: dict, dev, env=None) -> dict:
    """``dmpnn_head`` with ``agg_mode = DMPNN_MOLAGG_ATTENTIVE``: ``head_harness.run_case`` builds every other field; the mode and the
    four attention fields are set by wrapping ``dmpnn_head_ws_bytes`` (its first use of the finished argument block)."""
    lib = _lib.load()
    aW, ab = inp["att_W"].reshape(-1).to(dev).contiguous(), inp["att_b"].reshape(-1).to(dev).contiguous()
    gaW, gab = torch.full((case.d_h,), float("nan"), device=dev), torch.full((1,), float("nan"), device=dev)

    class _Lib:
        def __getattr__(self, name):
            return getattr(lib, name)

        def dmpnn_head_ws_bytes(self, href):
            h = href._obj
            h.agg_mode = _lib.MOLAGG_ATTENTIVE
            h.att_W, h.att_b = aW.data_ptr(), ab.data_ptr()
            if case.mode == "train":
                h.g_att_W, h.g_att_b = gaW.data_ptr(), gab.data_ptr()
            return lib.dmpnn_head_ws_bytes(href)

    load = _lib.load
    try:
        _lib.load = lambda: _Lib()
        res = hh.run_case(case, inp, dev, env)
    finally:
        _lib.load = load
    if case.mode == "train":
        res["g_att_W"], res["g_att_b"] = gaW.cpu(), gab.cpu()
    return res


def compare_head(case, got, ref, e32, report=print) -> list:
    names = head_output_names(case)
    fails = []
    for k in names:
        g, r = got[k].double().reshape(-1), ref[k].double().reshape(-1)
        assert g.shape == r.shape, (case.id, k)
        if not bool(torch.isfinite(g).all()):
            report(f"ATTNHEAD {case.id} {k} nonfinite")
            fails.append(f"{k}: not finite")
            continue
        err = parity_err_unfloored(g.numpy(), r.numpy())
        scale = float(r.abs().max())
        bar = 0.0 if scale == 0.0 else min(MARGIN * max(e32[k], EPS32), hh.cap_of(k))
        report(f"ATTNHEAD {case.id} {k} err={err:.3e} e32={e32[k]:.3e} bar={bar:.3e} maxref={scale:.3e}")
        if not err <= bar:
            fails.append(f"{k}: err {err:.3e} > bar {bar:.3e} (fp32 yardstick {e32[k]:.3e})")
    if case.mode == "train":
        v, bar = abs(float(got["g_att_b"])), MARGIN * EPS32 * ref["sum_abs_dl"]
        report(f"ATTNHEAD {case.id} g_att_b |gb|={v:.3e} bar={bar:.3e}")
        if not v <= bar:
            fails.append(f"g_att_b: |gb| {v:.3e} > {bar:.3e}")
    return fails
