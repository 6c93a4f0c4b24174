"""Shared helpers of ``tests/test_flat_boundaries.py``: the readout, clip and Adam entries of ``include/dmpnn.h`` through ctypes with
the LAYOUT in the caller's hands, and their references on the CPU — no fixtures, no pytest settings, a plain module in the style of
``tests/rows_harness.py`` (whose ``Mat``, ``_call`` and constants it imports).

* ``run_bounds`` / ``run_molagg_fwd`` / ``run_molagg_bwd`` / ``run_adam`` / ``run_clip``: one C call each.  Every float operand is a
  ``Mat`` with its own leading dimension and element offset (a flat buffer: one row); inputs carry NaN in their padding; an output
  or an in-place buffer lives in a ``PREFILL``-filled allocation whose padding and guard words ``Mat.read`` wants back bit for bit.
  ``Workspace``: exactly ``dmpnn_molagg_ws_bytes(n_mols)`` / ``dmpnn_clip_grad_ws_bytes()`` bytes at the front of a larger prefilled
  allocation, read back as integer words.
* ``bounds_ref`` / ``molagg_ref`` / ``molagg_bwd_ref`` / ``adam_ref`` / ``clip_ref``: plain loops and formulas.  The float32 run of
  ``molagg_ref`` / ``molagg_bwd_ref`` and the value mode of ``clip_ref`` are what the kernels promise BIT FOR BIT (rows added in
  increasing atom order, the first addend copied, one true division); the float64 runs of ``adam_ref`` and of ``clip_ref``'s norm
  mode are what the arithmetic outputs are held to with the rule of ``rows_harness.compare``.
"""
import numpy as np
import torch

from chemprop_amd import _lib
from rows_harness import EINVAL, EPS32, GUARD, MARGIN, PREFILL, Mat, _call  # noqa: F401  (re-exported: one set of constants)

SUM, MEAN, NORM = 0, 1, 2          # enum dmpnn_molagg_mode
CLIP_NORM, CLIP_VALUE = 0, 1       # enum dmpnn_clip_mode
POISON = 0x7FC00000                # the library's own NaN: what an invalid batch vector leaves in every output word
CLIP_PARTIALS = 256                # ws of dmpnn_clip_grad: partial[256] | total | 3 words never written


def f32(x) -> float:
    """``x`` rounded to float32, as a Python float: what a ``float`` argument of the ABI receives."""
    return float(np.float32(x))


def bits(t):
    return t.contiguous().view(torch.int32)


# ---- workspaces ------------------------------------------------------------------------------------------------------------------------
class Workspace:
    """``n_bytes`` (a multiple of 4) of workspace at the front of an int32 allocation of ``n_bytes / 4 + GUARD`` words, every word
    ``PREFILL`` (torch's allocations are at least 256-byte aligned)."""

    def __init__(self, dev, n_bytes):
        assert n_bytes % 4 == 0
        self.words = n_bytes // 4
        self.n_bytes = n_bytes
        self.base = torch.full((self.words + GUARD,), PREFILL, dtype=torch.int32, device=dev)
        self.ptr = self.base.data_ptr()

    def cpu(self) -> torch.Tensor:
        """The workspace's own words (int32, on the CPU)."""
        return self.base[:self.words].cpu()

    def guard_ok(self) -> bool:
        return bool((self.base[self.words:] == PREFILL).all())

    def pristine(self) -> bool:
        return bool((self.base == PREFILL).all())


def bounds_tables(ws: Workspace, n_mols):
    """``first | end | flag | 3 words of padding | done`` of a bounds workspace as Python data."""
    w = ws.cpu()
    assert w.numel() == 3 * n_mols + 4
    n = n_mols
    return dict(first=w[:n], end=w[n:2 * n], flag=int(w[2 * n]), pad=w[2 * n + 1:2 * n + 4], done=w[2 * n + 4:])


# ---- dmpnn_molagg_bounds -----------------------------------------------------------------------------------------------------------------
def batch_of(counts) -> torch.Tensor:
    """The sorted int64 batch vector of molecules with ``counts[m]`` atoms."""
    return torch.repeat_interleave(torch.arange(len(counts), dtype=torch.int64), torch.as_tensor(counts, dtype=torch.int64))


def bounds_ref(batch, n_mols):
    """``first[m]`` / ``end[m]``: the first and one past the last atom of molecule ``m`` (0 / 0 without atoms), and whether the vector
    is valid (every id in ``[0, n_mols)``, non-decreasing) — by a plain loop.  The tables of an invalid vector are not specified."""
    first, end = [0] * n_mols, [0] * n_mols
    valid, prev = True, -1
    for v, b in enumerate(batch.tolist()):
        if b < 0 or b >= n_mols:
            valid = False
            continue
        if b < prev:
            valid = False
        if b != prev:
            first[b] = v
        end[b] = v + 1
        prev = b
    return torch.tensor(first, dtype=torch.int32), torch.tensor(end, dtype=torch.int32), valid


def run_bounds(dev, batch, n_mols, ws_short=0, null_batch=False, n_atoms=None):
    """One ``dmpnn_molagg_bounds`` call on ``batch`` (int64, CPU; ``n_atoms``: what the call is told, default its length) ->
    ``rc``, ``msg``, ``launches``, the ``Workspace`` and the batch on the device."""
    lib = _lib.load()
    bd = batch.to(torch.int64).to(dev)
    ws = Workspace(dev, int(lib.dmpnn_molagg_ws_bytes(n_mols)))
    n = int(batch.numel()) if n_atoms is None else n_atoms
    rc, msg, launches = _call(dev, lib.dmpnn_molagg_bounds, None if (null_batch or bd.numel() == 0) else bd.data_ptr(), n, n_mols, ws.ptr,
                              ws.n_bytes - ws_short)
    return dict(rc=rc, msg=msg, launches=launches, ws=ws, batch=bd)


# ---- dmpnn_molagg_fwd / dmpnn_molagg_bwd ---------------------------------------------------------------------------------------------------
def _counts(batch, n_mols, dtype):
    return torch.bincount(batch, minlength=n_mols)[:n_mols].to(dtype).view(-1, 1)


def molagg_ref(H, batch, n_mols, mode, norm=1.0, dtype=torch.float32):
    """Per-molecule sum / mean / ``sum / norm`` of the rows of ``H`` in ``dtype``: rows added in increasing atom order, THE FIRST ADDEND
    COPIED (``scatter_reduce_(include_self=False)``: a lone ``-0.0`` stays ``-0.0``), then one true division by a tensor operand (no
    multiplication by a reciprocal); molecules without atoms give zero rows, the mean included.  In float32 this is the kernel's
    promise, bit for bit; in float64 it only serves the report."""
    H = H.to(dtype)
    out = torch.zeros(n_mols, H.shape[1], dtype=dtype)
    seen = [False] * n_mols
    for v, m in enumerate(batch.tolist()):
        out[m] = H[v] if not seen[m] else out[m] + H[v]
        seen[m] = True
    if mode == MEAN:
        cnt = _counts(batch, n_mols, dtype)
        out = torch.where(cnt > 0, out / cnt.clamp(min=1).expand_as(out), out)
    elif mode == NORM:
        out = out / torch.full_like(out, f32(norm))
    else:
        assert mode == SUM
    return out


def molagg_bwd_ref(G, batch, n_mols, mode, norm=1.0, dtype=torch.float32):
    """``gH[v] = G[batch[v]]`` (mean: / the molecule's own count, norm: / ``norm``; one true division) in ``dtype``."""
    gH = G.to(dtype)[batch]
    if mode == MEAN:
        gH = gH / _counts(batch, n_mols, dtype)[batch].expand_as(gH)
    elif mode == NORM:
        gH = gH / torch.full_like(gH, f32(norm))
    else:
        assert mode == SUM
    return gH


def run_molagg_fwd(dev, H, ws: Workspace, n_mols, mode, norm=1.0, ldh=None, ldo=None, off_h=0, off_o=0, say=None):
    """One ``dmpnn_molagg_fwd`` call on the tables of ``ws`` -> (rc, msg, the output ``Mat`` of ``[n_mols, d_h]``).  ``say``: arguments
    the call is told instead of the true ones (``ldh``, ``ldo``, ``d_h``, ``n_mols``, ``mode``: the argument-error cases)."""
    lib = _lib.load()
    say = dict(say or {})
    V, d = int(H.shape[0]), int(H.shape[1])
    mh, mo = Mat(dev, V, d, ldh, off_h, H), Mat(dev, n_mols, d, ldo, off_o)
    rc, msg, _ = _call(dev, lib.dmpnn_molagg_fwd, mh.ptr, say.get("ldh", mh.ld), V, say.get("d_h", d), say.get("n_mols", n_mols), ws.ptr,
                       say.get("mode", mode), norm, mo.ptr, say.get("ldo", mo.ld))
    return rc, msg, mo


def run_molagg_bwd(dev, G, batch_dev, ws: Workspace, n_mols, mode, norm=1.0, ldg=None, ldgh=None, off_g=0, off_gh=0):
    """One ``dmpnn_molagg_bwd`` call -> (rc, msg, the output ``Mat`` of ``[n_atoms, d_h]``); ``G``: ``[n_mols, d_h]``."""
    lib = _lib.load()
    V, d = int(batch_dev.numel()), int(G.shape[1])
    mg, mo = Mat(dev, n_mols, d, ldg, off_g, G), Mat(dev, V, d, ldgh, off_gh)
    rc, msg, _ = _call(dev, lib.dmpnn_molagg_bwd, mg.ptr, mg.ld, batch_dev.data_ptr() if V else None, V, d, n_mols, ws.ptr, mode, norm,
                       mo.ptr, mo.ld)
    return rc, msg, mo


# ---- dmpnn_adam_step -----------------------------------------------------------------------------------------------------------------------
def adam_hyper(lr, beta1, beta2, eps, wd, step, grad_scale=1.0):
    """The scalar arguments of ``dmpnn_adam_step`` at optimizer step ``step`` (1-based), as ``chemprop_amd.optim`` forms them."""
    return dict(lr=lr, beta1=beta1, beta2=beta2, eps=eps, wd=wd, bc1=1.0 - beta1 ** step, sqrt_bc2=(1.0 - beta2 ** step) ** 0.5,
                grad_scale=grad_scale)


def adam_ref(p, g, m, v, hyper, dtype=torch.float64):
    """The four lines of the header comment of ``dmpnn_optim.hip`` in ``dtype`` -> ``(p, m, v)`` after the step.  Every scalar is
    first rounded to float32, as the ABI receives it."""
    h = {k: f32(x) for k, x in hyper.items()}
    p, g, m, v = (t.to(dtype) for t in (p, g, m, v))
    gr = g * h["grad_scale"] + h["wd"] * p
    m = h["beta1"] * m + (1.0 - h["beta1"]) * gr
    v = h["beta2"] * v + (1.0 - h["beta2"]) * gr * gr
    p = p - (h["lr"] / h["bc1"]) * m / (v.sqrt() / h["sqrt_bc2"] + h["eps"])
    return p, m, v


def torch_adam(p, g, m, v, hyper, step, dtype, lr=None, eps=None):
    """One ``torch.optim.Adam(foreach=False)`` step in ``dtype`` from the state ``(m, v)`` after ``step - 1`` steps -> ``(p, m, v)``.
    torch forms its own bias corrections from ``step``; the gradient it sees is ``g grad_scale``."""
    h = {k: f32(x) for k, x in hyper.items()}
    P = torch.nn.Parameter(p.to(dtype).clone())
    opt = torch.optim.Adam([P], lr=h["lr"] if lr is None else lr, betas=(h["beta1"], h["beta2"]), eps=h["eps"] if eps is None else eps,
                           weight_decay=h["wd"], foreach=False)
    opt.state[P] = dict(step=torch.tensor(float(step - 1)), exp_avg=m.to(dtype).clone(), exp_avg_sq=v.to(dtype).clone())
    P.grad = g.to(dtype) * h["grad_scale"]
    opt.step()
    st = opt.state[P]
    return P.detach(), st["exp_avg"], st["exp_avg_sq"]


ADAM_BUFFERS = ("p", "g", "m", "v")


def run_adam(dev, p, g, m, v, hyper, n=None, off=None, dev_scalars=False):
    """One ``dmpnn_adam_step`` call on flat float32 CPU tensors -> (rc, msg, {name: Mat}).  ``off``: element offset per buffer name;
    ``n``: what the call is told (default the length); ``dev_scalars``: lr, bc1, sqrt_bc2 and grad_scale travel in a device array and
    the arguments hold garbage (NaN, NaN, NaN and 9)."""
    lib = _lib.load()
    off = dict(off or {})
    mats = {k: Mat(dev, 1, int(t.numel()), None, off.get(k, 0), t.view(1, -1)) for k, t in zip(ADAM_BUFFERS, (p, g, m, v))}
    h = dict(hyper)
    ds = None
    if dev_scalars:
        ds = torch.tensor([h["lr"], h["bc1"], h["sqrt_bc2"], h["grad_scale"]], dtype=torch.float32, device=dev)
        h.update(lr=float("nan"), bc1=float("nan"), sqrt_bc2=float("nan"), grad_scale=9.0)
    rc, msg, _ = _call(dev, lib.dmpnn_adam_step, mats["p"].ptr, mats["g"].ptr, mats["m"].ptr, mats["v"].ptr,
                       int(p.numel()) if n is None else n, h["lr"], h["beta1"], h["beta2"], h["eps"], h["wd"], h["bc1"], h["sqrt_bc2"],
                       h["grad_scale"], ds.data_ptr() if ds is not None else None)
    return rc, msg, mats


# ---- dmpnn_clip_grad -----------------------------------------------------------------------------------------------------------------------
def clip_ref(g, clip, mode, grad_scale=1.0, dtype=torch.float64):
    """``torch.nn.utils.clip_grad_norm_`` / ``clip_grad_value_`` on the AVERAGED gradient ``g grad_scale``, stated on the buffer that
    holds ``g`` (``clip`` and ``grad_scale`` rounded to float32 first, as the ABI receives them).

    Norm mode -> ``(total, coef, g_out)``: ``total = grad_scale ||g||_2``, ``coef = clip / (total + 1e-6)``, ``g_out = g coef`` where
    ``coef < 1`` and ``g`` itself otherwise (the scale stays out of the buffer: ``dmpnn_adam_step`` applies it).
    Value mode -> ``g_out = clamp(g, -c, c)`` with ``c = float32(clip) / float32(grad_scale)`` formed in float32: bit for bit what
    the kernel owes (``torch.clamp`` keeps NaN)."""
    g = g.to(dtype)
    if mode == CLIP_VALUE:
        c = float(np.float32(clip) / np.float32(grad_scale))
        return torch.clamp(g, -c, c)
    assert mode == CLIP_NORM
    total = torch.linalg.vector_norm(g) * torch.tensor(f32(grad_scale), dtype=dtype)
    coef = torch.tensor(f32(clip), dtype=dtype) / (total + 1e-6)
    return total, coef, (g * coef if not bool(coef >= 1) else g.clone())


def run_clip(dev, g, clip, mode, grad_scale=1.0, n=None, off=0, ws_null=False):
    """One ``dmpnn_clip_grad`` call on a flat float32 CPU tensor -> (rc, msg, the buffer's ``Mat``, the scratch ``Workspace``:
    exactly ``dmpnn_clip_grad_ws_bytes()`` bytes)."""
    lib = _lib.load()
    mg = Mat(dev, 1, int(g.numel()), None, off, g.view(1, -1))
    ws = Workspace(dev, int(lib.dmpnn_clip_grad_ws_bytes()))
    assert ws.words == CLIP_PARTIALS + 4
    rc, msg, _ = _call(dev, lib.dmpnn_clip_grad, mg.ptr, int(g.numel()) if n is None else n, clip, mode, grad_scale,
                       None if ws_null else ws.ptr)
    return rc, msg, mg, ws


def clip_blocks(n) -> int:
    """Workgroups (= partial sums written) of a norm-mode call on ``n`` floats: the launch rule of ``dmpnn_clip_grad`` restated."""
    return min((n // 4 + 255) // 256, CLIP_PARTIALS)
