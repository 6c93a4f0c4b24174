"""The readout, clip and Adam entries of ``include/dmpnn.h`` — ``dmpnn_molagg_bounds`` / ``_fwd`` / ``_bwd`` (``dmpnn_molagg.hip``),
``dmpnn_adam_step``, ``dmpnn_clip_grad`` (+ ``_ws_bytes``; ``dmpnn_optim.hip``) — through the C ABI at the edges of their dispatch
(``tests/flat_harness.py``).  They run in every training step and every fingerprint; the module tests (``test_agg.py``,
``test_optim.py``, ``test_lightning_fit.py``) reach them with dense tensors, ``dev_scalars = NULL`` and one buffer size.

What is held, and how tightly
* BIT FOR BIT, no margin: the tables ``first | end | flag | padding | done`` of the bounds pass (exact integers, both kernels, the
  molecule boundary on a workgroup edge, the first atom of the grid-stride loop); the forward reduce in the three modes against the
  sequential float32 reference (rows in increasing atom order, the first addend copied — the data carries ``-0.0`` first addends, the
  only values at which a copy and ``0 + x`` differ — one true division); the backward expand; the NaN poison (``0x7FC00000``) behind
  an invalid batch vector; value clipping against ``torch.clamp``; the identity side of norm clipping; ``dev_scalars`` against the
  argument path; entries with a zero gradient and zero moments under Adam.  The float64 error the forward tests print
  (``FLATSUM``) is NOT asserted: it is the error of float32 sequential summation itself, which the reference shares.
* ``min(MARGIN max(e32, 2**-23), cap)`` on the unfloored ``max|got - ref64| / max|ref64|``: Adam's ``m``, ``v`` and UPDATE
  ``p_old - p_new`` (and ``p_new`` with weight decay), the clip total ``ws[256]`` and the scaled buffer, the adjoint identity
  ``<fwd(H), G> = <H, bwd(G)>`` of the GPU outputs.  ``e32``: plain float32 PyTorch on the same inputs against float64 —
  ``torch.optim.Adam(foreach=False)``, ``torch.linalg.vector_norm``, ``g coef``, ``index_add_`` / indexing; ``cap = 2e-5``.
* Every output and in-place buffer lives in a NaN-prefilled allocation whose padding, guard words and, for the workspaces, every
  word the entry does not own must come back untouched; the inputs carry NaN in their padding.  An argument error writes nothing.

Adam's learning rate here is ``2**-7``: with parameters of order 1 the float32 rounding of ``p`` alone (up to ``2**-25``) is 3e-5
of an update of 1e-3 — above the cap for ANY float32 implementation, torch's included — and 4e-6 of one of ``2**-7``.

MARGIN (``rows_harness.MARGIN`` = 16, the suite's one number).  Measured on the MI355X with the ``FLATBAR`` report line of every
comparison (176 of them): the worst ``err / max(e32, 2**-23)`` is 1.19 — the update of ``n4-wd0-p0-gs1-step1000`` (err 1.4e-7 against
a float32 draw of 6.5e-8: the kernel multiplies ``sqrt(v)`` by ``1 / sqrt_bc2`` where torch divides); then 1.16 and 1.06 (the adjoint
identity at ``d_h`` 300 and 65, err 1.4e-7 and 3.6e-7), 1.03 (an update with weight decay: 1.6e-6, all of it the float32 rounding
of ``p``), 0.91 (``v``), 0.37 (the clipped buffer) and 0.26 (the clip total, err 3.1e-8).  2 x 1.19 = 2.38 -> 4, at most 16: the
shared constant is used, a relative bar of 1.9e-6 where ``e32`` is under ``2**-23`` and the cap of 2e-5 on the weight-decay updates
(``e32`` up to 7.6e-6).  The printed float64 error of the forward reduce ranges from 5.8e-9 to 1.8e-6 (1 000 rows added in turn).
Wall time of the module's 213 GPU tests on the MI355X: 5.6 s.

The value-clip NaN question: on the library as it was, ``test_flat_clip_value_bit_exact`` FAILED in all six cases — every NaN gradient
came back as ``-c`` (-0.3 at ``grad_scale`` 1, -1.2 at 0.25; entries 0, 7, 515, 1020, 1027 of 1 028).  ``k_clip_value`` now clamps
by compare-and-select, which differs from ``fminf(fmaxf(v, -c), c)`` on NaN alone, and the six cases pass bit for bit.

Tried against deliberately wrong builds (scratch copies, never committed; none can move an access out of bounds or loop for ever):
==============================================================  ==================================================================
the ``v == v0`` copy of ``k_mol_reduce`` replaced by ``0 + x``   ``test_flat_molagg_fwd_bit_exact`` (all 55), ``_fwd_layouts`` (all 15): the ``-0.0`` addends
mean dividing by ``cnt + 1``                                     ``test_flat_molagg_fwd_bit_exact[*-mean]`` (11), ``_fwd_layouts[mean-*]`` (5)
``next`` of ``k_mol_bounds`` defaulting to ``n_mols - 1``        ``test_flat_bounds_tables``: the 9 cases beyond 32 768 atoms whose last molecule has atoms
``k_adam`` using ``sqrt_bc2`` instead of its reciprocal          ``test_flat_adam_step`` (all 40)
``k_clip_scale`` summing ``n_partial - 1`` partials              ``test_flat_clip_norm`` (all 20)
``k_clip_sqsum``'s stride one workgroup short (never 0)          ``test_flat_clip_norm``: the 12 cases of 255 workgroups and more (groups counted twice)
==============================================================  ==================================================================
"""
import dataclasses
import functools
import glob
import os

import numpy as np
import pytest
import torch

import flat_harness as fh
import rows_harness as rh
from conftest import GOLDEN_DIR

MARGIN = rh.MARGIN
gpu = pytest.mark.gpu
bits = fh.bits


def _report(line):
    print(line.replace("ROWSBAR", "FLATBAR"))


def _hold(case_id, got, ref, e32):
    fails = rh.compare(case_id, got, ref, e32, "grad", margin=MARGIN, report=_report)
    assert not fails, f"{case_id}: " + "; ".join(fails)


def _e32(r32: dict, r64: dict) -> dict:
    return rh.yardstick(r64, r32)


def same_bits(a, b) -> bool:
    return a.shape == b.shape and bool((bits(a) == bits(b)).all())


# ---- dmpnn_molagg_bounds -----------------------------------------------------------------------------------------------------------------
def _cuts(n_atoms, cuts, n_tail_empty=0):
    """Counts of the molecules that start at atom 0 and at every atom of ``cuts``."""
    edges = [0] + sorted(set(c for c in cuts if 0 < c < n_atoms)) + [n_atoms]
    return [b - a for a, b in zip(edges, edges[1:])] + [0] * n_tail_empty


def _regular(n_atoms, extra=()):
    """Molecules of 37 atoms (no multiple of a wave or a workgroup) plus a boundary in front of every atom of ``extra``."""
    return _cuts(n_atoms, list(range(37, n_atoms, 37)) + list(extra))


def _with_empties(counts):
    """Empty molecules first (two), in the middle (one, then three in a row) and last (two)."""
    k = len(counts) // 2
    return [0, 0] + counts[:k] + [0] + counts[k:k + 1] + [0, 0, 0] + counts[k + 1:] + [0, 0]


BOUNDS_VALID = dict([
    ("1-atom", [1]),
    ("1023-atoms", _regular(1023)),
    ("1024-atoms-one-stride", _regular(1024)),
    ("1025-atoms-boundary-1023|1024", _regular(1025, (1024,))),
    ("32767-atoms", _regular(32767)),
    ("32768-atoms-last-single-workgroup", _regular(32768, (256, 257, 1024))),
    ("32769-atoms-first-multi-block", _regular(32769)),
    ("32769-boundary-255|256", _cuts(32769, list(range(512, 32769, 41)) + [256])),
    ("32769-boundary-256|257", _cuts(32769, list(range(512, 32769, 41)) + [257])),
    ("32769-boundary-1023|1024", _cuts(32769, [1024] + list(range(2000, 32769, 333)))),
    ("262145-atoms-one-into-grid-stride", _regular(262145)),
    ("262145-boundary-262143|262144", _cuts(262145, list(range(100, 262000, 97)) + [262144])),
    ("262145-last-atom-joins-its-molecule", _cuts(262145, list(range(100, 262000, 97)) + [262143])),
    ("empties-first-middle-last-small", _with_empties([3, 1, 2, 4])),
    ("empties-first-middle-last-1025", _with_empties(_regular(1025))),
    ("empties-first-middle-last-32769", _with_empties(_regular(32769, (256,)))),
    ("one-molecule-1025", [1025]),
    ("one-molecule-32769", [32769]),
    ("one-atom-per-molecule-1025", [1] * 1025),
    ("one-atom-per-molecule-32769", [1] * 32769),
    ("5-atoms-5000-molecules", [2, 0, 3] + [0] * 4997),
    ("no-atoms-7-molecules", [0] * 7),
    ("no-atoms-no-molecules", []),
])


@functools.lru_cache(maxsize=None)
def _bounds_case(cid):
    counts = BOUNDS_VALID[cid]
    batch = fh.batch_of(counts)
    first, end, valid = fh.bounds_ref(batch, len(counts))
    assert valid
    return batch, len(counts), first, end


@gpu
@pytest.mark.parametrize("cid", list(BOUNDS_VALID))
def test_flat_bounds_tables(cid, gpu_device):
    """``dmpnn_molagg_bounds`` on a valid batch vector: ``first`` and ``end`` equal the plain loop's, the flag, the three padding words
    and ``done[n_mols]`` are zero, the guard behind ``dmpnn_molagg_ws_bytes(n_mols)`` bytes is untouched.  Up to 32 768 atoms
    the single workgroup runs, which zeroes its own tables (more of them than it scans when ``n_mols`` exceeds ``n_atoms``); beyond, a
    memset and the multi-block kernel, whose threads read ``batch[v - 1]`` and ``batch[v + 1]`` across workgroup edges."""
    batch, n_mols, first, end = _bounds_case(cid)
    res = fh.run_bounds(gpu_device, batch, n_mols)
    assert res["rc"] == 0, res["msg"]
    assert res["launches"] == (1 if batch.numel() > 0 else 0)
    t = fh.bounds_tables(res["ws"], n_mols)
    assert res["ws"].guard_ok(), "a word behind the workspace was written"
    assert t["flag"] == 0 and not bool(t["pad"].any()) and not bool(t["done"].any()), (t["flag"], t["pad"].tolist())
    bad = torch.nonzero((t["first"] != first) | (t["end"] != end)).view(-1)
    assert bad.numel() == 0, f"{bad.numel()} molecules differ, the first: m={int(bad[0])} got [{int(t['first'][bad[0]])}, " \
                             f"{int(t['end'][bad[0]])}) want [{int(first[bad[0]])}, {int(end[bad[0]])})"


def _invalid_batch(kind, n_atoms):
    """(batch, n_mols): a valid vector of molecules of 3 atoms with ONE defect."""
    n_mols = -(-n_atoms // 3)
    batch = torch.arange(n_atoms, dtype=torch.int64) // 3
    mid = n_atoms // 2 + 1     # (the second atom of its molecule, whose predecessor's id is at least 1)
    if kind == "id-minus-1":
        batch[mid] = -1
    elif kind == "id-n_mols":
        batch[n_atoms - 1] = n_mols
    elif kind == "decreasing-pair-middle":
        batch[mid] = batch[mid - 1] - 1
    elif kind == "decreasing-pair-255|256":
        batch[256] = batch[255] - 1
    else:
        raise AssertionError(kind)
    return batch, n_mols


INVALID = [(k, n) for n in (6, 32769) for k in ("id-minus-1", "id-n_mols", "decreasing-pair-middle")] + [("decreasing-pair-255|256", 32769)]


@gpu
@pytest.mark.parametrize("kind,n_atoms", INVALID, ids=[f"{k}-{n}" for k, n in INVALID])
def test_flat_invalid_batch_poisons_fwd_and_bwd(kind, n_atoms, gpu_device):
    """An invalid batch vector on either bounds kernel: the flag word is nonzero, and a following ``dmpnn_molagg_fwd`` /
    ``dmpnn_molagg_bwd`` fills every ``[n_mols, d_h]`` / ``[n_atoms, d_h]`` word with ``0x7FC00000`` — padding and guards untouched."""
    dev = gpu_device
    batch, n_mols = _invalid_batch(kind, n_atoms)
    assert not fh.bounds_ref(batch, n_mols)[2]
    assert kind.startswith("id-") or (int(batch.min()) >= 0 and int(batch.max()) < n_mols), "a decreasing pair of ids that are in range"
    res = fh.run_bounds(dev, batch, n_mols)
    assert res["rc"] == 0, res["msg"]
    assert res["ws"].guard_ok()
    assert fh.bounds_tables(res["ws"], n_mols)["flag"] != 0
    gen = torch.Generator().manual_seed(n_atoms)
    for d_h, pad in ((5, 2), (8, 4)):      # the scalar and the vector build
        for mode in (fh.SUM, fh.MEAN, fh.NORM):
            rc, msg, out = fh.run_molagg_fwd(dev, torch.randn(n_atoms, d_h, generator=gen), res["ws"], n_mols, mode, 100.0, ldh=d_h + pad,
                                             ldo=d_h + 3)
            assert rc == 0, msg
            assert bool((bits(out.read("out")) == fh.POISON).all()), (d_h, mode)
            rc, msg, gH = fh.run_molagg_bwd(dev, torch.randn(n_mols, d_h, generator=gen), res["batch"], res["ws"], n_mols, mode, 100.0,
                                            ldg=d_h + 1, ldgh=d_h + 3)
            assert rc == 0, msg
            assert bool((bits(gH.read("gH")) == fh.POISON).all()), (d_h, mode)


@gpu
def test_flat_bounds_argument_errors(gpu_device):
    """A workspace one byte short, or a NULL batch with atoms: ``DMPNN_EINVAL`` and not a word written."""
    batch = fh.batch_of([2, 0, 3])
    for kw in (dict(ws_short=1), dict(null_batch=True)):
        res = fh.run_bounds(gpu_device, batch, 3, **kw)
        assert res["rc"] == fh.EINVAL and res["msg"], kw
        assert res["launches"] == 0 and res["ws"].pristine(), kw


# ---- dmpnn_molagg_fwd / dmpnn_molagg_bwd ---------------------------------------------------------------------------------------------------
D_H = (1, 3, 4, 63, 64, 65, 252, 256, 260, 300, 516)   # one | two slabs on the scalar build (64 | 65) and on the vector build (256 | 260);
#                                                       a partial last float4 never (d_h % 4 == 0 there), a partial last slab: 300, 516
COUNTS = [0, 1, 2, 1000, 0, 3, 1]                        # 7 molecules: 7, 14 or 21 waves — never a multiple of 4 (the last workgroup partly idle)
NORMS = (1.0, 100.0, 7.3)
AGG_MODES = [("sum", fh.SUM, 1.0), ("mean", fh.MEAN, 1.0)] + [(f"norm{c:g}", fh.NORM, c) for c in NORMS]


@functools.lru_cache(maxsize=None)
def _agg_inputs(d_h, counts=tuple(COUNTS)):
    """``H [V, d_h]`` (row ``v`` scaled by ``2**-(v % 12)``, column ``c`` by ``1 + c / d_h``: the order of a long sum is visible, a shifted
    slab or a transposed tile cannot pass), with ``-0.0`` as a lone and as a first addend; ``G [n_mols, d_h]``; the batch vector."""
    gen = torch.Generator().manual_seed(77 + d_h)
    batch = fh.batch_of(list(counts))
    V, n_mols = int(batch.numel()), len(counts)
    H = torch.randn(V, d_h, generator=gen) * (2.0 ** -(torch.arange(V) % 12).float()).view(-1, 1) * (1 + torch.arange(d_h).float() / d_h)
    H[0, ::2] = -0.0         # the molecule of one atom: a lone -0.0 is copied, 0 + (-0.0) would be +0.0
    H[1:3, -1] = -0.0        # the molecule of two atoms: -0.0 + -0.0 = -0.0 only when the first addend was copied
    H[3, 0] = -0.0           # the first atom of the long molecule: no trace in a nonzero sum
    G = torch.randn(n_mols, d_h, generator=gen) * (1 + torch.arange(d_h).float() / d_h)
    return H, G, batch, n_mols


@functools.lru_cache(maxsize=None)
def _agg_ref(d_h, mode, norm):
    H, G, batch, n_mols = _agg_inputs(d_h)
    return (fh.molagg_ref(H, batch, n_mols, mode, norm), fh.molagg_ref(H, batch, n_mols, mode, norm, torch.float64),
            fh.molagg_bwd_ref(G, batch, n_mols, mode, norm))


@functools.lru_cache(maxsize=2)
def _agg_ws(dev):
    _, _, batch, n_mols = _agg_inputs(4)
    res = fh.run_bounds(dev, batch, n_mols)
    assert res["rc"] == 0, res["msg"]
    return res


def _mismatch(got, ref):
    bad = torch.nonzero(bits(got) != bits(ref))
    return f"{bad.shape[0]} words differ, the first at {bad[0].tolist()}: got {float(got[tuple(bad[0])])!r} want {float(ref[tuple(bad[0])])!r}"


def _check_fwd(dev, d_h, label, mode, norm, **layout):
    H, _, _, n_mols = _agg_inputs(d_h)
    ref32, ref64, _ = _agg_ref(d_h, mode, norm)
    rc, msg, out = fh.run_molagg_fwd(dev, H, _agg_ws(dev)["ws"], n_mols, mode, norm, **layout)
    assert rc == 0, msg
    got = out.read("out")
    err = float((got.double() - ref64).abs().max() / ref64.abs().max())
    print(f"FLATSUM fwd d_h={d_h} {label} {layout or 'dense'} float64-err={err:.3e} (float32 sequential summation's own)")
    assert same_bits(got, ref32), f"d_h={d_h} {label}: " + _mismatch(got, ref32)
    empty = [m for m, c in enumerate(COUNTS) if c == 0]
    assert bool((bits(got[empty]) == 0).all()), "a molecule without atoms gives a row of +0.0, the mean included"


@gpu
@pytest.mark.parametrize("label,mode,norm", AGG_MODES, ids=[a[0] for a in AGG_MODES])
@pytest.mark.parametrize("d_h", D_H, ids=[f"h{d}" for d in D_H])
def test_flat_molagg_fwd_bit_exact(d_h, label, mode, norm, gpu_device):
    """``dmpnn_molagg_fwd``, dense rows, molecules of 0, 1, 2, 3 and 1 000 atoms in one batch: bit for bit the sequential float32
    reference.  The float64 error printed is that of float32 sequential summation itself (not asserted)."""
    _check_fwd(gpu_device, d_h, label, mode, norm)


FWD_LAYOUTS = [("h8-ldh12-vector-padded", dict(ldh=12)), ("h8-ldh9-scalar", dict(ldh=9)), ("h8-H+1float-scalar", dict(off_h=1)),
               ("h8-ldo11-out+1float-vector-scalar-stores", dict(ldo=11, off_o=1)),
               ("h8-everything-odd", dict(ldh=9, off_h=1, ldo=11, off_o=1))]


@gpu
@pytest.mark.parametrize("label,mode,norm", AGG_MODES[:3], ids=[a[0] for a in AGG_MODES[:3]])
@pytest.mark.parametrize("lid,layout", FWD_LAYOUTS, ids=[c[0] for c in FWD_LAYOUTS])
def test_flat_molagg_fwd_layouts(lid, layout, label, mode, norm, gpu_device):
    """``d_h = 8``: a padded ``ldh`` stays on the vector build, an ``ldh`` that is no multiple of 4 or a 4-byte aligned ``H`` falls to
    the scalar build, and the output may sit anywhere (the vector build stores scalars) — NaN in the padding of ``H`` throughout."""
    _check_fwd(gpu_device, 8, label, mode, norm, **layout)


@gpu
def test_flat_molagg_fwd_noops_and_argument_errors(gpu_device):
    """``n_mols = 0`` or ``d_h = 0``: ``DMPNN_OK``, nothing written; an unknown mode or ``ldh < d_h``: ``DMPNN_EINVAL``, nothing
    written."""
    dev = gpu_device
    H = _agg_inputs(8)[0]
    n_mols = len(COUNTS)
    ws = _agg_ws(dev)["ws"]
    for say, want in ((dict(n_mols=0), 0), (dict(d_h=0), 0), (dict(mode=3), fh.EINVAL), (dict(mode=-1), fh.EINVAL), (dict(ldh=7), fh.EINVAL),
                      (dict(ldo=7), fh.EINVAL)):
        rc, msg, out = fh.run_molagg_fwd(dev, H, ws, n_mols, fh.SUM, say=say)
        assert rc == want, (say, rc, msg)
        assert out.pristine(), say


BWD_LAYOUTS = [("dense", {}), ("padded", dict(ldg=lambda d: d + 3, ldgh=lambda d: d + 5)),
               ("padded+offset", dict(ldg=lambda d: d + 1, ldgh=lambda d: d + 2, off_g=1, off_gh=3))]


@gpu
@pytest.mark.parametrize("lid,layout", BWD_LAYOUTS, ids=[c[0] for c in BWD_LAYOUTS])
@pytest.mark.parametrize("d_h", D_H, ids=[f"h{d}" for d in D_H])
def test_flat_molagg_bwd_bit_exact(d_h, lid, layout, gpu_device):
    """``dmpnn_molagg_bwd`` in the three modes: ``gOut[batch[v]]``, the mean divided by the molecule's OWN count, bit for bit; 1 007
    atoms: the last workgroup holds three rows."""
    dev = gpu_device
    _, G, _, n_mols = _agg_inputs(d_h)
    res = _agg_ws(dev)
    lay = {k: (f(d_h) if callable(f) else f) for k, f in layout.items()}
    for label, mode, norm in AGG_MODES[:2] + AGG_MODES[-1:]:
        ref = _agg_ref(d_h, mode, norm)[2]
        rc, msg, gH = fh.run_molagg_bwd(dev, G, res["batch"], res["ws"], n_mols, mode, norm, **lay)
        assert rc == 0, msg
        got = gH.read("gH")
        assert same_bits(got, ref), f"d_h={d_h} {label}: " + _mismatch(got, ref)


def _adjoint(out, G, H, gH):
    """``<out, G>`` and ``<H, gH>`` accumulated in float64."""
    return float((out.double() * G.double()).sum()), float((H.double() * gH.double()).sum())


def _adjoint_inputs(d_h):
    """The batch of the sweep with ordinary rows (no ``2**-(v % 12)`` grading, no signed zeros): an inner product of them has a scale."""
    _, G, batch, n_mols = _agg_inputs(d_h)
    H = torch.randn(int(batch.numel()), d_h, generator=torch.Generator().manual_seed(5 + d_h)) + 0.5
    return H, G + 0.5, batch, n_mols


def _adjoint_yardstick(d_h, norm):
    """The gap of the identity in plain float32 PyTorch (``index_add_``, indexing, one division) -> (a32, b32)."""
    H, G, batch, n_mols = _adjoint_inputs(d_h)
    out = torch.zeros(n_mols, d_h).index_add_(0, batch, H) / fh.f32(norm)
    return _adjoint(out, G, H, G[batch] / fh.f32(norm))


ADJOINT = [(d, label, mode, norm) for d in (1, 65, 300) for label, mode, norm in (AGG_MODES[0], AGG_MODES[-1])]


@gpu
@pytest.mark.parametrize("d_h,label,mode,norm", ADJOINT, ids=[f"h{c[0]}-{c[1]}" for c in ADJOINT])
def test_flat_molagg_adjoint_identity(d_h, label, mode, norm, gpu_device):
    """``<fwd(H), G> = <H, bwd(G)>`` on the GPU outputs (sum and norm), accumulated in float64 on the host, within the rule's bar over
    the same gap of plain float32 PyTorch."""
    dev = gpu_device
    H, G, batch, n_mols = _adjoint_inputs(d_h)
    res = _agg_ws(dev)
    rc, msg, out = fh.run_molagg_fwd(dev, H, res["ws"], n_mols, mode, norm)
    assert rc == 0, msg
    rc, msg, gH = fh.run_molagg_bwd(dev, G, res["batch"], res["ws"], n_mols, mode, norm)
    assert rc == 0, msg
    a, b = _adjoint(out.read("out"), G, H, gH.read("gH"))
    a32, b32 = _adjoint_yardstick(d_h, norm if mode == fh.NORM else 1.0)
    _hold(f"adjoint-h{d_h}-{label}", dict(adjoint=torch.tensor([a])), dict(adjoint=torch.tensor([b], dtype=torch.float64)),
          dict(adjoint=abs(a32 - b32) / abs(b32)))


# ---- dmpnn_adam_step -----------------------------------------------------------------------------------------------------------------------
LR, BETA1, BETA2, ADAM_EPS, WD = 2.0 ** -7, fh.f32(0.9), fh.f32(0.999), fh.f32(1e-8), fh.f32(0.01)
ADAM_STRIDE = 4 * (2048 * 256 + 1)     # one float4 group into the grid-stride loop of k_adam
ADAM_N = (4, 1020, 1024, 1028, ADAM_STRIDE)


@dataclasses.dataclass(frozen=True)
class A:
    n: int
    wd: bool          # False: p_old = 0 and no weight decay (the update is not hidden under |p|); True: wd = 0.01, |p| in [0.25, 1)
    gs: float
    step: int         # 1: m = v = 0; 1000: moments carried over, sqrt_bc2 = 0.795 (0.0316 at step 1)

    @property
    def id(self):
        return f"n{self.n}-{'wd0.01-p~1' if self.wd else 'wd0-p0'}-gs{self.gs:g}-step{self.step}"


ADAM_CASES = [A(n, wd, gs, step) for n in ADAM_N for wd in (False, True) for gs in (1.0, 0.25) for step in (1, 1000)]


def _adam_inputs(case: A):
    """Flat float32 buffers whose data depends on the index: gradients graded over ``2**-20 .. 2**10``, one entry of every group of
    four (rotating) exactly 0 with ``m = v = 0``.  With weight decay the gradient carries the SIGN OF ITS PARAMETER: at step 1 the
    update is ``lr g' / (|g'| + eps')``, the sign of ``g' = g grad_scale + wd p``, so where the two terms cancel the float32 update is
    decided by the rounding of ``wd p`` — with random signs two of 2 097 156 entries cancelled to 1.4e-5 and 7e-6 of their terms and
    the update missed float64 by 1.4e-4 and 5.7e-4 on the MI355X, figures that two-rounding float32 arithmetic reproduces on the CPU
    to three digits (1.39e-4, 5.70e-4; torch's own draw, an fma, 7.8e-6): no property of the kernel, and nothing a bar can hold
    (``conftest.adam_comparable`` meets the same effect).  Without weight decay (``p = 0``) the signs are random."""
    n = case.n
    gen = torch.Generator().manual_seed(n % 9973 + 10 * case.step + int(case.wd))
    idx = torch.arange(n)
    zero = (idx + idx // 4) % 4 == 0
    z = torch.zeros(n)
    g = torch.where(zero, z, torch.randn(n, generator=gen) * 2.0 ** ((idx * 7) % 31 - 20).float())
    sign = torch.where(torch.rand(n, generator=gen) < 0.5, -1.0, 1.0)
    p = sign * (0.25 + 0.75 * torch.rand(n, generator=gen)) if case.wd else z.clone()
    if case.wd:
        g = g.abs() * sign
    if case.step == 1:
        m, v = z.clone(), z.clone()
    else:
        m = torch.where(zero, z, 0.3 * g * (1 + 0.5 * torch.randn(n, generator=gen)))
        v = torch.where(zero, z, g * g * (0.5 + torch.rand(n, generator=gen)))
    hyper = fh.adam_hyper(LR, BETA1, BETA2, ADAM_EPS, WD if case.wd else 0.0, case.step, case.gs)
    return dict(p=p, g=g, m=m, v=v, zero=zero, hyper=hyper)


def _adam_tensors(p_old, p, m, v, with_p):
    d = dict(m=m.double(), v=v.double(), update=p_old.double() - p.double())
    if with_p:
        d["p"] = p.double()
    return d


@functools.lru_cache(maxsize=4)
def _adam_ref(case: A):
    inp = _adam_inputs(case)
    r64 = _adam_tensors(inp["p"], *fh.adam_ref(inp["p"], inp["g"], inp["m"], inp["v"], inp["hyper"]), case.wd)
    r32 = _adam_tensors(inp["p"], *fh.torch_adam(inp["p"], inp["g"], inp["m"], inp["v"], inp["hyper"], case.step, torch.float32), case.wd)
    return inp, r64, _e32(r32, r64)


def _adam_read(mats, inp):
    """(p, m, v) read back (guards checked); the gradient buffer must not have changed."""
    assert same_bits(mats["g"].read("g").view(-1), inp["g"]), "the gradient buffer was written"
    return tuple(mats[k].read(k).view(-1) for k in ("p", "m", "v"))


@gpu
@pytest.mark.parametrize("case", ADAM_CASES, ids=lambda c: c.id)
def test_flat_adam_step(case, gpu_device):
    """``dmpnn_adam_step`` against the header's four lines in float64: ``m``, ``v`` and the update ``p_old - p_new`` (``p_new`` too with
    weight decay), each within the rule's bar over ``torch.optim.Adam(foreach=False)`` in float32; without weight decay an entry
    with zero gradient and zero moments keeps ``p``, ``m`` and ``v`` bit for bit.  The largest size is one float4 group beyond the
    2 048 x 256 threads of the launch: a group stepped twice or never shows in ``m``."""
    inp, r64, e32 = _adam_ref(case)
    rc, msg, mats = fh.run_adam(gpu_device, inp["p"], inp["g"], inp["m"], inp["v"], inp["hyper"])
    assert rc == 0, msg
    p, m, v = _adam_read(mats, inp)
    _hold(case.id, _adam_tensors(inp["p"], p, m, v, case.wd), r64, e32)
    if not case.wd:
        z = inp["zero"]
        assert int(z.sum()) == case.n // 4
        for name, new in (("p", p), ("m", m), ("v", v)):
            assert same_bits(new[z], inp[name][z]), f"{name}: an entry with g = m = v = 0 changed"


@gpu
@pytest.mark.parametrize("case", [A(1028, True, 0.25, 1000), A(ADAM_STRIDE, False, 1.0, 1)], ids=lambda c: c.id)
def test_flat_adam_dev_scalars_equal_the_arguments(case, gpu_device):
    """lr, bc1, sqrt_bc2 and grad_scale from the 4-float device array, NaN / NaN / NaN / 9 in the arguments: bit for bit the argument
    path."""
    inp = _adam_inputs(case)
    outs = []
    for dev_scalars in (False, True):
        rc, msg, mats = fh.run_adam(gpu_device, inp["p"], inp["g"], inp["m"], inp["v"], inp["hyper"], dev_scalars=dev_scalars)
        assert rc == 0, msg
        outs.append(_adam_read(mats, inp))
    for name, a, b in zip("pmv", *outs):
        assert bool(torch.isfinite(b).all()) and same_bits(a, b), name


@gpu
def test_flat_adam_nan_gradient_stays_in_its_entry(gpu_device):
    """A NaN gradient gives NaN in ``m``, ``v`` and ``p`` at that entry, and every other entry is what it is without the NaN."""
    case = A(1028, True, 1.0, 1000)
    inp = _adam_inputs(case)
    at = 517
    g_nan = inp["g"].clone()
    g_nan[at] = float("nan")
    outs = []
    for g in (inp["g"], g_nan):
        rc, msg, mats = fh.run_adam(gpu_device, inp["p"], g, inp["m"], inp["v"], inp["hyper"])
        assert rc == 0, msg
        outs.append(tuple(mats[k].read(k).view(-1) for k in ("p", "m", "v")))
    others = torch.arange(case.n) != at
    for name, clean, dirty in zip("pmv", *outs):
        assert bool(torch.isnan(dirty[at])), name
        assert same_bits(clean[others], dirty[others]), name


@gpu
def test_flat_adam_noop_and_argument_errors(gpu_device):
    """``n = 6``, or any of the four pointers 4 bytes off a 16-byte boundary: ``DMPNN_EINVAL`` and nothing written; ``n = 0``:
    ``DMPNN_OK`` and nothing written."""
    inp = _adam_inputs(A(8, True, 1.0, 1000))
    for kw, want in [(dict(n=6), fh.EINVAL), (dict(n=0), 0), (dict(n=-4), fh.EINVAL)] + [(dict(off={k: 1}), fh.EINVAL) for k in fh.ADAM_BUFFERS]:
        rc, msg, mats = fh.run_adam(gpu_device, inp["p"], inp["g"], inp["m"], inp["v"], inp["hyper"], **kw)
        assert rc == want, (kw, rc, msg)
        for k in fh.ADAM_BUFFERS:
            assert same_bits(mats[k].read(k).view(-1), inp[k]), (kw, k)


# ---- dmpnn_clip_grad -----------------------------------------------------------------------------------------------------------------------
CLIP_N = (4, 1024, 4 * 255 * 256, 4 * 256 * 256, 4 * (256 * 256 + 1))   # one workgroup; 255 | 256 of them (the cap); the grid-stride loop
CLIP_CASES = [(n, f, gs) for n in CLIP_N for f in (0.5, 2.0) for gs in (1.0, 0.25)]


@functools.lru_cache(maxsize=None)
def _clip_g(n):
    gen = torch.Generator().manual_seed(n % 9973)
    return torch.randn(n, generator=gen) * (1 + (torch.arange(n) % 7).float())


def _clip_ws_words(ws, n, total_expected=True):
    """The scratch after a norm-mode call on ``n`` floats -> the total ``ws[256]``; the partial slots no workgroup owns, ``ws[257..259]``
    and the guard must hold the prefill (a NaN: a kernel that READ one of them would have a NaN total)."""
    w = ws.cpu()
    blocks = fh.clip_blocks(n)
    assert ws.guard_ok(), "a word behind dmpnn_clip_grad_ws_bytes() was written"
    assert bool((w[blocks:fh.CLIP_PARTIALS] == fh.PREFILL).all()), f"a partial slot at or above {blocks} was written"
    assert bool((w[fh.CLIP_PARTIALS + 1:] == fh.PREFILL).all()), "ws[257..259] was written"
    assert bool((w[:blocks] != fh.PREFILL).all()), "a workgroup left its partial sum unwritten"
    return w[fh.CLIP_PARTIALS:fh.CLIP_PARTIALS + 1].view(torch.float32)


@gpu
@pytest.mark.parametrize("n,factor,gs", CLIP_CASES, ids=[f"n{n}-clip{f:g}xtotal-gs{gs:g}" for n, f, gs in CLIP_CASES])
def test_flat_clip_norm(n, factor, gs, gpu_device):
    """``DMPNN_CLIP_NORM`` with ``clip = 0.5 total`` (the buffer against ``g coef`` in float64) and ``clip = 2 total`` (the buffer
    bit-identical: ``grad_scale`` enters the norm and the coefficient, never the buffer); ``ws[256]`` against the float64 norm."""
    g = _clip_g(n)
    total64 = float(torch.linalg.vector_norm(g.double())) * gs
    clip = fh.f32(factor * total64)
    t64, c64, g64 = fh.clip_ref(g, clip, fh.CLIP_NORM, gs)
    t32, c32, g32 = fh.clip_ref(g, clip, fh.CLIP_NORM, gs, torch.float32)
    assert (float(c64) < 0.51 and float(c32) < 1) if factor < 1 else (float(c64) > 1.9 and float(c32) > 1)
    rc, msg, mg, ws = fh.run_clip(gpu_device, g, clip, fh.CLIP_NORM, gs)
    assert rc == 0, msg
    got = dict(total=_clip_ws_words(ws, n))
    ref, r32 = dict(total=t64.view(1)), dict(total=t32.view(1))
    buf = mg.read("g").view(-1)
    if factor < 1:
        got["g"], ref["g"], r32["g"] = buf, g64, g32
    _hold(f"clip-n{n}-x{factor:g}-gs{gs:g}", got, ref, _e32(r32, ref))
    if factor > 1:
        assert same_bits(buf, g), "coef >= 1 is the identity, bit for bit"


@gpu
def test_flat_clip_norm_nan_gradient(gpu_device):
    """One NaN gradient: the total is NaN and, as in torch, so is the whole buffer (a diverged step stays visible)."""
    g = _clip_g(1028).clone()
    g[300] = float("nan")
    rc, msg, mg, ws = fh.run_clip(gpu_device, g, 1.0, fh.CLIP_NORM)
    assert rc == 0, msg
    assert bool(torch.isnan(_clip_ws_words(ws, 1028)).all())
    assert bool(torch.isnan(mg.read("g")).all())
    assert bool(torch.isnan(fh.clip_ref(g, 1.0, fh.CLIP_NORM, dtype=torch.float32)[2]).all())


CLIP_VALUE_CASES = [(n, gs) for n in (4, 1028, 262148) for gs in (1.0, 0.25)]


def _value_inputs(n, c):
    """Random entries around the bound ``c`` with the special values in the first and in the last float4 group (the last group of
    262 148 floats is the one the grid-stride loop reaches): ``+-inf``, ``-0.0``, a denormal, exactly ``+-c``, NaN."""
    g = (_clip_g(n) * c * 0.4).clone()
    special = [float("nan"), float("inf"), -float("inf"), -0.0, 1e-42, c, -c, float("nan")]
    if n == 4:
        g[:] = torch.tensor([float("nan"), -float("inf"), -0.0, c])
        return g
    g[:8] = torch.tensor(special)
    g[-8:] = torch.tensor(special[::-1])
    g[n // 2 + 1] = float("nan")
    return g


@gpu
@pytest.mark.parametrize("n,gs", CLIP_VALUE_CASES, ids=[f"n{n}-gs{gs:g}" for n, gs in CLIP_VALUE_CASES])
def test_flat_clip_value_bit_exact(n, gs, gpu_device):
    """``DMPNN_CLIP_VALUE`` bit for bit against ``torch.clamp`` with the bound ``float32(clip) / float32(grad_scale)``: ``+-inf`` come
    back as ``+-c``, ``-0.0`` and a denormal as themselves, and NaN STAYS NaN, as under ``torch.nn.utils.clip_grad_value_`` — the
    scratch is not touched."""
    clip = 0.3
    c = float(np.float32(clip) / np.float32(gs))
    g = _value_inputs(n, c)
    ref = fh.clip_ref(g, clip, fh.CLIP_VALUE, gs, torch.float32)
    assert int(torch.isnan(ref).sum()) == int(torch.isnan(g).sum()) > 0 and float(ref[~torch.isnan(ref)].abs().max()) == c
    rc, msg, mg, ws = fh.run_clip(gpu_device, g, clip, fh.CLIP_VALUE, gs)
    assert rc == 0, msg
    assert ws.pristine(), "value clipping needs no scratch"
    got = mg.read("g").view(-1)
    nan_lost = torch.nonzero(torch.isnan(ref) & ~torch.isnan(got)).view(-1)
    assert nan_lost.numel() == 0, f"NaN gradients came back finite: {[(int(i), float(got[i])) for i in nan_lost[:4]]}"
    assert same_bits(got, ref), _mismatch(got.view(1, -1), ref.view(1, -1))


@gpu
def test_flat_clip_noops_and_argument_errors(gpu_device):
    """``n = 6``, mode 2, ``grad_scale = 0``, a NULL scratch in norm mode: ``DMPNN_EINVAL``; ``clip_val`` 0, negative or NaN:
    ``DMPNN_OK`` — the buffer and the scratch pristine in every case."""
    g = _clip_g(1024)[:8].clone()
    cases = [(dict(n=6, clip=0.1, mode=fh.CLIP_NORM), fh.EINVAL), (dict(n=6, clip=0.1, mode=fh.CLIP_VALUE), fh.EINVAL),
             (dict(clip=0.1, mode=2), fh.EINVAL), (dict(clip=0.1, mode=fh.CLIP_NORM, grad_scale=0.0), fh.EINVAL),
             (dict(clip=0.1, mode=fh.CLIP_VALUE, grad_scale=0.0), fh.EINVAL), (dict(clip=0.1, mode=fh.CLIP_NORM, ws_null=True), fh.EINVAL)]
    cases += [(dict(clip=cv, mode=mode), 0) for cv in (0.0, -1.0, float("nan")) for mode in (fh.CLIP_NORM, fh.CLIP_VALUE)]
    for kw, want in cases:
        rc, msg, mg, ws = fh.run_clip(gpu_device, g, kw.pop("clip"), kw.pop("mode"), **kw)
        assert rc == want, (kw, rc, msg)
        assert ws.pristine() and same_bits(mg.read("g").view(-1), g), kw


# ---- the references, where no GPU is needed ------------------------------------------------------------------------------------------------
AGG_GOLDENS = sorted(glob.glob(os.path.join(GOLDEN_DIR, "agg", "*.npz")))


def test_flat_molagg_ref_is_the_oracle_on_the_goldens_on_cpu():
    """``molagg_ref`` / ``molagg_bwd_ref`` in float32 equal ``oracle.agg_torch`` and the stored outputs and gradients of the four
    aggregation goldens bit for bit; ``bounds_ref`` is the run-length table of a sorted vector and rejects what the kernels reject."""
    from oracle import agg_torch as oa

    assert len(AGG_GOLDENS) == 4
    for path in AGG_GOLDENS:
        z = np.load(path)
        H, batch, G, c = torch.from_numpy(z["H"]), torch.from_numpy(z["batch"]), torch.from_numpy(z["G"]), float(z["norm"])
        n_mols = int(batch.max()) + 1
        for label, mode, oracle in (("sum", fh.SUM, oa.sum_(H, batch)), ("mean", fh.MEAN, oa.mean(H, batch)), ("norm", fh.NORM, oa.norm(H, batch, c))):
            got = fh.molagg_ref(H, batch, n_mols, mode, c)
            assert same_bits(got, oracle), (path, label)
            assert same_bits(got, torch.from_numpy(z[f"out_{label}"])), (path, label)
            assert same_bits(fh.molagg_bwd_ref(G, batch, n_mols, mode, c), torch.from_numpy(z[f"gH_{label}"])), (path, label)
    H, _, batch, n_mols = _agg_inputs(3)
    assert same_bits(fh.molagg_ref(H, batch, n_mols, fh.SUM)[[0, 4]], torch.zeros(2, 3)), "empty molecules: +0.0"
    assert bool((bits(fh.molagg_ref(H, batch, n_mols, fh.MEAN)[1, ::2]) == bits(torch.tensor([-0.0]))).all()), "a lone -0.0 is copied"
    first, end, valid = fh.bounds_ref(fh.batch_of([0, 2, 0, 0, 3, 1, 0]), 7)
    assert valid and first.tolist() == [0, 0, 0, 0, 2, 5, 0] and end.tolist() == [0, 2, 0, 0, 5, 6, 0]
    for cid in ("32769-boundary-255|256", "empties-first-middle-last-1025", "5-atoms-5000-molecules"):
        batch, n, first, end = _bounds_case(cid)
        cnt = torch.bincount(batch, minlength=n)
        assert torch.equal((end - first).long(), cnt) and torch.equal(first.long()[cnt > 0], (torch.cumsum(cnt, 0) - cnt)[cnt > 0])
    assert int(_bounds_case("32769-boundary-255|256")[0][255]) + 1 == int(_bounds_case("32769-boundary-255|256")[0][256])
    for kind, n in INVALID:
        assert not fh.bounds_ref(*_invalid_batch(kind, n))[2], (kind, n)


@pytest.mark.parametrize("wd", (0.0, WD), ids=("wd0", "wd0.01"))
def test_flat_adam_ref_is_torch_adam_in_float64_on_cpu(wd):
    """``adam_ref`` in float64 against ``torch.optim.Adam`` in float64 over three steps to 1e-14.  ``adam_ref`` takes its bias
    corrections rounded to float32 (as the ABI does) while torch forms its own in double: torch's ``lr`` and ``eps`` of each step are
    set so that its formula WITH its own corrections is the reference's with the rounded ones —
    ``lr_t = lr (bc1 / bc1_32) (s_32 / s)``, ``eps_t = eps s_32 / s`` with ``s = sqrt(bc2)``: the identity is exact in real numbers."""
    gen = torch.Generator().manual_seed(3)
    n = 64
    p, m, v = torch.randn(n, generator=gen, dtype=torch.float64), torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    for step in (1, 2, 3):
        g = torch.randn(n, generator=gen, dtype=torch.float64) * 2.0 ** (torch.arange(n) % 21 - 10).double()
        hyper = fh.adam_hyper(LR, BETA1, BETA2, ADAM_EPS, wd, step, 0.25)
        bc1, s = hyper["bc1"], hyper["sqrt_bc2"]
        lr_t, eps_t = LR * (bc1 / fh.f32(bc1)) * (fh.f32(s) / s), ADAM_EPS * fh.f32(s) / s
        want = fh.torch_adam(p, g, m, v, hyper, step, torch.float64, lr=lr_t, eps=eps_t)
        got = fh.adam_ref(p, g, m, v, hyper)
        for name, a, b in zip("pmv", got, want):
            err = float((a - b).abs().max() / b.abs().max())
            assert err <= 1e-14, (step, name, err)
        p, m, v = got


def test_flat_clip_ref_is_torch_clip_grad_in_float64_on_cpu():
    """``clip_ref`` in float64 against ``torch.nn.utils.clip_grad_norm_`` / ``clip_grad_value_`` on the averaged gradient
    ``g grad_scale`` (a power of two: the scale commutes with both exactly), to 1e-14 (norm) and bit for bit (value)."""
    g = _clip_g(1028).double()
    g[5], g[6] = float("inf"), -0.0
    for gs in (1.0, 0.25):
        for clip in (fh.f32(0.3), 1e6):
            P = torch.nn.Parameter(torch.zeros_like(g))
            P.grad = g * gs
            torch.nn.utils.clip_grad_value_([P], clip)
            assert same_bits_64(fh.clip_ref(g, clip, fh.CLIP_VALUE, gs) * gs, P.grad), (gs, clip)
        gf = _clip_g(1028).double()
        for factor in (0.5, 2.0):
            clip = fh.f32(factor * float(torch.linalg.vector_norm(gf)) * gs)
            P = torch.nn.Parameter(torch.zeros_like(gf))
            P.grad = gf * gs
            total = torch.nn.utils.clip_grad_norm_([P], clip)
            t, coef, out = fh.clip_ref(gf, clip, fh.CLIP_NORM, gs)
            assert abs(float(t) - float(total)) <= 1e-14 * float(total)
            assert float(((out * gs) - P.grad).abs().max() / P.grad.abs().max()) <= 1e-14, (gs, factor)
            assert (float(coef) < 1) == (factor < 1) and (factor < 1 or torch.equal(out, gf))
    nan = torch.tensor([float("nan"), 2.0, -3.0, -0.0])
    assert same_bits(fh.clip_ref(nan, 1.0, fh.CLIP_VALUE, dtype=torch.float32), torch.tensor([float("nan"), 1.0, -1.0, -0.0]))


def same_bits_64(a, b) -> bool:
    return a.shape == b.shape and bool((a.contiguous().view(torch.int64) == b.contiguous().view(torch.int64)).all())


def test_flat_yardsticks_under_the_caps_on_cpu():
    """The float32 yardstick of every arithmetic case stays under the cap — ``MARGIN max(e32, 2**-23)`` is what decides, not the cap —
    and no reference tensor is identically zero."""
    cap = rh.CAP["grad"]
    for case in ADAM_CASES:
        if case.n == ADAM_STRIDE and (case.gs != 1.0 or case.step != 1):
            continue      # (the large buffers: two of the eight here, all of them in the GPU test)
        _, r64, e32 = _adam_ref(case)
        assert max(e32.values()) < cap, (case.id, e32)
        assert all(float(t.abs().max()) > 0 for t in r64.values()), case.id
    _adam_ref.cache_clear()
    for n, factor, gs in CLIP_CASES:
        g = _clip_g(n)
        clip = fh.f32(factor * float(torch.linalg.vector_norm(g.double())) * gs)
        t64, _, g64 = fh.clip_ref(g, clip, fh.CLIP_NORM, gs)
        t32, _, g32 = fh.clip_ref(g, clip, fh.CLIP_NORM, gs, torch.float32)
        e32 = _e32(dict(total=t32.view(1), g=g32), dict(total=t64.view(1), g=g64))
        assert max(e32.values()) < cap, (n, factor, gs, e32)
    for d_h, label, mode, norm in ADJOINT:
        a32, b32 = _adjoint_yardstick(d_h, norm if mode == fh.NORM else 1.0)
        assert abs(a32 - b32) / abs(b32) < cap and abs(b32) > 1, (d_h, label, a32, b32)
