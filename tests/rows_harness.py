"""Shared helpers of the row-kernel tests (``tests/test_rows_boundaries.py``, the rows-route gradients of
``tests/test_parity_gpu.py``): no fixtures, no pytest settings — a plain module.

Three layers:

* ``Mat`` / ``run_wgrad`` / ``run_edge_bwd`` / ``run_gather`` / ``run_update``: the five row-level entries of ``include/dmpnn.h`` the
  suite never called directly — ``dmpnn_linear_wgrad`` (+ ``dmpnn_linear_wgrad_ws_bytes``), ``dmpnn_message_bwd``,
  ``dmpnn_aggregate_bwd``, ``dmpnn_gather_rows``, ``dmpnn_update_fwd`` — through ctypes with the LAYOUT in the caller's hands: every
  operand has its own leading dimension and an element offset into a larger allocation (offset 1: a 4-byte aligned pointer, 2: 8-byte,
  0: 16-byte).  The padding columns of an input hold NaN (whatever reads them into a sum shows); an output lives in a buffer
  prefilled with one NaN bit pattern, and ``Mat.read`` fails unless every word outside ``[rows, width]`` — padding columns, the
  words before the pointer, a guard region behind the last row — still holds it bit for bit.
* ``run_linear`` / ``run_segment_fwd``: the forward counterparts — ``dmpnn_linear_fwd``, ``dmpnn_linear16_fwd`` (+ ``_ok``,
  ``_wsplit_bytes``), ``dmpnn_message_fwd``, ``dmpnn_aggregate_fwd`` — the same way (``tests/test_forward_rows_boundaries.py``), with
  ``linear_build`` / ``linear16_build``: the dispatch rules restated, to label a case by the kernel build it runs.
* ``degree_graph`` / ``chain_graph`` / ``csr_tables``: small symmetric molecular graphs (``BatchMolGraph.from_tensors``) with
  prescribed in-degrees, and the stable incoming-edge CSR the plan builds (``GraphPlan.arrays()`` on the device).
* ``wgrad_ref`` / ``message_bwd_ref`` / ``update_ref`` / ``linear_ref`` / ``segment_fwd_ref`` / ``compare``: the references in float64 — each runnable in float32 as the
  yardstick, what plain fp32 PyTorch gives on the very same inputs — and the rule of ``head_harness.compare`` restated for named
  tensors: unfloored error within ``min(MARGIN max(e32, 2**-23), cap)``.
"""
import ctypes as C
import math

import torch

from chemprop_amd import _lib
from conftest import TOL, parity_err_unfloored
from oracle import dmpnn_torch as ot

EPS32 = 2.0 ** -23
# the floored bars the suite already holds (tests/test_parity_gpu.py): the unfloored bar of a tensor never exceeds them
CAP = dict(grad=2e-5, fwd=TOL)
# One number for the row-kernel tests: the worst err / max(e32, 2**-23) observed on the MI355X, doubled, rounded up to a power of two
# (the measurement and the arithmetic: the docstring of tests/test_rows_boundaries.py).
MARGIN = 16.0

PREFILL = 0x7FC01234   # a quiet NaN no kernel writes (the library's own NaN is 0x7FC00000)
GUARD = 64             # words behind the last row of every buffer
EINVAL, ENOSPC = -1, -3


# ---- layout --------------------------------------------------------------------------------------------------------------------------
class Mat:
    """``[rows, width]`` floats at element ``off`` of an allocation of ``off + rows * ld + GUARD`` words (torch's allocations are
    at least 256-byte aligned: ``off`` alone decides the alignment of ``ptr``).  ``data``: an input (padding NaN); ``None``: an
    output, every word ``PREFILL``."""

    def __init__(self, dev, rows, width, ld=None, off=0, data=None):
        ld = width if ld is None else ld
        assert ld >= width and off >= 0
        self.rows, self.width, self.ld, self.off = rows, width, ld, off
        self.base = torch.full((off + rows * ld + GUARD,), PREFILL, dtype=torch.int32, device=dev)
        assert self.base.data_ptr() % 16 == 0
        if data is not None:
            assert tuple(data.shape) == (rows, width), (tuple(data.shape), rows, width)
            self.view().copy_(data.to(torch.float32))
        self.ptr = self.base.data_ptr() + 4 * off

    def view(self):
        body = self.base[self.off:self.off + self.rows * self.ld].view(torch.float32)
        return body.view(self.rows, self.ld)[:, :self.width]

    def untouched(self) -> bool:
        """Every word outside ``[rows, width]`` still holds the prefill."""
        b = self.base.cpu()
        keep = torch.ones(b.numel(), dtype=torch.bool)
        body = keep[self.off:self.off + self.rows * self.ld].view(self.rows, self.ld)
        body[:, :self.width] = False
        return bool((b[keep] == PREFILL).all())

    def pristine(self) -> bool:
        """Nothing was written at all."""
        return bool((self.base == PREFILL).all())

    def read(self, what="output") -> torch.Tensor:
        assert self.untouched(), f"{what}: a word outside [rows, width] (padding column, guard region) was written"
        return self.view().cpu().clone()


def _call(dev, fn, *args):
    """One C call on torch's current stream of ``dev`` -> (rc, message, launches): kernels the call launched."""
    from chemprop_amd import engine

    lib = _lib.load()
    with engine._OnDevice(dev):
        n0 = int(lib.dmpnn_last_launch_count())
        rc = int(fn(*args, engine._stream_ptr(dev)))
        n1 = int(lib.dmpnn_last_launch_count())
    torch.cuda.synchronize()
    return rc, lib.dmpnn_last_error_string().decode(errors="replace") if rc else "", n1 - n0


# ---- dmpnn_linear_wgrad --------------------------------------------------------------------------------------------------------------
def wgrad_inputs(M, N, K1, K2, n_src=None, seed=0, graded=False):
    """float32 CPU operands: column ``c`` of ``gZ`` and of ``[A1 || A2]`` scaled by ``1 + c / width`` (a transposed or shifted tile
    cannot pass); ``n_src``: ``A1`` has that many rows and ``gather`` (int32, repeating) picks ``M`` of them; ``graded``: column
    ``n`` of ``gZ`` scaled by ``2**-(n % 16)`` instead."""
    gen = torch.Generator().manual_seed(1234 + seed)
    K = K1 + K2
    gZ = torch.randn(M, N, generator=gen)
    if graded:
        gZ = gZ * (2.0 ** -(torch.arange(N) % 16).float())
    else:
        gZ = gZ * (1 + torch.arange(N).float() / N)
    A = torch.randn(n_src if n_src is not None else M, K, generator=gen) * (1 + torch.arange(K).float() / K)
    A1 = A[:, :K1].contiguous()
    gather = None
    if n_src is not None:
        assert K1 > 0
        gather = torch.randint(0, n_src, (M,), generator=gen, dtype=torch.int32)
        A2 = torch.randn(M, K2, generator=gen) * (1 + (K1 + torch.arange(K2).float()) / K) if K2 else None
    else:
        A2 = A[:, K1:].contiguous() if K2 else None
    return dict(gZ=gZ, A1=A1, A2=A2, gather=gather)


def wgrad_ref(inp, dtype=torch.float64):
    """``gW = gZ^T [A1[g] || A2]``, ``gb = colsum(gZ)`` in ``dtype`` on the CPU."""
    gZ, A1 = inp["gZ"].to(dtype), inp["A1"].to(dtype)
    if inp["gather"] is not None:
        A1 = A1[inp["gather"].long()]
    A = A1 if inp["A2"] is None else torch.cat((A1, inp["A2"].to(dtype)), 1)
    return dict(gW=gZ.t() @ A, gb=gZ.sum(0))


def run_wgrad(dev, inp, want_gW=True, want_gb=True, ldz=None, lda1=None, lda2=None, ldgw=None, off=0, ws_short=0):
    """One ``dmpnn_linear_wgrad`` call.  ``off``: the element offset of ``gZ``, ``A1`` and ``A2`` alike.  The workspace is exactly
    ``dmpnn_linear_wgrad_ws_bytes(...)`` bytes (less ``ws_short``) at the front of a larger allocation.  Returns ``rc``, ``msg``,
    ``pipe`` (``f16``: operand split + product + reduce, three launches; ``f32``: product + reduce; ``memset``: none), the
    outputs read back (padding and guards checked), ``ws_tail_ok`` and the ``Mat`` objects."""
    lib = _lib.load()
    gZ, A1, A2, gather = inp["gZ"], inp["A1"], inp["A2"], inp["gather"]
    M, N, K1 = int(gZ.shape[0]), int(gZ.shape[1]), int(A1.shape[1])
    K2 = int(A2.shape[1]) if A2 is not None else 0
    mz = Mat(dev, M, N, ldz, off, gZ)
    m1 = Mat(dev, int(A1.shape[0]), K1, lda1, off, A1)
    m2 = Mat(dev, M, K2, lda2, off, A2) if K2 else None
    gi = gather.to(dev) if gather is not None else None
    oW = Mat(dev, N, K1 + K2, ldgw)
    ob = Mat(dev, 1, N)
    g = _lib.GemmArgs()
    g.M, g.N, g.K1, g.K2 = M, N, K1, K2
    g.A1, g.lda1 = m1.ptr, m1.ld
    if gi is not None:
        g.gather1, g.gather1_rows = gi.data_ptr(), int(A1.shape[0])
    if m2 is not None:
        g.A2, g.lda2 = m2.ptr, m2.ld
    nb = int(lib.dmpnn_linear_wgrad_ws_bytes(M, N, K1 + K2, 1 if want_gb else 0))
    tail = 4096
    ws = torch.full((nb + tail,), 0xA5, dtype=torch.uint8, device=dev)
    rc, msg, launches = _call(dev, lib.dmpnn_linear_wgrad, C.byref(g), mz.ptr, mz.ld, oW.ptr if want_gW else None, oW.ld,
                              ob.ptr if want_gb else None, ws.data_ptr(), nb - ws_short)
    return dict(rc=rc, msg=msg, pipe={0: "memset", 2: "f32", 3: "f16"}.get(launches, f"{launches} launches"), oW=oW, ob=ob,
                ws_bytes=nb, ws_tail_ok=bool((ws[nb - ws_short:] == 0xA5).all()), ws_pristine=bool((ws == 0xA5).all()),
                keep=(mz, m1, m2, gi))


# ---- graphs --------------------------------------------------------------------------------------------------------------------------
def _graph(pieces, seed, shuffle):
    """``pieces``: per molecule (n_atoms, [(u, v) bonds, molecule-local]).  Directed edges interleaved ``(u->v, v->u)`` as the
    featurizers emit them, then (``shuffle``) permuted as a whole, ``rev`` with them."""
    from chemprop_amd.data import BatchMolGraph

    src, dst, batch, o = [], [], [], 0
    for m, (n, bonds) in enumerate(pieces):
        for u, v in bonds:
            src += [o + u, o + v]
            dst += [o + v, o + u]
        batch += [m] * n
        o += n
    nE = len(src)
    src, dst = torch.tensor(src, dtype=torch.int64), torch.tensor(dst, dtype=torch.int64)
    rev = torch.arange(nE).view(-1, 2).flip(1).reshape(-1) if nE else torch.zeros(0, dtype=torch.int64)
    if shuffle and nE:
        p = torch.randperm(nE, generator=torch.Generator().manual_seed(99 + seed))   # new position k holds old edge p[k]
        inv = torch.empty_like(p)
        inv[p] = torch.arange(nE)
        src, dst, rev = src[p], dst[p], inv[rev[p]]
    return BatchMolGraph.from_tensors(torch.zeros(o, 1), torch.zeros(nE, 1), torch.stack((src, dst)), rev,
                                      torch.tensor(batch, dtype=torch.int64), len(pieces))


def degree_graph(degrees, seed=0, shuffle=True):
    """A symmetric graph with one piece per entry of ``degrees``: an isolated atom (0), the two atoms of a single bond (1), a star
    whose centre has that in-degree (2: a chain of three) — so the in-degrees that occur are ``set(degrees) | {1}``."""
    pieces = []
    for d in degrees:
        pieces.append((1, []) if d == 0 else (2, [(0, 1)]) if d == 1 else (d + 1, [(0, i) for i in range(1, d + 1)]))
    return _graph(pieces, seed, shuffle)


def chain_graph(n_chains, length, seed=0, shuffle=True):
    """``n_chains`` chains of ``length`` atoms each."""
    return _graph([(length, [(i, i + 1) for i in range(length - 1)])] * n_chains, seed, shuffle)


def in_degrees(bmg):
    return torch.bincount(bmg.edge_index[1], minlength=int(bmg.V.shape[0]))


def csr_tables(bmg):
    """The plan's CSR-row tables on the CPU: ``perm`` (row -> edge: the edges by destination, stable), ``inv`` (edge -> row)."""
    dst = bmg.edge_index[1]
    perm = torch.sort(dst, stable=True).indices
    inv = torch.empty_like(perm)
    inv[perm] = torch.arange(perm.numel())
    return dict(perm=perm, inv=inv)


def make_plan(bmg, dev):
    """A full plan of ``bmg`` on the device (the batch moved there) -> (plan, its arrays on the CPU as int64)."""
    from chemprop_amd import engine

    b = bmg.__copy__()
    b.to(dev)
    plan = engine.GraphPlan.from_bmg(b)
    return plan, {k: v.long() for k, v in plan.arrays().items()}


# ---- dmpnn_message_bwd / dmpnn_aggregate_bwd -------------------------------------------------------------------------------------------
def message_bwd_ref(bmg, gM, dtype=torch.float64):
    """The transpose of ``oracle.dmpnn_torch.message`` by autograd in ``dtype``."""
    src, dst = bmg.edge_index
    H = torch.zeros(gM.shape, dtype=dtype, requires_grad=True)
    ot.message(H, src, dst, bmg.rev_edge_index, int(bmg.V.shape[0])).backward(gM.to(dtype))
    return H.grad


def adjoint_gap(bmg, h, seed=0):
    """``|<gM, message(H)> - <message_bwd_ref(gM), H>|`` relative to the larger of the two, in float64."""
    gen = torch.Generator().manual_seed(7 + seed)
    nE = int(bmg.edge_index.shape[1])
    H, gM = torch.randn(nE, h, generator=gen, dtype=torch.float64), torch.randn(nE, h, generator=gen, dtype=torch.float64)
    src, dst = bmg.edge_index
    a = float((gM * ot.message(H, src, dst, bmg.rev_edge_index, int(bmg.V.shape[0]))).sum())
    b = float((message_bwd_ref(bmg, gM) * H).sum())
    return abs(a - b) / max(abs(a), abs(b), 1e-300)


def run_edge_bwd(dev, plan, which, gin, ld_in=None, ld_out=None, off_in=0, off_out=0):
    """``dmpnn_message_bwd`` (``which == "message"``: ``gin`` is ``gM [E, h]``) or ``dmpnn_aggregate_bwd`` (``"aggregate"``: ``gMv
    [V, h]``) -> (rc, msg, the output ``Mat`` of ``[E, h]``)."""
    lib = _lib.load()
    h = int(gin.shape[1])
    mi = Mat(dev, int(gin.shape[0]), h, ld_in, off_in, gin)
    mo = Mat(dev, plan.n_edges, h, ld_out, off_out)
    fn = lib.dmpnn_message_bwd if which == "message" else lib.dmpnn_aggregate_bwd
    rc, msg, _ = _call(dev, fn, plan.buf.data_ptr(), plan.n_atoms, plan.n_edges, h, mi.ptr, mi.ld, mo.ptr, mo.ld)
    return rc, msg, mo


# ---- dmpnn_gather_rows -----------------------------------------------------------------------------------------------------------------
def run_gather(dev, X, idx, ldx=None, ldo=None, off_x=0, off_o=0):
    lib = _lib.load()
    n_src, d = int(X.shape[0]), int(X.shape[1])
    mx = Mat(dev, n_src, d, ldx, off_x, X)
    mo = Mat(dev, int(idx.numel()), d, ldo, off_o)
    ii = idx.to(torch.int32).to(dev)
    rc, msg, _ = _call(dev, lib.dmpnn_gather_rows, mx.ptr, mx.ld, n_src, ii.data_ptr() if ii.numel() else None, int(ii.numel()), d,
                       mo.ptr, mo.ld)
    return rc, msg, mo


# ---- dmpnn_update_fwd ------------------------------------------------------------------------------------------------------------------
UPDATE_ACTS = ("relu", "leakyrelu", "tanh", "elu", "prelu")
LEAKY_SLOPE, PRELU_SLOPE = 0.1, 0.25


def update_inputs(n_edges, d_h, bias, seed=0):
    """``M``, ``H0`` in CSR-row order, ``W_h`` in ``nn.Linear``'s range with rows scaled by ``1 + n / d_h``, ``b_h`` or ``None``."""
    gen = torch.Generator().manual_seed(4321 + seed)
    k = 1.0 / math.sqrt(d_h)
    W = (2 * torch.rand(d_h, d_h, generator=gen) - 1) * k * (1 + torch.arange(d_h).float() / d_h).view(-1, 1)
    return dict(M=torch.randn(n_edges, d_h, generator=gen), H0=torch.randn(n_edges, d_h, generator=gen), W_h=W,
                b_h=(2 * torch.rand(d_h, generator=gen) - 1) * k if bias else None)


def update_ref(bmg, perm, inp, act, dtype=torch.float64):
    """One depth step in ``dtype`` from ``oracle.dmpnn_torch.update`` / ``message`` / ``segment_sum_dst`` in the caller's edge order,
    handed back in CSR-row order (row ``i`` is edge ``perm[i]``): ``H_out``, ``M_next``, ``Mv``."""
    perm = perm.long()
    inv = torch.empty_like(perm)
    inv[perm] = torch.arange(perm.numel())
    f = lambda t: None if t is None else t.to(dtype)
    tau = ot.activation_fn(act, torch.tensor([PRELU_SLOPE], dtype=dtype))
    w = ot.MPWeights(W_i=None, W_h=f(inp["W_h"]), W_o=None, b_o=None, b_h=f(inp["b_h"]))
    src, dst = bmg.edge_index
    nV = int(bmg.V.shape[0])
    H = ot.update(f(inp["M"])[inv], f(inp["H0"])[inv], w, tau)   # (edge order)
    return dict(H_out=H[perm], M_next=ot.message(H, src, dst, bmg.rev_edge_index, nV)[perm], Mv=ot.segment_sum_dst(H, dst, nV))


def run_update(dev, plan, inp, act, outputs=("H_out", "M_next", "Mv"), d_h=None, ld=None, off=0, only=None):
    """One ``dmpnn_update_fwd`` call -> (rc, msg, {name: Mat}) — ``ld`` / ``off``: of every edge and atom tensor alike, or of the
    tensors ``only`` names (``M``, ``H0``, ``H_out``, ``M_next``, ``Mv``; the others dense and aligned); ``d_h``: the width handed to
    the call (the tensors are as wide as ``inp`` makes them)."""
    lib = _lib.load()
    nE, w = int(inp["M"].shape[0]), int(inp["M"].shape[1])
    d_h = w if d_h is None else d_h
    lay = lambda k: (ld, off) if (only is None or k in only) else (None, 0)
    mM, mH0 = Mat(dev, nE, w, *lay("M"), inp["M"]), Mat(dev, nE, w, *lay("H0"), inp["H0"])
    W = inp["W_h"].to(dev).contiguous()
    b = inp["b_h"].to(dev) if inp["b_h"] is not None else None
    outs = dict(H_out=Mat(dev, nE, w, *lay("H_out")), M_next=Mat(dev, nE, w, *lay("M_next")), Mv=Mat(dev, plan.n_atoms, w, *lay("Mv")))
    p = lambda k: outs[k].ptr if k in outputs else None
    slope_t = torch.tensor([PRELU_SLOPE], device=dev) if act == "prelu" else None
    rc, msg, _ = _call(dev, lib.dmpnn_update_fwd, plan.buf.data_ptr(), plan.n_atoms, plan.n_edges, d_h, mM.ptr, mM.ld, mH0.ptr, mH0.ld,
                       W.data_ptr(), b.data_ptr() if b is not None else None, p("H_out"), outs["H_out"].ld, p("M_next"),
                       outs["M_next"].ld, p("Mv"), outs["Mv"].ld, _lib.ACT[act], LEAKY_SLOPE if act == "leakyrelu" else 0.0,
                       slope_t.data_ptr() if slope_t is not None else None)
    return rc, msg, outs


# ---- dmpnn_linear_fwd / dmpnn_linear16_fwd -------------------------------------------------------------------------------------------
LINEAR_ACTS = ("none", "relu", "leakyrelu", "prelu", "tanh", "elu")
SIMPLE_ACTS = ("none", "relu", "leakyrelu", "prelu")   # one branch-free formula in the fp32 kernel's epilogue; exact on load in k_segment
LINEAR_TENSORS = ("A1", "A2", "W", "Cadd", "C", "Zpre")
DECOY_SLOPE = 0.7   # what ``act_slope`` holds when the slope travels through ``act_slope_ptr``: the pointer has to win


def act_slope(act):
    return {"leakyrelu": LEAKY_SLOPE, "prelu": PRELU_SLOPE, "relu": 0.0, "none": 1.0}.get(act)


def linear_inputs(M, N, K1, K2, n_src=None, seed=0, graded=None, bias=True, cadd=True):
    """float32 CPU operands of ``C = tau([A1[g] || A2] W^T + bias + Cadd)``: row ``n`` of ``W`` (``nn.Linear``'s range) scaled by
    ``1 + n / N``, column ``k`` of ``[A1 || A2]`` by ``1 + k / K`` (a transposed, shifted or swapped tile cannot pass); ``K1 == 0``:
    the single operand sits in the ``A2`` slot; ``n_src``: ``A1`` has that many rows and ``gather`` (int32, repeating) picks ``M`` of
    them.  ``graded``: ``"rows"`` scales row ``r`` of the operands by ``2**-(r % 16)``; ``("groups", width, exps)`` scales the columns
    ``[g width, (g + 1) width)`` of ``[A1 || A2]`` by ``2**exps[g]`` (``None``: that group is all zero)."""
    gen = torch.Generator().manual_seed(4242 + seed)
    K = K1 + K2
    k = 1.0 / math.sqrt(K)
    W = (2 * torch.rand(N, K, generator=gen) - 1) * k * (1 + torch.arange(N).float() / N).view(-1, 1)
    col = 1 + torch.arange(K).float() / K
    if isinstance(graded, tuple):
        _, width, exps = graded
        assert len(exps) == -(-K // width), (K, width, exps)
        col = col * torch.tensor([0.0 if e is None else 2.0 ** e for e in exps]).repeat_interleave(width)[:K]
    rows = (lambda n: (2.0 ** -(torch.arange(n) % 16).float()).view(-1, 1)) if graded == "rows" else (lambda n: 1.0)
    A1 = A2 = gather = None
    if n_src is not None:
        assert K1 > 0
        A1 = torch.randn(n_src, K1, generator=gen) * col[:K1] * rows(n_src)
        gather = torch.randint(0, n_src, (M,), generator=gen, dtype=torch.int32)
    elif K1:
        A1 = torch.randn(M, K1, generator=gen) * col[:K1] * rows(M)
    if K2:
        A2 = torch.randn(M, K2, generator=gen) * col[K1:] * rows(M)
    return dict(M=M, N=N, K1=K1, K2=K2, A1=A1, A2=A2, gather=gather, W=W, bias=(2 * torch.rand(N, generator=gen) - 1) * k if bias else None,
                Cadd=torch.randn(M, N, generator=gen) if cadd else None)


def linear_ref(inp, act, dtype=torch.float64):
    """``Zpre = [A1[g] || A2] W^T + bias + Cadd`` and ``C = tau(Zpre)`` in ``dtype`` on the CPU.  A gather index equal to the number
    of source rows stands for a row of zeros (``include/dmpnn.h``: an index beyond ``gather1_rows`` reads zeros)."""
    f = lambda t: None if t is None else t.to(dtype)
    parts = []
    if inp["A1"] is not None:
        a = f(inp["A1"])
        if inp["gather"] is not None:
            a = torch.cat((a, torch.zeros(1, a.shape[1], dtype=dtype)))[inp["gather"].long()]
        parts.append(a)
    if inp["A2"] is not None:
        parts.append(f(inp["A2"]))
    Z = torch.nn.functional.linear(torch.cat(parts, 1), f(inp["W"]), f(inp["bias"]))
    if inp["Cadd"] is not None:
        Z = Z + f(inp["Cadd"])
    return dict(C=ot.activation_fn(act, torch.tensor([PRELU_SLOPE], dtype=dtype))(Z), Zpre=Z)


def linear_layout(inp, ld=None, off=None):
    """(ld, off) of the six tensors of a contraction call, the defaults (dense, aligned) filled in."""
    K = inp["K1"] + inp["K2"]
    width = dict(A1=inp["K1"], A2=inp["K2"], W=K, Cadd=inp["N"], C=inp["N"], Zpre=inp["N"])
    ld, off = dict(ld or {}), dict(off or {})
    assert set(ld) <= set(width) and set(off) <= set(width), (ld, off)
    return {k: ld.get(k, width[k]) for k in width}, {k: off.get(k, 0) for k in width}


def run_linear(dev, inp, act="none", pipe="f32", want=("C", "Zpre"), ld=None, off=None, slope_ptr=False, gather_rows=None, a1_tail=0,
               wsplit_ready=0, ws=None, ws_short=0, override=None):
    """One ``dmpnn_linear_fwd`` (``pipe == "f32"``) or ``dmpnn_linear16_fwd`` (``"f16"``) call.  ``ld`` / ``off``: per tensor of
    ``LINEAR_TENSORS``; ``slope_ptr``: the slope travels through ``act_slope_ptr`` (``act_slope`` holds a decoy; PReLU always does);
    ``gather_rows``: what ``gather1_rows`` says (default: the rows of ``A1``); ``a1_tail``: NaN rows stored behind the source rows;
    ``ws``: the workspace of an earlier call (else exactly ``dmpnn_linear16_wsplit_bytes`` bytes, less ``ws_short``, at the front of
    a larger ``0xA5`` allocation); ``override``: fields of ``dmpnn_gemm_args`` set after everything else (argument-error cases)."""
    lib = _lib.load()
    M, N, K1, K2 = inp["M"], inp["N"], inp["K1"], inp["K2"]
    lds, offs = linear_layout(inp, ld, off)
    mk = lambda k, rows, width, data=None: Mat(dev, rows, width, lds[k], offs[k], data)
    m1 = m2 = mc = None
    if K1:
        a1 = inp["A1"] if not a1_tail else torch.cat((inp["A1"], torch.full((a1_tail, K1), float("nan"))))
        m1 = mk("A1", int(a1.shape[0]), K1, a1)
    if K2:
        m2 = mk("A2", M, K2, inp["A2"])
    mw = mk("W", N, K1 + K2, inp["W"])
    if inp["Cadd"] is not None:
        mc = mk("Cadd", M, N, inp["Cadd"])
    outs = dict(C=mk("C", M, N), Zpre=mk("Zpre", M, N))
    gi = inp["gather"].to(dev) if inp["gather"] is not None else None
    b = inp["bias"].to(dev) if inp["bias"] is not None else None
    use_ptr = slope_ptr or act == "prelu"
    st = torch.tensor([act_slope(act) or 0.0], device=dev) if use_ptr else None
    g = _lib.GemmArgs()
    g.M, g.N, g.K1, g.K2 = M, N, K1, K2
    if m1 is not None:
        g.A1, g.lda1 = m1.ptr, m1.ld
    if gi is not None:
        g.gather1, g.gather1_rows = gi.data_ptr(), int(inp["A1"].shape[0]) if gather_rows is None else gather_rows
    if m2 is not None:
        g.A2, g.lda2 = m2.ptr, m2.ld
    g.W, g.ldw = mw.ptr, mw.ld
    g.bias = b.data_ptr() if b is not None else None
    if mc is not None:
        g.Cadd, g.ldcadd = mc.ptr, mc.ld
    if "C" in want:
        g.C, g.ldc = outs["C"].ptr, outs["C"].ld
    if "Zpre" in want:
        g.Zpre, g.ldz = outs["Zpre"].ptr, outs["Zpre"].ld
    g.act = _lib.ACT[act]
    g.act_slope = DECOY_SLOPE if use_ptr else (act_slope(act) or 0.0)
    g.act_slope_ptr = st.data_ptr() if st is not None else None
    for k, v in (override or {}).items():
        setattr(g, k, v)
    res = dict(outs=outs, ws=None, ws_bytes=0, ws_tail_ok=True, ws_pristine=True, keep=(m1, m2, mw, mc, gi, b, st))
    if pipe == "f16":
        nb = int(lib.dmpnn_linear16_wsplit_bytes(N, K1 + K2))
        if ws is None:
            ws = torch.full((nb + 4096,), 0xA5, dtype=torch.uint8, device=dev)
        assert ws.numel() == nb + 4096
        rc, msg, launches = _call(dev, lib.dmpnn_linear16_fwd, C.byref(g), ws.data_ptr(), nb - ws_short, wsplit_ready)
        res.update(ws=ws, ws_bytes=nb, ws_tail_ok=bool((ws[nb - ws_short:] == 0xA5).all()), ws_pristine=bool((ws == 0xA5).all()))
    else:
        rc, msg, launches = _call(dev, lib.dmpnn_linear_fwd, C.byref(g))
    res.update(rc=rc, msg=msg, launches=launches)
    return res


def _cdiv(a, b):
    return -(-a // b)


def linear_g(inp, ld=None, off=None, want=("C", "Zpre")):
    """``pick_g`` and the ``vec_c`` rule of ``launch_linear_ex`` restated -> (G, has_a2) of a call (labels and the coverage check
    only).  An element offset of 0 / 2 / 1 is a 16- / 8- / 4-byte aligned pointer."""
    lds, offs = linear_layout(inp, ld, off)
    N, K1, K2 = inp["N"], inp["K1"], inp["K2"]
    al = lambda k, B: (4 * offs[k]) % B == 0
    a1, a2 = ("A1", "A2") if K1 else ("A2", "A1")   # K1 == 0: the single operand is moved into the A1 slot
    if not K1:
        K1, K2 = K2, 0
    has_a2 = K2 > 0
    if not (N % 4 == 0 and all(lds[k] % 4 == 0 and al(k, 16) for k in want)):
        return 1, has_a2
    for G in (4, 2):
        ok = K1 % G == 0 and K2 % G == 0 and lds["W"] % G == 0 and al("W", 4 * G) and lds[a1] % G == 0 and al(a1, 4 * G)
        if has_a2:
            ok = ok and lds[a2] % G == 0 and al(a2, 4 * G)
        if inp["Cadd"] is not None:
            ok = ok and lds["Cadd"] % G == 0 and al("Cadd", 4 * G) and N % G == 0
        if ok:
            return G, has_a2
    return 1, has_a2


def linear_build(M, N, G, has_a2):
    """``pick_wn`` / ``pick_rt`` of ``csrc/dmpnn_gemm.hip`` restated -> ``(RT, WN, variant)`` of ``k_gemm<RT, WN, G, HAS_A2, EPI_PLAIN>``;
    variant: ``G4`` (one operand), ``G4+A2``, ``G2``, ``G1`` (the last two are two-operand builds whatever ``has_a2``)."""
    cost = {wn: _cdiv(N, 64 * wn) * wn for wn in (5, 4, 2, 1)}
    wn = min((5, 4, 2, 1), key=lambda w: (cost[w], -w))          # the first of 5, 4, 2, 1 with the least padded width
    row_tiles = _cdiv(M, 16)
    if row_tiles * _cdiv(N, 64 * wn) <= 128:                     # a short matrix: one workgroup per 64-column slice
        wn = next((w for w in (1, 2, 4) if w < wn and cost[w] == cost[wn] and row_tiles * _cdiv(N, 64 * w) <= 512), wn)
    ncb = _cdiv(N, 64 * wn)
    rt, best = 3, float("inf")
    for r in (3, 2, 1):
        c = _cdiv(_cdiv(M, 16 * r) * ncb, 256) * (r + 0.3)
        if c < best - 1e-9:
            rt, best = r, c
    if rt == 2 and G != 4:
        rt = 3
    return rt, wn, ("G4+A2" if has_a2 else "G4") if G == 4 else f"G{G}"


def linear16_build(M, N):
    """The ``WN`` / ``one_group`` rule of ``launch_linear16`` restated -> ``(WN, GC)`` of ``k_rows16<WN, GC>``."""
    col_blocks = _cdiv(N, 320)
    return _cdiv(N, 64 * col_blocks), 12 if _cdiv(M, 48) * col_blocks <= 512 else 4


# ---- dmpnn_message_fwd / dmpnn_aggregate_fwd -------------------------------------------------------------------------------------------
def segment_fwd_ref(bmg, Hin, which, act="none", undirected=False, dtype=torch.float64):
    """``M = message(H')`` (``which == "message"``) or ``Mv = segment_sum_dst(H')`` (``"aggregate"``) of ``H' = tau(Hin)``, averaged
    with its reverse row when ``undirected`` — ``oracle.dmpnn_torch`` in ``dtype``, incoming rows added in increasing edge id."""
    src, dst = bmg.edge_index
    nV = int(bmg.V.shape[0])
    H = ot.activation_fn(act, torch.tensor([PRELU_SLOPE], dtype=dtype))(Hin.to(dtype))
    if undirected:
        H = (H + H[bmg.rev_edge_index]) / 2
    return ot.message(H, src, dst, bmg.rev_edge_index, nV) if which == "message" else ot.segment_sum_dst(H, dst, nV)


def run_segment_fwd(dev, plan, which, Hin, act="none", slope=0.0, slope_ptr=None, undirected=False, ld_in=None, ld_out=None, off_in=0,
                    off_out=0):
    """``dmpnn_message_fwd`` (``which == "message"`` -> ``M [E, h]``) or ``dmpnn_aggregate_fwd`` (``"aggregate"`` -> ``Mv [V, h]``) on
    ``Hin [E, h]`` -> (rc, msg, the output ``Mat``).  ``slope_ptr``: a value placed on the device for ``act_slope_ptr``."""
    lib = _lib.load()
    h = int(Hin.shape[1])
    mi = Mat(dev, int(Hin.shape[0]), h, ld_in, off_in, Hin)
    mo = Mat(dev, plan.n_edges if which == "message" else plan.n_atoms, h, ld_out, off_out)
    st = torch.tensor([slope_ptr], device=dev) if slope_ptr is not None else None
    sp = st.data_ptr() if st is not None else None
    head = (plan.buf.data_ptr(), plan.n_atoms, plan.n_edges, h, mi.ptr, mi.ld, mo.ptr, mo.ld, _lib.ACT[act], slope, sp)
    if which == "message":
        rc, msg, _ = _call(dev, lib.dmpnn_message_fwd, *head, _lib.F_UNDIRECTED if undirected else 0)
    else:
        assert not undirected, "dmpnn_aggregate_fwd has no flags"
        rc, msg, _ = _call(dev, lib.dmpnn_aggregate_fwd, *head)
    return rc, msg, mo


# ---- the comparison ------------------------------------------------------------------------------------------------------------------
def yardstick(ref64: dict, ref32: dict) -> dict:
    """Per tensor the unfloored error of the float32 run against the float64 one."""
    return {k: parity_err_unfloored(ref32[k].double().numpy(), ref64[k].numpy()) for k in ref64}


def compare(case_id, got: dict, ref: dict, e32: dict, kinds, margin=None, report=print) -> list:
    """Every tensor of ``got`` against ``ref`` (float64), every entry: finite wherever the reference is, ``err = max|got - ref| /
    max|ref|`` (exactly 0 where ``max|ref|`` is 0) within ``min(margin max(e32, 2**-23), cap)``, ``cap`` by ``kinds`` (``grad`` /
    ``fwd``: one for all, or per name).  Reports one line per tensor BEFORE judging; returns the failures (empty: all held)."""
    margin = MARGIN if margin is None else margin
    fails = []
    for k in got:
        g, r = got[k].double().reshape(-1), ref[k].double().reshape(-1)
        assert g.shape == r.shape, (case_id, k, tuple(got[k].shape), tuple(ref[k].shape))
        assert bool(torch.isfinite(r).all()), (case_id, k, "the reference is not finite")
        if not bool(torch.isfinite(g).all()):
            report(f"ROWSBAR {case_id} {k} nonfinite")
            fails.append(f"{k}: not finite where the reference is")
            continue
        err = parity_err_unfloored(g.numpy(), r.numpy())
        scale = float(r.abs().max()) if r.numel() else 0.0
        cap = CAP[kinds if isinstance(kinds, str) else kinds[k]]
        bar = 0.0 if scale == 0.0 else min(margin * max(e32[k], EPS32), cap)
        ratio = err / max(e32[k], EPS32)
        report(f"ROWSBAR {case_id} {k} err={err:.3e} e32={e32[k]:.3e} ratio={ratio:.2f} bar={bar:.3e} maxref={scale:.3e}")
        if not err <= bar:
            fails.append(f"{k}: err {err:.3e} > bar {bar:.3e} (fp32 yardstick {e32[k]:.3e}, ratio {ratio:.1f}, max|ref| {scale:.3e})")
    return fails


def row_errors(got, ref):
    """Per output row ``n``: ``max_k |got - ref| / max_k |ref|`` (float64 tensors ``[N, K]``)."""
    return (got.double() - ref).abs().max(1).values / ref.abs().max(1).values
