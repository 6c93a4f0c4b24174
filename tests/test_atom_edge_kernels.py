"""The atom message in the edge kernels: the third mode of ``k_segment`` through ``dmpnn_message_fwd(flags = DMPNN_F_ATOM)`` and the
``MESSAGE`` variant of ``k_edge_bwd`` without the reverse row through ``dmpnn_atom_message_bwd`` (``tests/atom_harness.py``).

One hand-built batch: a single-atom molecule (in-degree 0), a chain, and stars whose centre has in-degree 4, 5, 6 and 7 — the last
specialised and the first generic bodies of both kernels (the forward switches on in-degrees 1 .. 6, the backward on 1 .. 4) — edges
shuffled.  Widths: 14 and 301 (the scalar build), 16, 256 | 260 and 512 | 516 (64 | 65 and 128 | 129 column groups of the vector
build), one case with padded leading dimensions, one batch without edges.

* forward: bit for bit the float32 sum of the incoming rows in increasing edge id;
* backward: against float64 at ``err <= min(MARGIN max(e32, 2**-23), 2e-5)``, ``e32`` the float32 run of the same transpose;
* the reference transpose is the exact adjoint of the reference message (float64, CPU);
* an asymmetric plan: the forward is the literal edge form ``M[e] = S[src e]``, the backward NaN.

MARGIN: the worst ``err / max(e32, 2**-23)`` of the backward cases on the MI355X is 0.87 (``h14``; 0.67 and 0.64 follow: the kernel
adds the rows of an atom in one order, float32 autograd in another, both float32 sums of at most 7 terms; the forward is bit-exact);
doubled and rounded up to a power of two: 2.
"""
import functools
import os

import pytest
import torch

import atom_harness as ah
import rows_harness as rh
from chemprop_amd import _lib
from conftest import GOLDEN_DIR, Golden

MARGIN = 2.0
gpu = pytest.mark.gpu
WIDTHS = (14, 301, 16, 256, 260, 512, 516)
CENTRES = (4, 5, 6, 7)
PADDED = [("h16-padded", 16, dict(ld_in=20, ld_out=24)), ("h14-padded-scalar", 14, dict(ld_in=15, ld_out=17))]
CASES = [(f"h{h}", h, {}) for h in WIDTHS] + PADDED


def bits(t):
    return t.contiguous().view(torch.int32)


@functools.lru_cache(maxsize=None)
def _graph(name):
    if name == "hand":
        pieces = [(1, []), (6, [(i, i + 1) for i in range(5)])] + [(d + 1, [(0, i) for i in range(1, d + 1)]) for d in CENTRES]
        return rh._graph(pieces, seed=4, shuffle=True)
    if name == "no-edges":
        return rh.degree_graph((0, 0, 0))
    if name == "garbage":
        return Golden(os.path.join(GOLDEN_DIR, "garbage_h24.npz")).bmg()
    raise KeyError(name)


_PLANS = {}


def _plan(name, dev):
    if name not in _PLANS:
        _PLANS[name] = rh.make_plan(_graph(name), dev)
    return _PLANS[name]


@functools.lru_cache(maxsize=None)
def _ref(h):
    """Inputs and references of one width — computed once, shared, never written to."""
    bmg = _graph("hand")
    gen = torch.Generator().manual_seed(300 + h)
    nE = int(bmg.edge_index.shape[1])
    scale = 1 + torch.arange(h).float() / h
    X, gM = torch.randn(nE, h, generator=gen) * scale, torch.randn(nE, h, generator=gen) * scale
    b64, b32 = ah.atom_message_bwd_ref(bmg, gM), ah.atom_message_bwd_ref(bmg, gM, torch.float32)
    return X, gM, ah.atom_message_seq32(bmg, X), b64, rh.yardstick(dict(gX=b64), dict(gX=b32))


def test_atom_edge_references_on_cpu():
    """The graph has the in-degrees the kernels switch on; the sequential float32 sum is the float32 run of the restatement bit for
    bit and float64's within float32; the transpose is the exact adjoint (``<gM, fwd(X)> == <bwd(gM), X>`` in float64); float32
    itself meets the cap on every width."""
    bmg = _graph("hand")
    deg = rh.in_degrees(bmg)
    assert {0, 1, 2, *CENTRES} == set(deg.tolist()) and int((deg == 0).sum()) == 1
    src, dst = bmg.edge_index
    rev = bmg.rev_edge_index
    assert torch.equal(src[rev], dst) and torch.equal(dst[rev], src) and torch.equal(rev[rev], torch.arange(rev.numel()))
    assert not torch.equal(dst, torch.sort(dst).values), "the edges are shuffled"
    for h in WIDTHS:
        X, gM, seq32, b64, e32 = _ref(h)
        assert torch.equal(bits(seq32), bits(ah.atom_message_ref(bmg, X, torch.float32)))
        f64 = ah.atom_message_ref(bmg, X)
        assert float((seq32.double() - f64).abs().max()) <= 8 * 2.0 ** -24 * float(f64.abs().max())
        a, b = float((gM.double() * f64).sum()), float((b64 * X.double()).sum())
        assert abs(a - b) <= 1e-12 * max(abs(a), abs(b)), (h, a, b)
        # the literal edge form is the same function on a symmetric graph
        assert torch.equal(ah.atom_message_literal(src, dst, X, int(bmg.V.shape[0])), f64)
        assert e32["gX"] < rh.CAP["grad"] and float(b64.abs().max()) > 0, (h, e32)
    g = _graph("garbage")
    assert not torch.equal(g.edge_index[0][g.rev_edge_index], g.edge_index[1]), "the garbage graph is not symmetric"
    assert "dmpnn_atom_message_bwd" in _lib.EXPORTS


@gpu
@pytest.mark.parametrize("cid,h,layout", CASES, ids=[c[0] for c in CASES])
def test_atom_message_fwd_and_bwd(cid, h, layout, gpu_device):
    bmg = _graph("hand")
    plan, _ = _plan("hand", gpu_device)
    X, gM, seq32, b64, e32 = _ref(h)
    rc, msg, out = ah.run_atom_message_fwd(gpu_device, plan, X, **layout)
    assert rc == 0, msg
    got = out.read("M")
    same = bits(got) == bits(seq32)
    assert bool(same.all()), f"{cid}: {int((~same).sum())} entries differ from the float32 sum in increasing edge id"
    rc, msg, out = ah.run_atom_message_bwd(gpu_device, plan, gM, **layout)
    assert rc == 0, msg
    fails, _ = ah.compare(f"atom_message_bwd-{cid}", dict(gX=out.read("gX")), dict(gX=b64), e32, MARGIN)
    assert not fails, "; ".join(fails)


@gpu
def test_atom_message_without_edges_and_flag_errors(gpu_device):
    """``n_edges == 0``: both entries succeed and write nothing.  ``DMPNN_F_ATOM | DMPNN_F_UNDIRECTED``: ``DMPNN_EINVAL`` with a
    message, nothing written."""
    plan, _ = _plan("no-edges", gpu_device)
    for h in (16, 14):
        rc, msg, out = ah.run_atom_message_fwd(gpu_device, plan, torch.zeros(0, h))
        assert rc == 0 and out.pristine(), msg
        rc, msg, out = ah.run_atom_message_bwd(gpu_device, plan, torch.zeros(0, h))
        assert rc == 0 and out.pristine(), msg
    plan, _ = _plan("hand", gpu_device)
    rc, msg, out = ah.run_atom_message_fwd(gpu_device, plan, _ref(16)[0], flags=_lib.F_ATOM | _lib.F_UNDIRECTED)
    assert rc == rh.EINVAL and "DMPNN_F_ATOM" in msg and out.pristine(), (rc, msg)


@gpu
def test_atom_message_on_an_asymmetric_plan(gpu_device):
    """The garbage golden's graph: the forward is the literal edge form (the float32 sum in increasing edge id, bit for bit), the
    backward poisons every entry with NaN."""
    bmg = _graph("garbage")
    plan, arr = _plan("garbage", gpu_device)
    assert int(arr["hdr"][0]) & 1, "the garbage graph is expected to be flagged asymmetric"
    src, dst = bmg.edge_index
    gen = torch.Generator().manual_seed(9)
    for h, layout in ((24, {}), (7, {}), (24, dict(ld_out=25))):
        X = torch.randn(plan.n_edges, h, generator=gen)
        rc, msg, out = ah.run_atom_message_fwd(gpu_device, plan, X, **layout)
        assert rc == 0, msg
        got = out.read("M")
        lit32 = ah.atom_message_literal(src, dst, X, plan.n_atoms, torch.float32)
        assert torch.equal(bits(got), bits(lit32)), "the literal edge form M[e] = S[src e], rows added in increasing edge id"
        lit64 = ah.atom_message_literal(src, dst, X, plan.n_atoms)
        assert float((got.double() - lit64).abs().max()) <= 32 * 2.0 ** -24 * float(lit64.abs().max())
        rc, msg, out = ah.run_atom_message_bwd(gpu_device, plan, X, **layout)
        assert rc == 0, msg
        assert bool(torch.isnan(out.read("gX")).all())
