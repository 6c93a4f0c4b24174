"""K0 for a batch that carries the host's tile table (``data.BatchMolGraph.plan_table``) and the one-pass weight split.

* the split buffer and ``inv_scale`` the split kernels write, byte for byte against a numpy statement of the layout and of the
  arithmetic (``x s -> hi -> x s - hi -> lo`` under ``scale_for`` of the row maximum): through ``dmpnn_linear16_fwd`` (one matrix of
  any shape) and through the tile kernel's training forward (six jobs: a column block with its scale taken over the whole row, two
  transposed jobs);
* the module forward of an own batch (table from the host, batch vector validated beside it) ``torch.equal`` to the forward of the
  same five tensors through ``from_tensors`` (K0 plans from the batch vector on the device), on the slow path and on the steady one;
* a batch corrupted in place is NaN on both, never a finite number from a table that no longer describes it.
"""
from __future__ import annotations

import copy
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


# ---- the split, stated in numpy ---------------------------------------------------------------------------------------------------
def _al256(x):
    return (x + 255) // 256 * 256


def _scale_for(mx):
    """``scale_for`` (csrc/dmpnn_mega16_impl.hpp): the power of two that puts mx at [2^13, 2^14), exponent within +-126; 1 for 0 / inf."""
    mx = mx.astype(np.float32)
    ok = (mx > 0) & (mx < np.float32(3.0e38))
    _, e = np.frexp(np.where(ok, mx, np.float32(1)))
    k = np.clip(14 - e, -126, 126)
    return np.where(ok, np.ldexp(np.float32(1), k), np.float32(1)).astype(np.float32)


def split_ref(W, nc, scale_over=None):
    """W [N, K] fp32 (element (n, k) of the job) -> (bytes of the fragment-major split buffer [T][c][hi|lo][lg][li][8 halfs] over whole
    column tiles and chunks, inv_scale [N]).  ``scale_over`` [N, Ks]: the columns the row scale is taken over (default: W)."""
    N, K = W.shape
    NT = (N + 15) // 16
    with np.errstate(all="ignore"):
        mx = np.fmax.reduce(np.abs(W if scale_over is None else scale_over), axis=1, initial=np.float32(0))   # (fmaxf: NaN is skipped)
        s = _scale_for(mx)
        x = np.zeros((NT * 16, nc * 32), dtype=np.float32)
        x[:N, :K] = W * s[:, None]
        hi = x.astype(np.float16)
        lo = (x - hi.astype(np.float32)).astype(np.float16)
        inv = (np.float32(1) / s).astype(np.float32)
    lo_bits = lo.view(np.uint16)
    # inf - inf: IEEE 754 leaves the sign and payload of an invalid operation's NaN open and the host's differs from the device's;
    # gfx950's v_sub_f32 gives 0xFFC00000, narrowed 0xFE00 (measured on the split kernels before and after the one-pass rewrite)
    lo_bits[np.isnan(lo)] = 0xFE00
    frag = lambda a: a.reshape(NT, 16, nc, 4, 8).transpose(0, 2, 3, 1, 4)   # [T][li][c][lg][j] -> [T][c][lg][li][j]
    out = np.stack([frag(hi.view(np.uint16)), frag(lo_bits)], axis=2)      # [T][c][part][lg][li][j]
    return np.ascontiguousarray(out).view(np.uint8).reshape(-1), inv


def _special_rows(W, gen):
    """An all-zero row, rows holding +inf / -inf among ordinary values, a row of subnormals, a row of huge and tiny values."""
    N, K = W.shape
    W = W.clone()
    W[1 % N] = 0.0
    if N > 4:
        W[2, K // 2] = float("inf")
        W[3, 0] = float("-inf")
        W[4] = torch.rand(K, generator=gen) * 1e-40
    if N > 6:
        W[5] = torch.randn(K, generator=gen) * 1e30
        W[5, K - 1] = 1e-20
        W[6] = torch.randn(K, generator=gen) * 1e-30
    return W


@pytest.mark.parametrize("N", [16, 20, 300, 320])
def test_split_bytes_one_matrix(gpu_device, N):
    """``dmpnn_linear16_fwd`` with ``M = 0``: the weight split alone (``k_split_weights``), one matrix [N, K]."""
    from chemprop_amd import _lib
    from chemprop_amd.engine import _stream_ptr

    lib = _lib.load()
    gen = torch.Generator().manual_seed(100 + N)
    wrong = []
    for K in (1, 31, 32, 33, 86, 300, 372):
        for ld_extra in (0, 3):                                   # (rows that start off a 16-byte boundary too)
            W = _special_rows(torch.randn(N, K, generator=gen) * 0.3, gen)
            buf = torch.full((N, K + ld_extra), float("nan"))
            buf[:, :K] = W
            Wd = buf.to(gpu_device)
            nb = int(lib.dmpnn_linear16_wsplit_bytes(N, K))
            ws = torch.full((nb + 256,), 0xA5, dtype=torch.uint8, device=gpu_device)
            g = _lib.GemmArgs()
            g.M, g.N, g.K1, g.K2 = 0, N, K, 0
            g.W, g.ldw = Wd.data_ptr(), K + ld_extra
            with torch.cuda.device(gpu_device):
                _lib.check(lib.dmpnn_linear16_fwd(C.byref(g), ws.data_ptr(), nb, 0, _stream_ptr(gpu_device)), "dmpnn_linear16_fwd")
            got = ws.cpu().numpy()
            nc, NT = (K + 31) // 32, (N + 15) // 16
            ref, inv = split_ref(W.numpy(), nc)
            assert ref.size == NT * nc * 2048
            o = _al256(ref.size)
            if not np.array_equal(got[:ref.size], ref):
                at = int(np.flatnonzero(got[:ref.size] != ref)[0])
                wrong.append((K, ld_extra, "split byte", at, int(got[at]), int(ref[at])))
            if not np.array_equal(got[o:o + 4 * N], inv.view(np.uint8)):
                wrong.append((K, ld_extra, "inv_scale row", int(np.flatnonzero(got[o:o + 4 * N] != inv.view(np.uint8))[0]) // 4))
            assert (got[nb:] == 0xA5).all()
    assert not wrong, wrong


def test_split_bytes_of_a_training_forward(gpu_device):
    """The six jobs of the tile kernel's training forward: W_i, W_h, W_o[:, d_v:] and W_o[:, :d_v] (both under the scale of the WHOLE
    W_o row), and the backward's two transposed matrices W_o[:, d_v:]^T and W_h^T."""
    from chemprop_amd import engine, synth

    d_v, d_e, N = 72, 14, 300
    gen = torch.Generator().manual_seed(3)
    W_i = _special_rows(torch.randn(N, d_v + d_e, generator=gen) * 0.2, gen)
    W_h = _special_rows(torch.randn(N, N, generator=gen) * 0.1, gen)
    W_o = torch.randn(N, d_v + N, generator=gen) * 0.1
    W_o[7, :d_v] *= 64.0          # the row maximum in the OTHER column block
    W_o[8, d_v:] *= 64.0
    W_o[9] = 0.0
    b_o = torch.randn(N, generator=gen)
    bmg = synth.random_batch(8, "qm9", seed=1)
    bmg.to(gpu_device)
    plan = engine.GraphPlan.from_bmg(bmg)
    dev = gpu_device
    _, st = engine.forward(plan, bmg.V, bmg.E, W_i.to(dev), W_h.to(dev), W_o.to(dev), b_o.to(dev), keep=True)
    assert st.route == "mega16", st.route
    got = st.refs[-1].cpu().numpy()
    NT, nc_i, nc_h, nc_v = (N + 15) // 16, (d_v + d_e + 31) // 32, (N + 31) // 32, (d_v + 31) // 32
    o = 0
    off = {}
    for name, nbytes in (("wi", NT * nc_i * 2048), ("wh", NT * nc_h * 2048), ("wom", NT * nc_h * 2048), ("wov", NT * nc_v * 2048),
                         ("sc_i", N * 4), ("sc_h", N * 4), ("sc_o", N * 4)):
        off[name] = o
        o += _al256(nbytes)
    one = _al256(NT * nc_h * 2048) + _al256(N * 4)
    Wi, Wh, Wo = W_i.numpy(), W_h.numpy(), W_o.numpy()
    jobs = [("wi", "sc_i", Wi, nc_i, None), ("wh", "sc_h", Wh, nc_h, None), ("wom", "sc_o", Wo[:, d_v:], nc_h, Wo),
            ("wov", None, Wo[:, :d_v], nc_v, Wo)]
    for name, sc, W, nc, over in jobs:
        ref, inv = split_ref(np.ascontiguousarray(W), nc, over)
        assert np.array_equal(got[off[name]:off[name] + ref.size], ref), name
        if sc:
            assert np.array_equal(got[off[sc]:off[sc] + 4 * N], inv.view(np.uint8)), sc
    for j, Wt in enumerate((np.ascontiguousarray(Wo[:, d_v:].T), np.ascontiguousarray(Wh.T))):   # W'[n][k] = W[k][n]
        ref, inv = split_ref(Wt, nc_h)
        base = o + j * one
        assert np.array_equal(got[base:base + ref.size], ref), ("transposed", j)
        so = base + _al256(NT * nc_h * 2048)
        assert np.array_equal(got[so:so + 4 * N], inv.view(np.uint8)), ("transposed scale", j)


# ---- own batch == the same tensors through the device planner ---------------------------------------------------------------------
D_V, D_E = 72, 14


def _mols(sizes, seed):
    """Molecules of the given (atoms, directed edges) sizes: random bonds inside each, random features."""
    from chemprop_amd.data import MolGraph

    rng = np.random.default_rng(seed)
    out = []
    for na, ne in sizes:
        src, dst = [], []
        for _ in range(ne // 2):
            u = int(rng.integers(na))
            v = (u + 1 + int(rng.integers(na - 1))) % na
            src += [u, v]
            dst += [v, u]
        n = len(src)
        out.append(MolGraph(rng.standard_normal((na, D_V)).astype(np.float32), rng.standard_normal((n, D_E)).astype(np.float32),
                            np.array([src, dst], dtype=np.int64).reshape(2, n), np.arange(n, dtype=np.int64) ^ 1))
    return out


def _qm9_sizes(n, seed):
    from chemprop_amd import synth

    return [(len(m.V), int(m.edge_index.shape[1])) for m in synth.random_molgraphs(n, "qm9", seed=seed)]


def _put(sizes, at):
    s = list(sizes)
    for i, v in at.items():
        s[i] = v
    return s


SHAPES = {
    "one_molecule": lambda: [(9, 20)],
    "qm9_65": lambda: _qm9_sizes(65, 65),
    "single_atoms": lambda: _put(_qm9_sizes(80, 3), {**{i: (1, 0) for i in range(6)}, **{i: (1, 0) for i in range(58, 71)}, 79: (1, 0)}),
    "limit_48_32": lambda: _put(_qm9_sizes(70, 4), {0: (32, 48), 40: (32, 48), 63: (32, 48), 64: (32, 48)}),
}
MODELS = {"h128_relu": (128, "relu", False), "h300_relu": (300, "relu", False), "h128_tanh_bias": (128, "tanh", True),
          "h300_tanh_bias": (300, "tanh", True)}


def _pair(sizes, seed, dev):
    from chemprop_amd.data import BatchMolGraph

    own = BatchMolGraph(_mols(sizes, seed))
    own.to(dev)
    assert own.plan_table is not None and own.plan_table[0].device.type == "cuda"
    bare = BatchMolGraph.from_tensors(own.V, own.E, own.edge_index, own.rev_edge_index, own.batch, len(own))
    assert bare.plan_table is None
    return own, bare


def _module(model, dev):
    from chemprop_amd.nn import BondMessagePassing

    d_h, act, bias = MODELS[model]
    torch.manual_seed(17)
    return BondMessagePassing(d_v=D_V, d_e=D_E, d_h=d_h, bias=bias, activation=act).eval().to(dev)


def _both_paths(mp, bmg):
    """(slow-path forward, steady-path forward) of a module that has seen nothing yet."""
    mp = copy.deepcopy(mp)
    with torch.no_grad():
        a = mp(bmg)
        assert mp.__dict__.get("_dmpnn_route") == "mega16", mp.__dict__.get("_dmpnn_route")
        assert mp.__dict__.get("_dmpnn_replay") is not None
        b = mp(bmg)
    return a, b


def _same(a, b):
    return torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(torch.nan_to_num(a), torch.nan_to_num(b))


@pytest.mark.parametrize("model", list(MODELS))
@pytest.mark.parametrize("shape", list(SHAPES))
def test_own_batch_equals_device_planner(gpu_device, monkeypatch, shape, model):
    monkeypatch.setenv("DMPNN_VALIDATE", "never")   # (the first batches of a module are validated on full plans otherwise)
    own, bare = _pair(SHAPES[shape](), 5, gpu_device)
    mp = _module(model, gpu_device)
    ref_slow, ref_steady = _both_paths(mp, bare)
    got_slow, got_steady = _both_paths(mp, own)
    assert bool(torch.isfinite(ref_slow).all()) and float(ref_slow.abs().max()) > 0
    assert torch.equal(ref_slow, ref_steady)
    assert torch.equal(got_slow, ref_slow), "slow path: host table vs device planner"
    assert torch.equal(got_steady, ref_slow), "steady path: host table vs device planner"


def test_the_table_is_what_k0_reads(gpu_device, monkeypatch):
    """A table that is out of order (written over in place: the batch still carries it) makes every output NaN on both paths — the
    forward of an own batch does take its tiles from the table."""
    monkeypatch.setenv("DMPNN_VALIDATE", "never")
    own, _ = _pair(SHAPES["qm9_65"](), 5, gpu_device)
    assert own.plan_table[2] > 3
    own.plan_table[1][2] = own.plan_table[1][1] - 1
    for out in _both_paths(_module("h128_relu", gpu_device), own):
        assert bool(torch.isnan(out).all())


def _corrupt(kind, bmg):
    """One defect, written INTO the batch's tensors (nothing is rebound: an own batch keeps its table)."""
    b, ei = bmg.batch, bmg.edge_index
    nV, nE = b.numel(), ei.shape[1]
    if kind == "unsorted":              # [.., 3, 3, 2, 2, 5, ..]: every id in range
        b[b == 4] = 2
    elif kind == "last_below":          # the last molecule's id below earlier ones
        b[b == int(b[-1])] = 1
    elif kind == "id_beyond":
        b[nV // 2] = nV + 5
    elif kind == "id_negative":
        b[nV // 2] = -1
    elif kind == "dst_beyond":
        ei[1, nE // 2] = nV + 3
    elif kind == "edge_leaves_tile_dst":   # a destination in a molecule far away: batch[dst] is no longer sorted
        ei[1, 3] = nV - 1
    elif kind == "edge_leaves_tile_src":   # a source far away: the tile of that edge is not closed
        ei[0, 3] = nV - 1
    else:
        raise KeyError(kind)


ALL_NAN = ["unsorted", "last_below", "id_beyond", "id_negative", "dst_beyond", "edge_leaves_tile_dst"]


@pytest.mark.parametrize("kind", ALL_NAN + ["edge_leaves_tile_src"])
def test_corrupted_batches(gpu_device, monkeypatch, kind):
    monkeypatch.setenv("DMPNN_VALIDATE", "never")
    own, bare = _pair(SHAPES["qm9_65"](), 9, gpu_device)
    mp = _module("h128_relu", gpu_device)
    with torch.no_grad():
        good = copy.deepcopy(mp)(own)
    assert bool(torch.isfinite(good).all())
    _corrupt(kind, own)                  # (bare shares the tensors)
    assert own.plan_table is not None
    ref_slow, ref_steady = _both_paths(mp, bare)
    got_slow, got_steady = _both_paths(mp, own)
    if kind in ALL_NAN:
        assert bool(torch.isnan(ref_slow).all()) and bool(torch.isnan(ref_steady).all())
        assert bool(torch.isnan(got_slow).all()) and bool(torch.isnan(got_steady).all())
    else:   # the tile that is not closed is NaN, the others are what they were
        nan_rows = torch.isnan(ref_slow).any(dim=1)
        assert bool(nan_rows.any()) and not bool(nan_rows.all())
        assert torch.equal(ref_slow[~nan_rows], good[~nan_rows])
    assert _same(ref_slow, ref_steady) and _same(got_slow, ref_slow) and _same(got_steady, ref_slow)


def test_tile_start_inside_a_molecule_of_the_batch_vector(gpu_device, monkeypatch):
    """The batch vector rewritten in place so that it stays sorted and in range, but a tile of the table now starts inside one of its
    molecules: the table no longer describes the batch — NaN, not the forward of the tiles as they were."""
    monkeypatch.setenv("DMPNN_VALIDATE", "never")
    own, _ = _pair(SHAPES["qm9_65"](), 9, gpu_device)
    a = int(own.plan_table[1][2])
    own.batch[a] = own.batch[a - 1]
    assert own.plan_table is not None
    for out in _both_paths(_module("h128_relu", gpu_device), own):
        assert bool(torch.isnan(out).all())
