"""The tile plan made on the HOST where the batch is made (``dmpnn_pack_tiles_blocked``, ``data.BatchMolGraph.plan_table``).

The packer is integer work and must be the device planners' packing bit for bit: it is held against the one statement the planner
kernels are held against (``oracle.collate_numpy.blocked_molecule_tiles``, ``tests/test_k0_planners.py``).  A batch built by
``BatchMolGraph(mgs)`` carries the table (in the tail of the buffer its batch vector lives in); bare tensors, oversize batches and
batches whose tensors were rebound do not.  No GPU needed.
"""
from __future__ import annotations

import copy
import pickle

import numpy as np
import pytest
import torch

from oracle.collate_numpy import batch_tile_plan, blocked_molecule_tiles


def _pack(n_atoms, n_edges, cap=None):
    from chemprop_amd import _lib

    lib = _lib.load()
    n = len(n_atoms)
    ao, eo = np.zeros(n + 1, dtype=np.int32), np.zeros(n + 1, dtype=np.int32)
    ao[1:], eo[1:] = np.cumsum(n_atoms), np.cumsum(n_edges)
    if cap is None:
        cap = int(lib.dmpnn_max_tiles(int(ao[-1]), int(eo[-1]))) + 1
    tr, ta = np.full(cap, -7, dtype=np.int32), np.full(cap, -7, dtype=np.int32)
    nt = int(lib.dmpnn_pack_tiles_blocked(ao.ctypes.data, eo.ctypes.data, n, tr.ctypes.data, ta.ctypes.data, cap))
    return nt, tr, ta


def _qm9(n, seed):
    from chemprop_amd import synth

    ms = synth.random_molgraphs(n, "qm9", seed=seed)
    return [len(m.V) for m in ms], [int(m.edge_index.shape[1]) for m in ms]


def _case(name):
    if name.startswith("qm9_"):
        return _qm9(int(name[4:]), int(name[4:]))
    na, ne = _qm9(140, 7)
    if name == "limit_48_32":        # exactly a tile: packed like any other molecule (alone: nothing else fits beside it)
        na[3], ne[3] = 32, 48
        na[64], ne[64] = 32, 48
    elif name == "over_49_33":       # one beyond: a tile of its own (the tile kernel's generic path), wherever it stands
        na[0], ne[0] = 33, 49
        na[63], ne[63] = 33, 48
        na[64], ne[64] = 32, 49
        na[139], ne[139] = 40, 60
    elif name == "no_atoms":         # ids without atoms: in front, around a block boundary, in a run, at the end
        for i in (0, 1, 63, 64, 65, 100, 101, 102, 139):
            na[i], ne[i] = 0, 0
    elif name == "single_atoms":     # 32 lone atoms fill a tile; runs across the block boundary
        for i in list(range(0, 40)) + list(range(58, 71)) + list(range(120, 140)):
            na[i], ne[i] = 1, 0
    elif name == "only_single_atoms":
        na, ne = [1] * 300, [0] * 300
    else:
        raise KeyError(name)
    return na, ne


CASES = ["qm9_1", "qm9_63", "qm9_64", "qm9_65", "qm9_128", "qm9_129", "qm9_512", "limit_48_32", "over_49_33", "no_atoms", "single_atoms",
         "only_single_atoms"]


@pytest.mark.parametrize("name", CASES)
def test_packer_is_the_device_planners_packing(name):
    na, ne = _case(name)
    tr, ta = blocked_molecule_tiles(na, ne)
    nt, got_r, got_a = _pack(na, ne)
    assert nt == len(tr) - 1
    assert np.array_equal(got_r[:nt + 1], tr) and np.array_equal(got_a[:nt + 1], ta)
    assert (got_r[nt + 1:] == -7).all() and (got_a[nt + 1:] == -7).all(), "wrote behind n_tiles + 1 entries"


def test_packer_random_counts():
    rng = np.random.default_rng(11)
    for _ in range(200):
        n = int(rng.integers(1, 400))
        kind = int(rng.integers(4))
        if kind == 0:      # molecule-like
            na = rng.integers(1, 14, size=n)
            ne = 2 * rng.integers(0, 14, size=n)
        elif kind == 1:    # anything up to well beyond the tile, empty ids included
            na = rng.integers(0, 40, size=n)
            ne = rng.integers(0, 60, size=n)
        elif kind == 2:    # tiny: many molecules per tile, the block boundary decides
            na = rng.integers(0, 3, size=n)
            ne = rng.integers(0, 3, size=n)
        else:              # around the limits
            na = rng.choice([1, 16, 31, 32, 33], size=n)
            ne = rng.choice([0, 24, 47, 48, 49], size=n)
        tr, ta = blocked_molecule_tiles(na, ne)
        nt, got_r, got_a = _pack(na, ne)
        assert nt == len(tr) - 1, (kind, n)
        assert np.array_equal(got_r[:nt + 1], tr) and np.array_equal(got_a[:nt + 1], ta), (kind, n)


def test_packer_bad_arguments():
    na, ne = _qm9(65, 3)
    tr, _ = blocked_molecule_tiles(na, ne)
    n_tiles = len(tr) - 1
    assert _pack(na, ne, cap=n_tiles + 1)[0] == n_tiles          # n_tiles + 1 entries: exactly enough
    assert _pack(na, ne, cap=n_tiles)[0] == -2                   # one short: refused like dmpnn_pack_tiles
    assert _pack(na, ne, cap=1)[0] == -2
    nt, tr0, ta0 = _pack([], [])
    assert nt == 0 and tr0[0] == 0 and ta0[0] == 0
    from chemprop_amd import _lib

    lib = _lib.load()
    one = np.zeros(2, dtype=np.int32)
    assert lib.dmpnn_pack_tiles_blocked(one.ctypes.data, one.ctypes.data, 1, None, one.ctypes.data, 2) == -2
    assert lib.dmpnn_pack_tiles_blocked(None, one.ctypes.data, 1, one.ctypes.data, one.ctypes.data, 2) == -2
    assert lib.dmpnn_pack_tiles_blocked(one.ctypes.data, one.ctypes.data, -1, one.ctypes.data, one.ctypes.data, 2) == -2


# ---- the batch carries it --------------------------------------------------------------------------------------------------------
def _table(bmg):
    tr, ta, nt = bmg.plan_table
    assert tr.dtype == torch.int32 and ta.dtype == torch.int32 and tr.numel() == nt + 1 and ta.numel() == nt + 1
    return tr.numpy(), ta.numpy(), nt


def _expect(bmg):
    ref = batch_tile_plan(bmg.batch.numpy(), bmg.edge_index[1].numpy())
    assert ref["valid"]
    return ref["mtile_row"], ref["mtile_atom"], ref["n_tiles"]


def test_own_batch_carries_the_planners_table():
    from chemprop_amd import synth
    from chemprop_amd.data import BatchMolGraph

    mgs = synth.random_molgraphs(65, "qm9", seed=5)
    bmg = BatchMolGraph(mgs)
    er, ea, en = _expect(bmg)
    tr, ta, nt = _table(bmg)
    assert nt == en and np.array_equal(tr, er) and np.array_equal(ta, ea)
    # the batch vector is what it always was: int64, contiguous, one id per atom
    ref = np.repeat(np.arange(65), [len(m.V) for m in mgs])
    assert bmg.batch.dtype == torch.int64 and bmg.batch.is_contiguous() and np.array_equal(bmg.batch.numpy(), ref)
    # ... and the table rides in the buffer behind it: moving the batch moves it (still five tensors to copy)
    assert tr.ctypes.data == bmg.batch.data_ptr() + 8 * bmg.batch.numel()
    bmg.to("cpu")
    tr, ta, nt = _table(bmg)
    assert nt == en and np.array_equal(tr, er) and np.array_equal(ta, ea)
    assert tr.ctypes.data == bmg.batch.data_ptr() + 8 * bmg.batch.numel()
    c = copy.copy(bmg)
    assert c.plan_table is bmg.plan_table and c.batch is bmg.batch
    p = pickle.loads(pickle.dumps(bmg))
    tr, ta, nt = _table(p)
    assert nt == en and np.array_equal(tr, er) and np.array_equal(ta, ea) and torch.equal(p.batch, bmg.batch)


def test_batches_without_a_table():
    from chemprop_amd import synth
    from chemprop_amd.data import BatchMolGraph

    mgs = synth.random_molgraphs(20, "qm9", seed=6)
    own = BatchMolGraph(mgs)
    assert own.plan_table is not None and own.oversize is False
    bare = BatchMolGraph.from_tensors(own.V, own.E, own.edge_index, own.rev_edge_index, own.batch, len(own))
    assert bare.plan_table is None
    # a molecule beyond the tile: the per-step routes, no table
    big = BatchMolGraph(mgs + [synth.random_molgraph(np.random.default_rng(0), n_atoms=40)])
    assert big.oversize is True and big.plan_table is None
    # rebinding any of the five tensors: the table described the tensors it was made with
    for name in ("V", "E", "edge_index", "rev_edge_index", "batch"):
        b = BatchMolGraph(mgs)
        setattr(b, name, getattr(b, name).clone())
        assert b.plan_table is None, name
    # ... other attributes do not
    b = BatchMolGraph(mgs)
    b.tiles = None
    assert b.plan_table is not None
    # beyond what the single-workgroup planner covers: K0 stays on the device (its multi-launch planner)
    many = BatchMolGraph(synth.random_molgraphs(700, "qm9", seed=7))
    assert int(many.E.shape[0]) > 10240 and many.plan_table is None and many.oversize is False


def test_trailing_ids_without_atoms_are_not_planned():
    """What the planners that read ``batch[-1]`` do: molecules behind the last atom do not exist for them."""
    from chemprop_amd import synth
    from chemprop_amd.data import BatchMolGraph, MolGraph

    mgs = synth.random_molgraphs(10, "qm9", seed=8)
    d_v, d_e = mgs[0].V.shape[1], mgs[0].E.shape[1]
    empty = MolGraph(np.zeros((0, d_v), np.float32), np.zeros((0, d_e), np.float32), np.zeros((2, 0), np.int64), np.zeros(0, np.int64))
    bmg = BatchMolGraph(mgs[:5] + [empty] + mgs[5:] + [empty, empty])
    er, ea, en = _expect(bmg)
    tr, ta, nt = _table(bmg)
    assert nt == en and np.array_equal(tr, er) and np.array_equal(ta, ea)
