"""What a module-path forward of every message-passing block does, as one JSON document: ``python scripts/dump_block_routes.py TREE OUT.json``
(on the MI355X; ``main`` puts ``TREE`` in front of ``sys.path`` first).

Every case is a fresh module under ``torch.manual_seed(0)`` and FOUR consecutive forwards of one batch — the two validated first
batches, the first batch on a tile plan, a steady batch.  Per call: ``_dmpnn_route``, the ``[light, tiles_only]`` of every plan the
call built through ``GraphPlan.from_bmg``, whether the call was a replayed forward and whether a replay state exists behind it, a
SHA-256 of the raw bytes of every output and — training cases, after ``out.sum().backward()`` — of every parameter's gradient and of
``V.grad`` / ``E.grad`` / ``V_d.grad`` where the case asks for them.  A call that raises records the exception's class and message.
The compute kernels use no atomics, so the hashes reproduce: ``main`` runs every case twice and refuses to write a table whose two
runs differ.  ``tests/golden/block_routes_parent.json`` is this script's output on the commit before the module-path forwards were
consolidated; ``tests/test_block_routes_gpu.py`` holds the working tree to it, string by string.
"""
import hashlib
import json
import sys

import numpy as np
import torch
from torch import nn

D_H, D_VD, D_ED = 32, 4, 3

BLOCKS = {   # name -> (module, class, constructor arguments)
    "bond": ("nn", "BondMessagePassing", {}),
    "atom": ("nn", "AtomMessagePassing", {}),
    "mabbond/v": ("mab", "MABBondMessagePassing", dict(return_edge_embeddings=False)),
    "mabbond/e": ("mab", "MABBondMessagePassing", dict(return_vertex_embeddings=False)),
    "mabbond/ve": ("mab", "MABBondMessagePassing", {}),
    "mabatom/v": ("mab", "MABAtomMessagePassing", dict(return_edge_embeddings=False)),
    "mabatom/e": ("mab", "MABAtomMessagePassing", dict(return_vertex_embeddings=False)),
    "mabatom/ve": ("mab", "MABAtomMessagePassing", {}),
}
FOUR = ("bond", "atom", "mabbond/ve", "mabatom/ve")
MODES = ("eval", "train", "train_frozen_ih", "input_grad")
FEATURES = {   # name -> constructor arguments (descriptors are made for d_vd / d_ed)
    "base": {}, "vd": dict(d_vd=D_VD), "ed": dict(d_ed=D_ED), "undirected": dict(undirected=True), "dropout": dict(dropout=0.25),
    "custom": dict(activation="softplus"), "prelu": dict(activation="prelu"), "depth1": dict(depth=1), "bias": dict(bias=True),
}
REFUSALS = ("vd_wrong_width", "vd_without_d_vd", "cpu_batch")


def cases() -> list:
    """``(block, mode, feature, batch, d_e)`` of every case, in the order they run."""
    out = [(b, m, "base", "own", 14) for b in BLOCKS for m in MODES]
    for f in FEATURES:
        if f == "base":
            continue
        for b in FOUR:
            if f == "ed" and not b.startswith("mab"):
                continue
            out += [(b, m, f, "own", 14) for m in (("train",) if f == "dropout" else ("eval", "train"))]
    out += [(b, "input_grad", "vd", "own", 14) for b in FOUR]
    out += [(b, m, "base", bt, 14) for bt in ("bare", "packed", "own+chain", "bare+chain") for b in FOUR for m in ("eval", "train")]
    out += [("bond", "train", "dropout", bt, 14) for bt in ("bare", "bare+chain", "own+chain")]   # (oversize counted on the device)
    out += [("bond", m, "base", "noedges", 14) for m in ("eval", "train")]
    # the row chain on a batch without edges: the bond chain's W_h contraction on no rows, the step the other two skip
    out += [("bond", "train", "custom", "noedges", 14), ("atom", "train", "base", "noedges", 14), ("mabatom/ve", "train", "base", "noedges", 14)]
    out += [(b, m, "base", "own", 13) for b in ("atom", "mabatom/ve") for m in ("eval", "train")]   # odd d_e: the rows chain under grad
    out += [(b, "eval", r, "own", 14) for r in REFUSALS for b in ("bond", "atom", "mabbond/ve")]
    return out


def case_name(c) -> str:
    return "|".join(str(x) for x in c)


def _mols(batch: str, d_e: int):
    from chemprop_amd import synth

    if batch == "noedges":
        rng = np.random.default_rng(0)
        return [synth.random_molgraph(rng, d_v=72, d_e=d_e, n_atoms=1) for _ in range(4)]
    mols = synth.random_molgraphs(8, "qm9", seed=0, d_e=d_e)
    return mols + [synth.chain_molgraph(40, d_e=d_e)] if batch.endswith("+chain") else mols


def _batch(batch: str, d_e: int, dev):
    from chemprop_amd.data import BatchMolGraph, PackedBatch

    mols = _mols(batch, d_e)
    if batch == "packed":
        return PackedBatch(mols).to_device(dev)
    b = BatchMolGraph(mols)
    if batch.startswith("bare"):   # the same tensors without the batching code's knowledge (oversize unknown, no table)
        b = BatchMolGraph.from_tensors(b.V, b.E, b.edge_index, b.rev_edge_index, b.batch, len(mols))
    if dev is not None:
        b.to(dev)
    return b


def _module(block: str, feature: str, d_e: int):
    import importlib

    mod, cls, kw = BLOCKS[block]
    kw = dict(kw, d_h=D_H, d_v=72, d_e=d_e)
    if feature == "vd_wrong_width":
        kw.update(d_vd=D_VD)
    kw.update(FEATURES.get(feature, {}))
    if kw.get("activation") == "softplus":
        kw["activation"] = nn.Softplus()   # a module the kernels have no code for
    return getattr(importlib.import_module("chemprop_amd." + mod), cls)(**kw)


def _sha(t) -> str:
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def run_case(c, dev) -> list:
    from chemprop_amd import engine

    block, mode, feature, batch, d_e = c
    torch.manual_seed(0)
    m = _module(block, feature, d_e).to(dev)
    m.train(mode in ("train", "train_frozen_ih"))
    if mode == "train_frozen_ih":
        for p in list(m.W_i.parameters()) + list(m.W_h.parameters()):
            p.requires_grad_(False)
    if mode == "input_grad":
        for p in m.parameters():
            p.requires_grad_(False)
    bmg = _batch(batch, d_e, None if feature == "cpu_batch" else dev)
    gen = torch.Generator().manual_seed(1)
    extra = {}
    if feature == "vd" or feature == "vd_without_d_vd":
        extra["V_d"] = torch.randn(bmg.V.shape[0], D_VD, generator=gen).to(dev)
    if feature == "vd_wrong_width":
        extra["V_d"] = torch.randn(bmg.V.shape[0], D_VD + 1, generator=gen).to(dev)
    if feature == "ed":
        extra["E_d"] = torch.randn(bmg.E.shape[0], D_ED, generator=gen).to(dev)
    leaves = {}
    if mode == "input_grad":
        leaves = {"V": bmg.V, "E": bmg.E, **{k: v for k, v in extra.items() if k == "V_d"}}
        for t in leaves.values():
            t.requires_grad_(True)
    plans = []
    from_bmg = engine.GraphPlan.from_bmg

    def recording(*a, **k):
        plan = from_bmg(*a, **k)
        plans.append([bool(plan.light), bool(plan.tiles_only)])
        return plan

    calls = []
    engine.GraphPlan.from_bmg = staticmethod(recording)
    try:
        for _ in range(4):
            del plans[:]
            for p in list(m.parameters()) + list(leaves.values()):
                p.grad = None
            had_replay = m.__dict__.get("_dmpnn_replay") is not None
            rec = {}
            try:
                with torch.set_grad_enabled(mode != "eval"):
                    out = m(bmg, **extra)
                outs = [o for o in (out if isinstance(out, tuple) else (out,))]
                rec["out"] = [None if o is None else _sha(o) for o in outs]
                if mode != "eval":
                    sum(o.sum() for o in outs if o is not None).backward()
                    rec["grad"] = {k: (None if p.grad is None else _sha(p.grad)) for k, p in list(m.named_parameters()) + list(leaves.items())}
            except Exception as e:   # (a refusal is part of the record)
                rec = {"raises": type(e).__name__, "message": str(e)}
            rec["route"] = m.__dict__.get("_dmpnn_route")
            rec["plans"] = [list(p) for p in plans]
            rec["replayed"] = had_replay and not plans and "raises" not in rec
            rec["replay_state"] = m.__dict__.get("_dmpnn_replay") is not None
            calls.append(rec)
        torch.cuda.synchronize()
    finally:
        engine.GraphPlan.from_bmg = from_bmg
    return calls


def required_routes(table: dict) -> list:
    """The routes a table must hold at least once (else it checks nothing): the names that are missing."""
    calls = [r for rec in table.values() for r in rec]
    routes = {str(r["route"]) for r in calls}
    missing = [r for r in ("mega16", "mega16/atom", "rows", "rows/atom") if r not in routes]
    if not any(r.startswith(("fused16", "general")) for r in routes):
        missing.append("fused16* | general*")
    if not any(r["replayed"] for r in calls):
        missing.append("a replayed forward")
    return missing


def records(dev=None) -> dict:
    dev = torch.device("cuda:0") if dev is None else dev
    return {case_name(c): run_case(c, dev) for c in cases()}


def main(tree: str, out: str) -> None:
    sys.path[:0] = [tree]
    first, second = records(), records()
    unstable = [k for k in first if first[k] != second[k]]
    if unstable:
        raise SystemExit(f"not reproducible, nothing written: {unstable}")
    missing = required_routes(first)
    if missing:
        raise SystemExit(f"the cases never reach: {missing} (routes seen: {sorted({str(r['route']) for rec in first.values() for r in rec})})")
    with open(out, "w") as f:
        json.dump(first, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"{len(first)} cases -> {out}")


if __name__ == "__main__":
    main(*sys.argv[1:3])
