"""One training step of a regression model with ATOM MESSAGES (`chemprop train --atom-messages`: AtomMessagePassing, d_h 300, depth 3,
norm aggregation, batch norm, one hidden layer of 300, MSE, ReLU), with and without dropout in the block:

  fused         FusedTrainer(atom_messages=True, rows_dropout=True).step: K0, the block, the head, backward, Adam — one call.  p = 0 at
                QM9 size: the tile kernels with DMPNN_F_ATOM; everything else: the per-step general route on the f16 pipe
  module path   MPNN.loss(...).backward() + FlatAdam.step: what such a model trained on before — one autograd node on the tile
                kernels (p = 0, QM9 size), else the chain of row kernels with torch's tau and nn.Dropout between them

at 512 QM9-shaped and at 512 ZINC-shaped molecules, p = 0 and p = 0.2.  Per shape the configurations are warmed, then timed
ALTERNATELY in one process: `groups` rounds, in each round K steps of every configuration between two device synchronisations; per
configuration the per-step time of every round and their median.
`--bond-only` times the default BOND model's p = 0 step on both shapes instead (no keyword of this change is used; with `--root DIR`
the package is imported from another checkout, which is how that step is compared with the parent commit in the same visit).
`--combine parent_first.json atom.json this_bond.json parent_second.json` writes the four processes' results of one visit, with the
two comparisons drawn from them, to `--out` (profiles/atom_step.json).
usage: python scripts/time_atom_step.py [--steps K] [--warmup W] [--groups G] [--bond-only] [--root DIR] [--out file.json]"""
import argparse
import json
import os
import sys
import time

import torch

SHAPES = ((512, "qm9"), (512, "zinc"))
P = 0.2


def run(step, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e6


def combine(paths, out_path):
    d = dict(zip(("parent_first", "atom", "this_bond", "parent_second"), (json.load(open(p)) for p in paths)))
    a = d["atom"]
    out = dict(script="scripts/time_atom_step.py", steps=a["steps"], warmup=a["warmup"], groups=a["groups"], device=a["device"],
               order="one GPU call, process by process: parent --bond-only, this tree (the eight atom configurations), this tree --bond-only, "
                     "parent --bond-only",
               results=a["results"], this_tree_bond_only=d["this_bond"]["results"], parent_bond_only_first=d["parent_first"]["results"],
               parent_bond_only_second=d["parent_second"]["results"])
    r, sp = a["results"], {}
    for n, kind in SHAPES:
        for p in ("0", f"{P:g}"):
            f, m = r[f"fused, p {p}, {n} {kind} mols"], r[f"module path, p {p}, {n} {kind} mols"]
            sp[f"p {p}, {n} {kind} mols"] = dict(fused_us=f["us_per_step"], module_us=m["us_per_step"], speedup=round(m["us_per_step"] / f["us_per_step"], 2),
                                                module_spread_us=round(max(m["groups_us"]) - min(m["groups_us"]), 1))
    out["fused_against_module_path"] = sp
    bond = {}
    for k, t in d["this_bond"]["results"].items():
        pg = d["parent_first"]["results"][k]["groups_us"] + d["parent_second"]["results"][k]["groups_us"]
        bond[k] = dict(this_tree_us=t["us_per_step"], parent_us=[d["parent_first"]["results"][k]["us_per_step"], d["parent_second"]["results"][k]["us_per_step"]],
                       parent_groups_min_max_us=[min(pg), max(pg)], within_parent_spread=bool(min(pg) <= t["us_per_step"] <= max(pg)))
    out["bond_step_against_parent"] = bond
    with open(out_path, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(dict(fused_against_module_path=sp, bond_step_against_parent=bond)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--groups", type=int, default=5)
    ap.add_argument("--bond-only", action="store_true")
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--out", default=None)
    ap.add_argument("--combine", nargs=4, default=None, metavar="JSON")
    args = ap.parse_args()
    if args.combine:
        return combine(args.combine, args.out or os.path.join(args.root, "profiles", "atom_step.json"))
    sys.path.insert(0, os.path.abspath(args.root))
    from chemprop_amd import agg as cagg
    from chemprop_amd import distributed as ddp
    from chemprop_amd import synth
    from chemprop_amd.model import MPNN, FusedTrainer, RegressionFFN
    from chemprop_amd.nn import AtomMessagePassing, BondMessagePassing
    from chemprop_amd.optim import FlatAdam

    dev = torch.device("cuda:0")

    def model(cls, p):
        torch.manual_seed(0)
        mp = cls(dropout=p)
        return MPNN(mp, cagg.NormAggregation(), RegressionFFN(n_tasks=1, input_dim=mp.output_dim), batch_norm=True).to(dev).train()

    res = {}
    for n, kind in SHAPES:
        bmg = synth.random_batch(n, kind, seed=1)
        bmg.to(dev)
        y = torch.randn(n, 1, generator=torch.Generator().manual_seed(2)).to(dev)
        configs, routes, syncs = {}, {}, []
        if args.bond_only:
            t0 = FusedTrainer(model(BondMessagePassing, 0.0), lr=1e-5)
            configs["bond model, fused, p 0"] = lambda t0=t0: t0.step(bmg, y)
            routes["bond model, fused, p 0"] = lambda t0=t0: str(t0.last_route)
        else:
            for p in (0.0, P):
                tr = FusedTrainer(model(AtomMessagePassing, p), lr=1e-5, rows_dropout=True, atom_messages=True)
                m = model(AtomMessagePassing, p)
                sync = ddp.GradSync(list(m.parameters()), modules=[m])
                opt = FlatAdam(sync, lr=1e-5)
                syncs.append(sync)

                def module_step(m=m, sync=sync, opt=opt):   # (what integration.HipMPNN.training_step runs where the fused step refuses)
                    with ddp.backward_on_calling_thread():
                        sync.zero_grad()
                        m.loss(bmg, y).backward()
                    sync.allreduce()
                    opt.step()

                configs[f"fused, p {p:g}"] = lambda tr=tr: tr.step(bmg, y)
                configs[f"module path, p {p:g}"] = module_step
                routes[f"fused, p {p:g}"] = lambda tr=tr: str(tr.last_route)
                routes[f"module path, p {p:g}"] = lambda m=m: "module:" + str(m.message_passing.__dict__.get("_dmpnn_route"))
        for step in configs.values():
            run(step, args.warmup)
        per = {k: [] for k in configs}
        for _ in range(args.groups):
            for k, step in configs.items():
                per[k].append(run(step, args.steps))
        for s in syncs:
            s.wait()
        for k, v in per.items():
            res[f"{k}, {n} {kind} mols"] = dict(us_per_step=round(sorted(v)[len(v) // 2], 1), groups_us=[round(x, 1) for x in v],
                                               route=routes[k](), n_atoms=int(bmg.V.shape[0]), n_edges=int(bmg.E.shape[0]))
    out = dict(steps=args.steps, warmup=args.warmup, groups=args.groups, bond_only=bool(args.bond_only), device=torch.cuda.get_device_name(dev),
               results=res)
    print(json.dumps(out))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
