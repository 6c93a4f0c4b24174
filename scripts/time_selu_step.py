"""One training step of the default regression model (BondMessagePassing d_h 300, depth 3, norm aggregation, batch norm, one hidden
layer of 300, MSE) with `--activation selu` in the block and the predictor, with and without dropout in the block:

  (a) selu, fused     FusedTrainer(..., rows_dropout=True).step: K0, the block, the head, backward, Adam — one call
      selu, module    MPNN.loss(...).backward() + FlatAdam.step — on the PARENT commit (`--root DIR --parent`) this is what such a
                      model ran on: nn.SELU was a foreign module, so the block is the chain of row kernels with torch's tau (and
                      nn.Dropout) between them, the predictor linear_fn plus torch ops, the head refused
  (b) elu, fused      the same model with "elu" on this tree: the same kernels, two other constants
  (c) relu, fused     the default ReLU model's one-call step (p = 0), this tree against the parent commit

at 512 QM9-shaped and at 512 ZINC-shaped molecules, p = 0 and p = 0.2.  Per shape the configurations are warmed, then timed
ALTERNATELY in one process: `--groups` rounds, in each round K steps of every configuration between two device synchronisations; per
configuration the per-step time of every round, their median and their spread (max - min).  The parent commit is timed by the same
script in a process of its own (`--root DIR --parent`: the package is imported from that checkout; the SELU model's module path and
the ReLU model's fused step), this tree and the parent in turn.
`--combine DIR` gathers DIR/this_N.json, DIR/parent_N.json (N = 1, 2, ..: the processes in the order they ran) and the `bench.py
--gpus 1 --steps 200 --warmup 20` result lines DIR/bench_this_N.json / DIR/bench_parent_N.json into `--out` (profiles/selu_step.json).
usage: python scripts/time_selu_step.py [--steps K] [--warmup W] [--groups G] [--root DIR] [--parent] [--out file.json] [--combine DIR]"""
import argparse
import glob
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


def _median(v):
    return sorted(v)[len(v) // 2]


def combine(d, out_path):
    load = lambda pat: [json.load(open(p)) for p in sorted(glob.glob(os.path.join(d, pat)))]
    this, parent = load("this_*.json"), load("parent_*.json")
    out = dict(script="scripts/time_selu_step.py", steps=this[0]["steps"], warmup=this[0]["warmup"], groups=this[0]["groups"], device=this[0]["device"],
               protocol="every configuration warmed, then timed alternately in one process: groups of K steps between two device synchronisations; "
                        "median and spread (max - min) of the groups' per-step times; this tree and the parent commit in processes of their own, in turn",
               this_tree=[t["results"] for t in this], parent_commit=[q["results"] for q in parent])
    groups = lambda runs, k: [x for r in runs for x in r["results"][k]["groups_us"]] if runs and all(k in r["results"] for r in runs) else None
    a, b, c = {}, {}, {}
    for n, kind in SHAPES:
        shape = f"{n} {kind} mols"
        for p in ("0", f"{P:g}"):
            f, m = groups(this, f"selu, fused, p {p}, {shape}"), groups(parent, f"selu, module path, p {p}, {shape}")
            e = groups(this, f"elu, fused, p {p}, {shape}")
            if f and m:
                a[f"p {p}, {shape}"] = dict(fused_us=round(_median(f), 1), fused_spread_us=round(max(f) - min(f), 1), parent_module_path_us=round(_median(m), 1),
                                           parent_module_path_spread_us=round(max(m) - min(m), 1), speedup=round(_median(m) / _median(f), 2),
                                           route=this[0]["results"][f"selu, fused, p {p}, {shape}"]["route"],
                                           parent_route=parent[0]["results"][f"selu, module path, p {p}, {shape}"]["route"])
            if f and e:
                b[f"p {p}, {shape}"] = dict(selu_us=round(_median(f), 1), selu_spread_us=round(max(f) - min(f), 1), elu_us=round(_median(e), 1),
                                           elu_spread_us=round(max(e) - min(e), 1),
                                           within_spreads=bool(abs(_median(f) - _median(e)) <= max(max(f) - min(f), max(e) - min(e))))
        t, q = groups(this, f"relu, fused, p 0, {shape}"), groups(parent, f"relu, fused, p 0, {shape}")
        if t and q:
            c[f"relu one-call step, {shape}"] = dict(this_tree_us=round(_median(t), 1), this_tree_spread_us=round(max(t) - min(t), 1), parent_us=round(_median(q), 1),
                                                     parent_spread_us=round(max(q) - min(q), 1), parent_min_max_us=[round(min(q), 1), round(max(q), 1)],
                                                     within_parent_spread=bool(min(q) <= _median(t) <= max(q)), not_slower_than_parent_range=bool(_median(t) <= max(q)))
    bt, bp = load("bench_this_*.json"), load("bench_parent_*.json")
    if bt and bp:
        key = next((k for k in ("graphs_per_s", "mols_per_s", "throughput", "value") if k in bt[0]), None)
        c["bench.py --gpus 1 --steps 200 --warmup 20"] = dict(this_tree=bt, parent=bp, metric=key)
        if key:
            tv, pv = [x[key] for x in bt], [x[key] for x in bp]
            c["bench.py --gpus 1 --steps 200 --warmup 20"].update(this_tree_values=tv, parent_values=pv, parent_min_max=[min(pv), max(pv)],
                                                                  within_parent_spread=bool(min(pv) <= _median(tv) <= max(pv)),
                                                                  not_slower_than_parent_range=bool(_median(tv) >= min(pv)))
    out.update(a_selu_one_call_step_against_parent_module_path=a, b_selu_against_elu_on_this_tree=b, c_no_regression_for_relu=c)
    with open(out_path, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps({k: out[k] for k in out if k not in ("this_tree", "parent_commit")}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--groups", type=int, default=5)
    ap.add_argument("--parent", action="store_true", help="the configurations of the parent commit: the SELU model's module path, the ReLU model's fused step")
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--out", default=None)
    ap.add_argument("--combine", default=None, metavar="DIR")
    args = ap.parse_args()
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if args.combine:
        return combine(args.combine, args.out or os.path.join(here, "profiles", "selu_step.json"))
    sys.path.insert(0, os.path.abspath(args.root))
    from chemprop_amd import agg as cagg
    from chemprop_amd import distributed as ddp
    from chemprop_amd import synth
    from chemprop_amd.model import MPNN, FusedTrainer, RegressionFFN
    from chemprop_amd.nn import BondMessagePassing
    from chemprop_amd.optim import FlatAdam

    dev = torch.device("cuda:0")

    def model(act, p):
        torch.manual_seed(0)
        mp = BondMessagePassing(dropout=p, activation=act)
        return MPNN(mp, cagg.NormAggregation(), RegressionFFN(n_tasks=1, input_dim=mp.output_dim, activation=act), batch_norm=True).to(dev).train()

    res = {}
    for n, kind in SHAPES:
        bmg = synth.random_batch(n, kind, seed=1)
        bmg.to(dev)
        y = torch.randn(n, 1, generator=torch.Generator().manual_seed(2)).to(dev)
        configs, routes, syncs = {}, {}, []

        def fused(name, act, p, **kw):
            tr = FusedTrainer(model(act, p), lr=1e-5, **kw)
            configs[name] = lambda: tr.step(bmg, y)
            routes[name] = lambda: str(tr.last_route)

        def module_path(name, act, p):
            m = model(act, p)
            sync = ddp.GradSync(list(m.parameters()), modules=[m])
            opt = FlatAdam(sync, lr=1e-5)
            syncs.append(sync)

            def step():   # (what integration.HipMPNN.training_step runs where the fused step refuses)
                with ddp.backward_on_calling_thread():
                    sync.zero_grad()
                    m.loss(bmg, y).backward()
                sync.allreduce()
                opt.step()

            configs[name] = step
            routes[name] = lambda: "module:" + str(m.message_passing.__dict__.get("_dmpnn_route"))

        fused("relu, fused, p 0", "relu", 0.0)
        for p in (0.0, P):
            if args.parent:
                module_path(f"selu, module path, p {p:g}", "selu", p)
            else:
                fused(f"selu, fused, p {p:g}", "selu", p, rows_dropout=True)
                fused(f"elu, fused, p {p:g}", "elu", p, rows_dropout=True)
        for step in configs.values():
            run(step, args.warmup)
        per = {k: [] for k in configs}
        for _ in range(args.groups):
            for k, step in configs.items():
                per[k].append(run(step, args.steps))
        for s in syncs:
            s.wait()
        for k, v in per.items():
            res[f"{k}, {n} {kind} mols"] = dict(us_per_step=round(_median(v), 1), groups_us=[round(x, 1) for x in v], spread_us=round(max(v) - min(v), 1),
                                               route=routes[k](), n_atoms=int(bmg.V.shape[0]), n_edges=int(bmg.E.shape[0]))
    out = dict(steps=args.steps, warmup=args.warmup, groups=args.groups, root=os.path.basename(os.path.abspath(args.root)) if args.parent else "this tree",
               device=torch.cuda.get_device_name(dev), results=res)
    print(json.dumps(out))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
