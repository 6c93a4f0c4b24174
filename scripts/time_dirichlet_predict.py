#!/usr/bin/env python
"""Inference of models with a Dirichlet classification head (depth 3, d_h 300, norm aggregation, batch norm, one hidden layer of 300,
ReLU — the shapes of ``profiles/dirichlet_step.json``): a 12-task ``BinaryDirichletFFN`` and a 5-class, 4-task
``MulticlassDirichletFFN`` at 512 QM9-shaped and 512 ZINC-shaped molecules, two calls each:

  predict                 ``MPNN.predict(bmg)``
  predict with targets    predictions AND the validation loss: ``fused_predict(model, bmg, targets=T)`` where the inference head takes
                          the model, else what a validation step runs on the modules — ``model(bmg)`` and ``model.loss(bmg, T)``, a
                          second pass over the fingerprint

The protocol is ``scripts/bench_predict.py``'s (``alternate`` / ``summary`` / ``verdict`` are imported from it): one process, eval mode
under ``torch.no_grad()``, every shape warmed first, the two calls ALTERNATED in blocks of ``--calls`` calls, ``--reps`` blocks each, a
block timed by the host clock with one device synchronise at each end; per call the median block with min..max in microseconds.

``--parent TREE``: the comparison side — the same models and the same two calls on the tree at TREE (a built checkout of the parent
commit, where ``MPNN.predict`` on these models IS the module path), each tree in a process of its own (one process cannot hold two
builds of the package), the trees alternated ``--rounds`` times; per tree the median over every round's blocks and their min..max.  A
speed-up is claimed only where the medians differ by more than the larger of the two spreads.

Writes ``profiles/dirichlet_predict.json`` (``--out``).  Needs a HIP device: there is nothing to measure without one."""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_predict import alternate, summary, verdict  # noqa: E402  (the protocol: not copied)

SHAPES = ((512, "qm9"), (512, "zinc"))
HEADS = (("binary, 12 tasks", 2, 12), ("K=5, 4 tasks", 5, 4))
CALLS = ("predict", "predict with targets")
D_H, DEPTH = 300, 3


def measure(args) -> dict:
    """Both calls of every model on the package that ``sys.path`` leads to: microseconds per call of every block."""
    import torch

    import chemprop_amd
    from chemprop_amd import _lib, synth
    from chemprop_amd import agg as cagg
    from chemprop_amd import model as cm
    from chemprop_amd.nn import BondMessagePassing
    from chemprop_amd.predict import fused_predict

    lib = _lib.load()
    dev = torch.device("cuda:0")
    res = dict(package=os.path.dirname(chemprop_amd.__file__), device=torch.cuda.get_device_name(0), models={})
    with torch.no_grad():
        for n, kind in SHAPES:
            bmg = synth.random_batch(n, kind, seed=1000)
            bmg.to(dev)
            for name, K, t in HEADS:
                torch.manual_seed(0)
                pred = cm.BinaryDirichletFFN(n_tasks=t, input_dim=D_H) if K == 2 else cm.MulticlassDirichletFFN(K, n_tasks=t, input_dim=D_H)
                model = cm.MPNN(BondMessagePassing(d_h=D_H, depth=DEPTH), cagg.NormAggregation(), pred, batch_norm=True).to(dev).eval()
                model.bn.running_mean.uniform_(-0.1, 0.1), model.bn.running_var.uniform_(0.5, 2.0)
                gen = torch.Generator().manual_seed(2)
                T = torch.randint(0, K, (n, t), generator=gen).float()
                T[torch.rand(n, t, generator=gen) < 0.1] = float("nan")
                T = T.to(dev)

                def predict():
                    return model.predict(bmg)

                def with_targets():
                    r = fused_predict(model, bmg, targets=T)
                    return (r.preds, r.loss[0]) if r is not None else (model(bmg), model.loss(bmg, T))

                taken = fused_predict(model, bmg, targets=T) is not None and fused_predict(model, bmg, targets=T) is not None
                launches = int(lib.dmpnn_last_launch_count()) if taken else None   # (of the steady call with targets: the split images ready)
                for _ in range(args.warmup):
                    predict(), with_targets()
                a, (b, loss), m = predict(), with_targets(), model(bmg)
                torch.cuda.synchronize()
                blocks = alternate(predict, with_targets, args.calls, args.reps, events=False)
                res["models"][f"{name}, {n} {kind} mols"] = {
                    "n_atoms": int(bmg.V.shape[0]), "inference head": taken, "head launches with targets": launches,
                    "max |predict - forward| / max |forward|": float((a - m).abs().max() / m.abs().max()), "loss": float(loss),
                    CALLS[0]: blocks[0], CALLS[1]: blocks[1]}
    return res


def child(tree: str, args) -> dict:
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--tree", tree, "--calls", str(args.calls), "--reps", str(args.reps),
                          "--warmup", str(args.warmup)], env=dict(os.environ, DMPNN_LIB=os.path.join(tree, "chemprop_amd", "libdmpnn_gfx950.so")),
                         capture_output=True, text=True, timeout=600)
    if out.returncode != 0:
        raise SystemExit(f"time_dirichlet_predict: the process on {tree} failed ({out.returncode})\n{out.stderr[-2000:]}")
    r = json.loads(out.stdout.strip().splitlines()[-1])
    assert os.path.abspath(r["package"]).startswith(os.path.abspath(tree) + os.sep), (r["package"], tree)
    return r


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit")
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "dirichlet_predict.json"))
    ap.add_argument("--tree", default=HERE, help=argparse.SUPPRESS)   # (the child processes: the package to import)
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        sys.path.insert(0, os.path.abspath(args.tree))
        import torch

        if not torch.cuda.is_available():
            print("time_dirichlet_predict: no HIP device — nothing is measured without one", file=sys.stderr)
            return 2
        print(json.dumps(measure(args)))
        return 0
    trees = {"this tree": HERE}
    if args.parent:
        trees["parent"] = os.path.abspath(args.parent)
    runs = {k: [] for k in trees}
    for _ in range(args.rounds):   # (every tree in a process of its own, the trees alternated)
        for k, tree in trees.items():
            runs[k].append(child(tree, args))
    results = {}
    for model in runs["this tree"][0]["models"]:
        row = {k: v for k, v in runs["this tree"][0]["models"][model].items() if k not in CALLS}
        for call in CALLS:
            per = {k: summary([us for r in rs for us in r["models"][model][call]]) for k, rs in runs.items()}
            row[call] = dict(per, **({"against the parent": verdict(per["this tree"], per["parent"])} if args.parent else {}))
        if args.parent:
            row["inference head on the parent"] = runs["parent"][0]["models"][model]["inference head"]
        results[model] = row
        print(json.dumps({model: row}), flush=True)
    out = dict(tool="scripts/time_dirichlet_predict.py", device=runs["this tree"][0]["device"], calls_per_block=args.calls, blocks_per_call=args.reps,
               rounds=args.rounds, clock="host clock, one synchronise at each end of a block", unit="microseconds per call",
               verdict="module_over_predict = parent median / this tree's median; a claim only beyond the larger of the two spreads (max - min)",
               results=results)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(f"wrote {args.out}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
