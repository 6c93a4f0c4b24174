"""One training step of a WIDE regression model (depth 3, norm aggregation, batch norm, one hidden layer of 300, MSE, ReLU; the block
wider than the 320 columns of the tile and lean step kernels) with and without dropout in the block (`chemprop train --dropout p
--message-hidden-dim 600`; the predictor's stays 0 here):

  fused, block p 0        FusedTrainer.step: the per-step general route on the f16 pipe (general16), the route rule's choice
  fused, block p 0.2      FusedTrainer(rows_dropout=True).step: the same route with the hash mask in the row kernels' epilogue
  module path, p 0.2      MPNN.loss(...).backward() + FlatAdam.step: the same row kernels with torch's nn.Dropout between them —
                          what the p = 0.2 model ran on before the row kernels carried the mask

at 512 ZINC-shaped molecules with d_h 600 and at 4 096 molecules of 40 atoms with d_h 400.  Per shape the three configurations are
warmed, then timed ALTERNATELY in one process: `groups` rounds, in each round K steps of every configuration between two device
synchronisations; per configuration the per-step time of every round and their median.
usage: python scripts/time_rows_dropout_step.py [--steps K] [--warmup W] [--groups G] [--out file.json]"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from chemprop_amd import agg as cagg  # noqa: E402
from chemprop_amd import synth  # noqa: E402
from chemprop_amd.model import MPNN, FusedTrainer, RegressionFFN  # noqa: E402
from chemprop_amd.nn import BondMessagePassing  # noqa: E402
from chemprop_amd import distributed as ddp  # noqa: E402
from chemprop_amd.optim import FlatAdam  # noqa: E402

SHAPES = ((512, "zinc", 600), (4096, "synth40", 400))
P = 0.2


def model(p_block, d_h, dev):
    torch.manual_seed(0)
    mp = BondMessagePassing(d_h=d_h, dropout=p_block)
    return MPNN(mp, cagg.NormAggregation(), RegressionFFN(n_tasks=1, input_dim=mp.output_dim), batch_norm=True).to(dev).train()


def run(step, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--groups", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    res = {}
    for n, kind, d_h in SHAPES:
        bmg = synth.random_batch(n, kind, seed=1)
        bmg.to(dev)
        y = torch.randn(n, 1, generator=torch.Generator().manual_seed(2)).to(dev)
        trainers = {p: FusedTrainer(model(p, d_h, dev), lr=1e-5, rows_dropout=True) for p in (0.0, P)}
        m = model(P, d_h, dev)
        sync = ddp.GradSync(list(m.parameters()), modules=[m])
        opt = FlatAdam(sync, lr=1e-5)

        def module_step():   # (what integration.HipMPNN.training_step runs where the fused step refuses: bench.py's step_module)
            with ddp.backward_on_calling_thread():
                sync.zero_grad()
                m.loss(bmg, y).backward()
            sync.allreduce()
            opt.step()

        configs = {"fused, block p 0": lambda: trainers[0.0].step(bmg, y), f"fused, block p {P}": lambda: trainers[P].step(bmg, y),
                   f"module path, block p {P}": module_step}
        for step in configs.values():
            run(step, args.warmup)
        per = {k: [] for k in configs}
        for _ in range(args.groups):
            for k, step in configs.items():
                per[k].append(run(step, args.steps))
        sync.wait()
        routes = {"fused, block p 0": str(trainers[0.0].last_route), f"fused, block p {P}": str(trainers[P].last_route), f"module path, block p {P}": "module"}
        for k, v in per.items():
            res[f"{k}, {n} {kind} mols, d_h {d_h}"] = dict(us_per_step=round(sorted(v)[len(v) // 2], 1), groups_us=[round(x, 1) for x in v], route=routes[k],
                                                           n_edges=int(bmg.E.shape[0]))
    out = dict(steps=args.steps, warmup=args.warmup, groups=args.groups, device=torch.cuda.get_device_name(dev), results=res)
    print(json.dumps(out))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
