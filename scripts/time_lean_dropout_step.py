"""One training step of the default regression model (d_h 300, depth 3, norm aggregation, batch norm, one hidden layer of 300, MSE,
ReLU) on molecules BEYOND the tile kernels, with and without dropout in the block (`chemprop train --dropout p`; the predictor's
stays 0 here):

  fused, block p 0        FusedTrainer.step: the lean step kernels (k_step16 / k_bstep16), chosen by the route rule from 20 000
                          directed edges on — below that the rule's own choice for p = 0, reported as it is
  fused, block p 0.1      FusedTrainer.step: the lean step kernels with the hash mask inside them, asked for at any edge count
  module path, p 0.1      MPNN.loss(...).backward() + FlatAdam.step: the general row kernels with torch's nn.Dropout between them —
                          what the p = 0.1 model ran on before the lean kernels carried the mask

at 512 ZINC-shaped molecules and at 512 and 4 096 molecules of 40 atoms.  Per shape the three configurations are warmed, then timed
ALTERNATELY in one process: `groups` rounds, in each round K steps of every configuration between two device synchronisations; per
configuration the per-step time of every round and their median.
usage: python scripts/time_lean_dropout_step.py [--steps K] [--warmup W] [--groups G] [--out file.json]"""
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

SHAPES = ((512, "zinc"), (512, "synth40"), (4096, "synth40"))


def model(p_block, dev):
    torch.manual_seed(0)
    mp = BondMessagePassing(dropout=p_block)
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
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--groups", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    res = {}
    for n, kind in SHAPES:
        bmg = synth.random_batch(n, kind, seed=1)
        bmg.to(dev)
        y = torch.randn(n, 1, generator=torch.Generator().manual_seed(2)).to(dev)
        trainers = {p: FusedTrainer(model(p, dev), lr=1e-5) for p in (0.0, 0.1)}
        m = model(0.1, dev)
        sync = ddp.GradSync(list(m.parameters()), modules=[m])
        opt = FlatAdam(sync, lr=1e-5)

        def module_step():   # (what integration.HipMPNN.training_step runs where the fused step refuses: bench.py's step_module)
            with ddp.backward_on_calling_thread():
                sync.zero_grad()
                m.loss(bmg, y).backward()
            sync.allreduce()
            opt.step()

        configs = {"fused, block p 0": lambda: trainers[0.0].step(bmg, y), "fused, block p 0.1": lambda: trainers[0.1].step(bmg, y),
                   "module path, block p 0.1": module_step}
        for step in configs.values():
            run(step, args.warmup)
        per = {k: [] for k in configs}
        for _ in range(args.groups):
            for k, step in configs.items():
                per[k].append(run(step, args.steps))
        sync.wait()
        routes = {"fused, block p 0": str(trainers[0.0].last_route), "fused, block p 0.1": str(trainers[0.1].last_route), "module path, block p 0.1": "module"}
        for k, v in per.items():
            res[f"{k}, {n} {kind} mols"] = dict(us_per_step=round(sorted(v)[len(v) // 2], 1), groups_us=[round(x, 1) for x in v], route=routes[k],
                                               n_edges=int(bmg.E.shape[0]))
    out = dict(steps=args.steps, warmup=args.warmup, groups=args.groups, device=torch.cuda.get_device_name(dev), results=res)
    print(json.dumps(out))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
