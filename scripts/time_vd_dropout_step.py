"""One training step of a regression model WITH ATOM DESCRIPTORS (d_h 300, depth 3, d_vd 20, norm aggregation, batch norm, one hidden
layer of 300, MSE, ReLU) with and without dropout in the block (`chemprop train --atom-descriptors-path ... --dropout p`; the
predictor's stays 0 here):

  fused, block p 0        FusedTrainer.step: the block, the atom-descriptor stage (dmpnn_vd_forward / _backward), the head — one call
  fused, block p 0.2      FusedTrainer(vd_dropout=True).step: the same call with the hash mask in the block's kernels AND, the fourth
                          site, in the atom-descriptor stage's own kernels
  module path, p 0.2      MPNN.loss(...).backward() + FlatAdam.step: the row kernels with torch's nn.Dropout between them — what the
                          p = 0.2 model ran on before the stage carried the mask

at 512 QM9-shaped and at 512 ZINC-shaped molecules.  Per shape the configurations are warmed, then timed ALTERNATELY in one process:
`groups` rounds, in each round K steps of every configuration between two device synchronisations; per configuration the per-step
time of every round and their median.  `--only-p0` times the first configuration alone (no keyword of this change is used: the same
script runs on a commit without it, which is how the p = 0 step is compared across commits).
usage: python scripts/time_vd_dropout_step.py [--steps K] [--warmup W] [--groups G] [--only-p0] [--out file.json]"""
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

SHAPES = ((512, "qm9"), (512, "zinc"))
P, D_VD = 0.2, 20


def model(p_block, dev):
    torch.manual_seed(0)
    mp = BondMessagePassing(d_vd=D_VD, dropout=p_block)
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
    ap.add_argument("--only-p0", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    res = {}
    for n, kind in SHAPES:
        bmg = synth.random_batch(n, kind, seed=1)
        bmg.to(dev)
        gen = torch.Generator().manual_seed(2)
        y = torch.randn(n, 1, generator=gen).to(dev)
        V = torch.randn(int(bmg.V.shape[0]), D_VD, generator=gen).to(dev)
        t0 = FusedTrainer(model(0.0, dev), lr=1e-5)
        configs = {"fused, block p 0": lambda: t0.step(bmg, y, V_d=V)}
        routes = {"fused, block p 0": lambda: str(t0.last_route)}
        sync = None
        if not args.only_p0:
            tp = FusedTrainer(model(P, dev), lr=1e-5, rows_dropout=True, vd_dropout=True)
            m = model(P, dev)
            sync = ddp.GradSync(list(m.parameters()), modules=[m])
            opt = FlatAdam(sync, lr=1e-5)

            def module_step():   # (what integration.HipMPNN.training_step runs where the fused step refuses: bench.py's step_module)
                with ddp.backward_on_calling_thread():
                    sync.zero_grad()
                    m.loss(bmg, y, V_d=V).backward()
                sync.allreduce()
                opt.step()

            configs[f"fused, block p {P}"] = lambda: tp.step(bmg, y, V_d=V)
            configs[f"module path, block p {P}"] = module_step
            routes[f"fused, block p {P}"] = lambda: str(tp.last_route)
            routes[f"module path, block p {P}"] = lambda: "module"
        for step in configs.values():
            run(step, args.warmup)
        per = {k: [] for k in configs}
        for _ in range(args.groups):
            for k, step in configs.items():
                per[k].append(run(step, args.steps))
        if sync is not None:
            sync.wait()
        for k, v in per.items():
            res[f"{k}, {n} {kind} mols, d_vd {D_VD}"] = dict(us_per_step=round(sorted(v)[len(v) // 2], 1), groups_us=[round(x, 1) for x in v],
                                                            route=routes[k](), n_atoms=int(bmg.V.shape[0]), n_edges=int(bmg.E.shape[0]))
    out = dict(steps=args.steps, warmup=args.warmup, groups=args.groups, only_p0=bool(args.only_p0), device=torch.cuda.get_device_name(dev),
               results=res)
    print(json.dumps(out))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
