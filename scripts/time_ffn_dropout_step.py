"""One training step of the default regression model (d_h 300, depth 3, norm aggregation, batch norm, one hidden layer of 300, MSE,
ReLU) at 512 QM9-shaped molecules, with and without dropout in the block and the predictor (`chemprop train --dropout p` sets both):

  fused, block p b, predictor p f     FusedTrainer(ffn_dropout=True).step, (b, f) in {0, 0.1}^2   (the four-launch row form of the head;
                                                                                                   f = 0.1 is the new case)
  module path, block p 0.1, ...       MPNN.loss(...).backward() + FlatAdam.step                   (the route the p = 0.1 model took
                                                                                                   before: torch's nn.Dropout between
                                                                                                   the predictor's layers)
  the fused steps at 4 096 molecules                                                              (the chain form of the head)

Per configuration: W warm-up steps, then `groups` groups of K steps each between two device synchronisations; the per-step time of
every group, the median reported.
usage: python scripts/time_ffn_dropout_step.py [--steps K] [--warmup W] [--groups G] [--out file.json]"""
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


def model(p_block, p_ffn, dev):
    torch.manual_seed(0)
    mp = BondMessagePassing(dropout=p_block)
    return MPNN(mp, cagg.NormAggregation(), RegressionFFN(n_tasks=1, input_dim=mp.output_dim, dropout=p_ffn), batch_norm=True).to(dev).train()


def timed(step, steps, warmup, groups):
    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    per = []
    for _ in range(groups):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            step()
        torch.cuda.synchronize()
        per.append((time.perf_counter() - t0) / steps * 1e6)
    per.sort()
    return per[len(per) // 2], per


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--groups", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    res = {}
    for n in (512, 4096):
        bmg = synth.random_batch(n, "qm9", seed=1)
        bmg.to(dev)
        y = torch.randn(n, 1, generator=torch.Generator().manual_seed(2)).to(dev)
        for pb, pf in ((0.0, 0.0), (0.0, 0.1), (0.1, 0.0), (0.1, 0.1)):
            tr = FusedTrainer(model(pb, pf, dev), lr=1e-5, ffn_dropout=True)
            med, per = timed(lambda: tr.step(bmg, y), args.steps, args.warmup, args.groups)
            res[f"fused, block p {pb}, predictor p {pf}, {n} mols"] = dict(us_per_step=round(med, 1), groups_us=[round(v, 1) for v in per],
                                                                          route=str(tr.last_route))
        if n != 512:
            continue
        m = model(0.1, 0.1, dev)
        sync = ddp.GradSync(list(m.parameters()), modules=[m])
        opt = FlatAdam(sync, lr=1e-5)

        def module_step():   # (what integration.HipMPNN.training_step ran for this model before: bench.py's step_module)
            with ddp.backward_on_calling_thread():
                sync.zero_grad()
                m.loss(bmg, y).backward()
            sync.allreduce()
            opt.step()

        med, per = timed(module_step, args.steps, args.warmup, args.groups)
        sync.wait()
        res[f"module path, block p 0.1, predictor p 0.1, {n} mols"] = dict(us_per_step=round(med, 1), groups_us=[round(v, 1) for v in per])
    out = dict(steps=args.steps, warmup=args.warmup, groups=args.groups, device=torch.cuda.get_device_name(dev), results=res)
    print(json.dumps(out))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
