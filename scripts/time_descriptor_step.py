"""One training step of the default regression model (d_h 300, depth 3, norm aggregation, batch norm, one hidden layer of 300, MSE) at
512 QM9-shaped molecules, with and without molecule descriptors X_d:

  fused, no X_d                  FusedTrainer.step                                  (the one-call step as before)
  fused, d_xd 200                FusedTrainer.step(..., X_d=...)                    (the four-launch row form of the head)
  fused, d_xd 2048 binary        FusedTrainer.step(..., X_d=...)                    (the chain form: the first layer is 2 348 wide)
  module path, d_xd 200 | 2048   MPNN.loss(..., X_d=...).backward() + FlatAdam.step on the same model shapes and batch

Per configuration: W warm-up steps, then `groups` groups of K steps each between two device synchronisations; the per-step time of
every group, the median reported.
usage: python scripts/time_descriptor_step.py [--steps K] [--warmup W] [--groups G] [--out file.json]"""
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


def model(d_xd, dev):
    torch.manual_seed(0)
    mp = BondMessagePassing()
    return MPNN(mp, cagg.NormAggregation(), RegressionFFN(n_tasks=1, input_dim=mp.output_dim + d_xd), batch_norm=True).to(dev).train()


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
    ap.add_argument("--n-mols", type=int, default=512)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    n = args.n_mols
    bmg = synth.random_batch(n, "qm9", seed=1)
    bmg.to(dev)
    gen = torch.Generator().manual_seed(2)
    y = torch.randn(n, 1, generator=gen).to(dev)
    x200 = torch.randn(n, 200, generator=gen).to(dev)
    x2048 = (torch.rand(n, 2048, generator=gen) < 0.1).float().to(dev)

    res = {}
    for name, d_xd, X in (("fused, no X_d", 0, None), ("fused, d_xd 200", 200, x200), ("fused, d_xd 2048 binary", 2048, x2048)):
        tr = FusedTrainer(model(d_xd, dev), lr=1e-5)
        med, per = timed(lambda: tr.step(bmg, y, X_d=X), args.steps, args.warmup, args.groups)
        res[name] = dict(us_per_step=round(med, 1), groups_us=[round(v, 1) for v in per], route=str(tr.last_route))

    for d_xd, X in ((200, x200), (2048, x2048)):
        m = model(d_xd, dev)
        sync = ddp.GradSync(list(m.parameters()), modules=[m])
        opt = FlatAdam(sync, lr=1e-5)

        def module_step():   # (what integration.HipMPNN.training_step runs on the module path: bench.py's step_module with X_d)
            with ddp.backward_on_calling_thread():
                sync.zero_grad()
                m.loss(bmg, y, X_d=X).backward()
            sync.allreduce()
            opt.step()

        med, per = timed(module_step, args.steps, args.warmup, args.groups)
        sync.wait()
        res[f"module path, d_xd {d_xd}"] = dict(us_per_step=round(med, 1), groups_us=[round(v, 1) for v in per])
    out = dict(n_mols=n, steps=args.steps, warmup=args.warmup, groups=args.groups, device=torch.cuda.get_device_name(dev), results=res)
    print(json.dumps(out))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
