"""One training step of a two-component regression model (two D-MPNN blocks of d_h 300, depth 3, norm aggregation, batch norm over
the 600-wide fingerprint, one hidden layer of 300, MSE) at 512 molecules per component, and the single-component step as the control:

  fused, single qm9              FusedTrainer.step on MPNN                               (the control)
  fused, shared qm9 + qm9        FusedTrainer.step on MulticomponentMPNN, one shared block (merged batch of 1 024 molecules)
  fused, separate qm9 + qm9      FusedTrainer.step, one block per component
  fused, separate cgr + qm9      FusedTrainer.step, a CGR component beside a QM9 one (different d_v / d_e)
  module path, <the same three>  MulticomponentMPNN.loss(...).backward() + FlatAdam.step

Per configuration: W warm-up steps, then `groups` groups of K steps each between two device synchronisations; the per-step time of
every group, the median reported.
usage: python scripts/time_multicomponent_step.py [--steps K] [--warmup W] [--groups G] [--out file.json]"""
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
from chemprop_amd.model import MPNN, FusedTrainer, MulticomponentMPNN, RegressionFFN  # noqa: E402
from chemprop_amd.nn import BondMessagePassing, MulticomponentMessagePassing  # noqa: E402
from chemprop_amd import distributed as ddp  # noqa: E402
from chemprop_amd.optim import FlatAdam  # noqa: E402

DIMS = dict(qm9=(72, 14), cgr=(106, 28))


def model(kinds, shared, dev):
    torch.manual_seed(0)
    if kinds is None:
        mp = BondMessagePassing()
        return MPNN(mp, cagg.NormAggregation(), RegressionFFN(n_tasks=1, input_dim=mp.output_dim), batch_norm=True).to(dev).train()
    blocks = [BondMessagePassing(*DIMS[k]) for k in (kinds[:1] if shared else kinds)]
    mp = MulticomponentMessagePassing(blocks, len(kinds), shared=shared)
    return MulticomponentMPNN(mp, cagg.NormAggregation(), RegressionFFN(n_tasks=1, input_dim=mp.output_dim), batch_norm=True).to(dev).train()


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
    bat = {}
    for k, seed in (("qm9", 1), ("qm9b", 3), ("cgr", 5)):
        bat[k] = synth.random_batch(n, k.rstrip("b"), seed=seed)
        bat[k].to(dev)
    y = torch.randn(n, 1, generator=torch.Generator().manual_seed(2)).to(dev)
    configs = (("single qm9", None, False, bat["qm9"]), ("shared qm9 + qm9", ["qm9", "qm9"], True, [bat["qm9"], bat["qm9b"]]),
               ("separate qm9 + qm9", ["qm9", "qm9"], False, [bat["qm9"], bat["qm9b"]]),
               ("separate cgr + qm9", ["cgr", "qm9"], False, [bat["cgr"], bat["qm9"]]))
    res = {}
    for name, kinds, shared, b in configs:
        tr = FusedTrainer(model(kinds, shared, dev), lr=1e-5)
        med, per = timed(lambda: tr.step(b, y), args.steps, args.warmup, args.groups)
        res[f"fused, {name}"] = dict(us_per_step=round(med, 1), groups_us=[round(v, 1) for v in per], route=str(tr.last_route))
    for name, kinds, shared, b in configs[1:]:
        m = model(kinds, shared, dev)
        sync = ddp.GradSync(list(m.parameters()), modules=[m])
        opt = FlatAdam(sync, lr=1e-5)

        def module_step():   # (the module path: every block through its autograd node, the head as one more, the flat Adam)
            with ddp.backward_on_calling_thread():
                sync.zero_grad()
                m.loss(b, y).backward()
            sync.allreduce()
            opt.step()

        med, per = timed(module_step, args.steps, args.warmup, args.groups)
        sync.wait()
        res[f"module path, {name}"] = dict(us_per_step=round(med, 1), groups_us=[round(v, 1) for v in per])
    out = dict(n_mols=n, steps=args.steps, warmup=args.warmup, groups=args.groups, device=torch.cuda.get_device_name(dev), results=res)
    print(json.dumps(out))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
