"""One training step of the default regression model (depth 3, d_h 300, batch norm, one hidden layer of 300, MSE, ReLU) with
AttentiveAggregation, and the aggregation on its own:

  fused, attentive         FusedTrainer(attentive=True).step: the attention as a stage of two kernels around the head, one call
  module path, chain       MPNN.loss(...).backward() + FlatAdam.step with DMPNN_ATTN=chain: the chain of torch ops around two generic
                           reductions — what this model ran on before the kernels
  module path, new node    the same path on the one autograd node of dmpnn_molagg_attn_fwd / _bwd
  fused, norm              FusedTrainer.step of the same model with NormAggregation: what the stage costs

at 512 QM9-shaped and 512 ZINC-shaped molecules.  Per shape the configurations are warmed, then timed ALTERNATELY in one process:
`groups` rounds, in each round K steps of every configuration between two device synchronisations; per configuration the per-step
time of every round, their median and their spread (max - min).

The aggregation alone, forward + backward (autograd on the module, HIP events around K repetitions), new node against chain, at
512 QM9-shaped molecules and at 4 096 molecules of 40 atoms, d_h 300.
usage: python scripts/time_attentive_step.py [--steps K] [--warmup W] [--groups G] [--out file.json]"""
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
AGG_SHAPES = ((512, "qm9"), (4096, "synth40"))
D_H = 300


def model(attentive, dev):
    torch.manual_seed(0)
    mp = BondMessagePassing(d_h=D_H)
    agg = cagg.AttentiveAggregation(output_size=D_H) if attentive else cagg.NormAggregation()
    return MPNN(mp, agg, RegressionFFN(n_tasks=1, input_dim=mp.output_dim), batch_norm=True).to(dev).train()


def run(step, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e6


def run_events(step, steps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(steps):
        step()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / steps * 1e3


def alternate(configs, runner, args):
    for step in configs.values():
        runner(step, args.warmup)
    per = {k: [] for k in configs}
    for _ in range(args.groups):
        for k, step in configs.items():
            per[k].append(runner(step, args.steps))
    return {k: dict(us=round(sorted(v)[len(v) // 2], 1), spread_us=round(max(v) - min(v), 1), groups_us=[round(x, 1) for x in v]) for k, v in per.items()}


def with_env(value, fn):
    def step():
        if value is None:
            os.environ.pop("DMPNN_ATTN", None)
        else:
            os.environ["DMPNN_ATTN"] = value
        try:
            fn()
        finally:
            os.environ.pop("DMPNN_ATTN", None)
    return step


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--groups", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    res, agg_res = {}, {}
    for n, kind in SHAPES:
        bmg = synth.random_batch(n, kind, seed=1)
        bmg.to(dev)
        y = torch.randn(n, 1, generator=torch.Generator().manual_seed(2)).to(dev)
        fused = FusedTrainer(model(True, dev), lr=1e-5, attentive=True)
        norm = FusedTrainer(model(False, dev), lr=1e-5)
        mods = {}
        for name in ("chain", "node"):
            m = model(True, dev)
            sync = ddp.GradSync(list(m.parameters()), modules=[m])
            mods[name] = (m, sync, FlatAdam(sync, lr=1e-5))

        def module_step(name):
            m, sync, opt = mods[name]

            def step():   # (what integration.HipMPNN.training_step runs where the fused step refuses)
                with ddp.backward_on_calling_thread():
                    sync.zero_grad()
                    m.loss(bmg, y).backward()
                sync.allreduce()
                opt.step()
            return step

        configs = {"fused, attentive": lambda: fused.step(bmg, y),
                   "module path, chain": with_env("chain", module_step("chain")),
                   "module path, new node": with_env(None, module_step("node")),
                   "fused, norm": lambda: norm.step(bmg, y)}
        r = alternate(configs, run, args)
        for _, sync, _ in mods.values():
            sync.wait()
        r["fused, attentive"]["route"], r["fused, norm"]["route"] = str(fused.last_route), str(norm.last_route)
        for k, v in r.items():
            res[f"{k}, {n} {kind} mols"] = dict(v, n_atoms=int(bmg.V.shape[0]), n_edges=int(bmg.E.shape[0]))
    for n, kind in AGG_SHAPES:
        bmg = synth.random_batch(n, kind, seed=1)
        bmg.to(dev)
        nV = int(bmg.V.shape[0])
        torch.manual_seed(3)
        mod = cagg.AttentiveAggregation(output_size=D_H).to(dev)
        H = torch.randn(nV, D_H, device=dev, requires_grad=True)
        G = torch.randn(n, D_H, device=dev)

        def fb():
            H.grad = mod.W.weight.grad = mod.W.bias.grad = None
            (mod(H, bmg.batch) * G).sum().backward()

        r = alternate({"new node": with_env(None, fb), "chain": with_env("chain", fb)}, run_events, args)
        for k, v in r.items():
            agg_res[f"aggregation forward + backward, {k}, {n} {kind} mols"] = dict(v, n_atoms=nV, d_h=D_H)
    out = dict(steps=args.steps, warmup=args.warmup, groups=args.groups, device=torch.cuda.get_device_name(dev), results=res, aggregation=agg_res)
    print(json.dumps(out))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
