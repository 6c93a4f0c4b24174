"""One training step of a model with a binary MCC head (depth 3, d_h 300, batch norm, one hidden layer of 300, ReLU, a
BinaryClassificationFFN of 12 tasks with BinaryMCC — `chemprop train --task-type classification --loss-function mcc`):

  one-call step            FusedTrainer.step: the criterion is the MCC stage of the head (k_mcc_cols + k_mcc_finish)
  module path, torch ops   MPNN.loss(...).backward() + FlatAdam.step with head_loss forced to None: aggregation, batch norm, the
                           predictor and the criterion (masked_loss(kind="mcc")) as torch ops and autograd nodes — what such a
                           model ran on before DMPNN_LOSS_MCC
  module path, one node    the same path with everything behind the block as the one _HeadLoss node

at 512 QM9-shaped and 512 ZINC-shaped molecules.  The method is scripts/time_spectral_step.py's: the configurations are warmed,
then timed ALTERNATELY in one process — `groups` rounds, in each round K steps of every configuration between two device
synchronisations on a host clock; per configuration the median per-step time and the spread (max - min) over the rounds.

--unchanged TREE: also the paths that share the head's host driver with the new code but must not slow down — the one-call step and
the MPNN.predict call of the default regression model at 512 QM9-shaped molecules (the regression row of scripts/bench_predict.py)
— on this tree and on the tree at TREE (a checkout of the parent commit, built), each in a process of its own (one process cannot
hold two builds of the package), the two trees alternated `--rounds` times; per tree and path the median over every round's groups,
and the spread over all of them.  --bench with it: `bench.py --gpus 1 --steps S --warmup W` of either tree, alternated the same way
(the headline value and ms_per_step of its JSON line).

--profile-steps N: nothing but N one-call steps of the MCC model at 512 QM9-shaped molecules behind a warm-up — the program a
kernel trace is taken of for the criterion stage's own kernel time.

usage: python scripts/time_mcc_step.py [--steps K] [--warmup W] [--groups G] [--unchanged TREE [--bench]] [--rounds R] [--out file.json]"""
import argparse
import json
import os
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=200)
ap.add_argument("--warmup", type=int, default=20)
ap.add_argument("--groups", type=int, default=5)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--unchanged", default=None, help="a built checkout of the parent commit")
ap.add_argument("--profile-steps", type=int, default=0)
ap.add_argument("--bench", action="store_true", help="with --unchanged: bench.py's headline of either tree as well")
ap.add_argument("--bench-steps", type=int, default=20)
ap.add_argument("--bench-warmup", type=int, default=5)
ap.add_argument("--out", default=None)
ap.add_argument("--tree", default=HERE, help=argparse.SUPPRESS)             # (the child processes of --unchanged: the package to import)
ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
ARGS = ap.parse_args()
sys.path.insert(0, os.path.abspath(ARGS.tree))

import torch  # noqa: E402

from chemprop_amd import agg as cagg  # noqa: E402
from chemprop_amd import distributed as ddp  # noqa: E402
from chemprop_amd import model as cm  # noqa: E402
from chemprop_amd import synth  # noqa: E402
from chemprop_amd.nn import BondMessagePassing  # noqa: E402
from chemprop_amd.optim import FlatAdam  # noqa: E402

SHAPES = ((512, "qm9"), (512, "zinc"))
D_H, TASKS = 300, 12
PATHS = ("regression step", "regression predict")


def run(step, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e6


def alternate(configs, args):
    for step in configs.values():
        run(step, args.warmup)
    per = {k: [] for k in configs}
    for _ in range(args.groups):
        for k, step in configs.items():
            per[k].append(run(step, args.steps))
    return per


def summary(v):
    return dict(us=round(sorted(v)[len(v) // 2], 1), spread_us=round(max(v) - min(v), 1), groups_us=[round(x, 1) for x in v])


def build(pred, dev):
    torch.manual_seed(0)
    mp = BondMessagePassing(d_h=D_H)
    return cm.MPNN(mp, cagg.NormAggregation(), pred(mp.output_dim), batch_norm=True).to(dev).train()


def targets(n, dev):
    """0 / 1 targets, about 30 % positives, 20 % missing."""
    gen = torch.Generator().manual_seed(2)
    T = (torch.rand(n, TASKS, generator=gen) < 0.3).float()
    T[torch.rand(n, TASKS, generator=gen) < 0.2] = float("nan")
    return T.to(dev)


def mcc_pred(d):
    return cm.BinaryClassificationFFN(n_tasks=TASKS, input_dim=d, criterion=cm.BinaryMCC(torch.ones(TASKS)))


def mcc(args, dev):
    res = {}
    real_head_loss = cm.head_loss
    for n, kind in SHAPES:
        bmg = synth.random_batch(n, kind, seed=1)
        bmg.to(dev)
        T = targets(n, dev)
        fused = cm.FusedTrainer(build(mcc_pred, dev), lr=1e-5)
        mods = {}
        for which in ("torch", "node"):
            m = build(mcc_pred, dev)
            sync = ddp.GradSync(list(m.parameters()), modules=[m])
            mods[which] = (m, sync, FlatAdam(sync, lr=1e-5))

        def module_step(which):
            m, sync, opt = mods[which]

            def step():   # (what integration.HipMPNN.training_step runs where the fused step refuses)
                cm.head_loss = (lambda *a, **k: None) if which == "torch" else real_head_loss
                try:
                    with ddp.backward_on_calling_thread():
                        sync.zero_grad()
                        m.loss(bmg, T).backward()
                    sync.allreduce()
                    opt.step()
                finally:
                    cm.head_loss = real_head_loss
            return step

        per = alternate({"one-call step": lambda: fused.step(bmg, T), "module path, torch ops": module_step("torch"),
                         "module path, one node": module_step("node")}, args)
        for _, sync, _ in mods.values():
            sync.wait()
        r = {k: summary(v) for k, v in per.items()}
        r["one-call step"]["route"] = str(fused.last_route)
        r["ratio torch ops / one-call"] = round(r["module path, torch ops"]["us"] / r["one-call step"]["us"], 3)
        r["ratio one node / one-call"] = round(r["module path, one node"]["us"] / r["one-call step"]["us"], 3)
        res[f"binary MCC, t = {TASKS}, {n} {kind} mols"] = dict(r, n_atoms=int(bmg.V.shape[0]), n_edges=int(bmg.E.shape[0]))
    return res


def unchanged_child(args, dev):
    """The one-call step and the MPNN.predict call of the default regression model at 512 QM9-shaped molecules (either tree)."""
    n = 512
    bmg = synth.random_batch(n, "qm9", seed=1)
    bmg.to(dev)
    y = torch.randn(n, 1, generator=torch.Generator().manual_seed(2)).to(dev)
    reg = cm.FusedTrainer(build(lambda d: cm.RegressionFFN(n_tasks=1, input_dim=d), dev), lr=1e-5)
    ev = build(lambda d: cm.RegressionFFN(n_tasks=1, input_dim=d), dev).eval()
    per = alternate({"regression step": lambda: reg.step(bmg, y), "regression predict": lambda: ev.predict(bmg)}, args)
    return dict(per, routes=[str(reg.last_route)])


def unchanged(args):
    trees = {"this tree": HERE, "parent": os.path.abspath(args.unchanged)}
    per = {k: {name: [] for name in PATHS} for k in trees}
    routes = {}
    for _ in range(args.rounds):
        for k, tree in trees.items():
            env = dict(os.environ, DMPNN_LIB=os.path.join(tree, "chemprop_amd", "libdmpnn_gfx950.so"))
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--tree", tree, "--steps", str(args.steps),
                                  "--warmup", str(args.warmup), "--groups", str(args.groups)], env=env, capture_output=True, text=True, check=True, timeout=300)
            r = json.loads(out.stdout.strip().splitlines()[-1])
            print(f"unchanged: {k} done", file=sys.stderr, flush=True)
            assert os.path.abspath(r["package"]).startswith(tree + os.sep), (r["package"], tree)
            routes[k] = r["routes"]
            for name in per[k]:
                per[k][name] += r[name]
    res = {k: {name: summary(v) for name, v in d.items()} for k, d in per.items()}
    for name in PATHS:
        a, b = res["this tree"][name], res["parent"][name]
        res[f"{name}: this tree - parent, us"] = round(a["us"] - b["us"], 1)
        res[f"{name}: inside the parent's spread"] = bool(abs(a["us"] - b["us"]) <= b["spread_us"])
    res["routes"] = routes
    if args.bench:
        res["bench.py headline"] = bench(args, trees)
    return res


def bench(args, trees):
    """`bench.py --gpus 1 --steps S --warmup W` in either tree, alternated: the value and ms_per_step of its one JSON result line."""
    per = {k: dict(value=[], ms_per_step=[]) for k in trees}
    for _ in range(args.rounds):
        for k, tree in trees.items():
            env = dict(os.environ, DMPNN_LIB=os.path.join(tree, "chemprop_amd", "libdmpnn_gfx950.so"))
            out = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", str(args.bench_steps), "--warmup", str(args.bench_warmup)],
                                 cwd=tree, env=env, capture_output=True, text=True, check=True, timeout=400)
            line = json.loads([l for l in out.stdout.strip().splitlines() if l.startswith("{")][-1])
            per[k]["value"].append(line["value"])
            per[k]["ms_per_step"].append(line["ms_per_step"])
            print(f"bench.py: {k} {line['value']}", file=sys.stderr, flush=True)
    res = {}
    for k, d in per.items():
        v, ms = sorted(d["value"]), sorted(d["ms_per_step"])
        res[k] = dict(value=v[len(v) // 2], value_runs=d["value"], value_spread=round(max(v) - min(v), 3), ms_per_step=ms[len(ms) // 2],
                      ms_per_step_runs=d["ms_per_step"])
    res["unit"] = "M edge-updates/s (higher is better)"
    res["this tree - parent"] = round(res["this tree"]["value"] - res["parent"]["value"], 3)
    res["inside the parent's spread"] = bool(abs(res["this tree - parent"]) <= res["parent"]["value_spread"])
    return res


def profile(args, dev):
    bmg = synth.random_batch(512, "qm9", seed=1)
    bmg.to(dev)
    T = targets(512, dev)
    fused = cm.FusedTrainer(build(mcc_pred, dev), lr=1e-5)
    run(lambda: fused.step(bmg, T), args.warmup)
    print(json.dumps(dict(profile_steps=args.profile_steps, us=round(run(lambda: fused.step(bmg, T), args.profile_steps), 1))))


def main():
    args = ARGS
    dev = torch.device("cuda:0")
    if args.child:
        import chemprop_amd

        print(json.dumps(dict(unchanged_child(args, dev), package=os.path.dirname(chemprop_amd.__file__))))
        return
    if args.profile_steps:
        profile(args, dev)
        return
    out = dict(steps=args.steps, warmup=args.warmup, groups=args.groups, device=torch.cuda.get_device_name(dev), mcc=mcc(args, dev))
    if args.unchanged:
        torch.cuda.synchronize()
        out["unchanged"] = dict(rounds=args.rounds, **unchanged(args))
    print(json.dumps(out))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
