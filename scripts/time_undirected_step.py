"""One training step of a regression model with UNDIRECTED messages (`chemprop train --undirected`: BondMessagePassing(undirected=True),
d_h 300, depth 3, norm aggregation, batch norm, one hidden layer of 300, MSE, ReLU), with and without dropout in the block:

  fused         FusedTrainer(undirected=True, rows_dropout=True).step: K0, the block, the head, backward, Adam — one call, on the
                per-step general route on the f16 pipe (p > 0: DMPNN_F_UNDIRECTED_MASK)
  module path   MPNN.loss(...).backward() + FlatAdam.step: what such a model trained on before — the block through its own autograd
                node (p = 0), else the chain of row kernels with torch's tau and nn.Dropout between them

at 512 QM9-shaped and at 512 ZINC-shaped molecules, p = 0 and p = 0.2.  Per shape the configurations are warmed, then timed
ALTERNATELY in one process: `groups` rounds, in each round K steps of every configuration between two device synchronisations; per
configuration the per-step time of every round, their median and their spread (max - min).
`--module-only` times the module path alone and `--bond-only` the default DIRECTED bond model's p = 0 step (no keyword of this change
is used); with `--root DIR` the package is imported from another checkout, which is how both are timed on the parent commit.
`--message-only` launches the undirected message step (`dmpnn_message_fwd`, DMPNN_F_UNDIRECTED, tau none and ReLU on load) `--steps`
times per shape on an aligned [n_edges, 300] input and times nothing itself: it is what a `rocprofv3 --kernel-trace --stats` run
wraps — this tree runs the hot builds k_segment<4, 0, 1, none | relu>, the parent commit (`--root`) the generic build <4, 0, -1, -1>.
`--kernel-csv FILE` reads that run's kernel trace (csv) and writes, per k_segment build and grid size (= shape), the mean / min / max
duration of the last `--steps` launches to `--out`.
`--combine DIR` gathers the results (DIR/step.json, parent_module.json, kernel_this.json, kernel_parent_{1,2}.json, headline.json and,
per visit N, vN_this_bond_*.json / vN_parent_bond_*.json, as far as they exist) into `--out` (profiles/undirected_step.json).
usage: python scripts/time_undirected_step.py [--steps K] [--warmup W] [--groups G] [--module-only | --bond-only | --message-only]
                                              [--root DIR] [--out file.json] [--kernel-csv FILE] [--combine DIR]"""
import argparse
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


def _load(d, name):
    p = os.path.join(d, name)
    return json.load(open(p)) if os.path.isfile(p) else None


def combine(d, out_path):
    step = _load(d, "step.json")
    out = dict(script="scripts/time_undirected_step.py", steps=step["steps"], warmup=step["warmup"], groups=step["groups"], device=step["device"],
               results=step["results"])
    r, sp = step["results"], {}
    pm = _load(d, "parent_module.json")
    for n, kind in SHAPES:
        for p in ("0", f"{P:g}"):
            f, m = r[f"fused, p {p}, {n} {kind} mols"], r[f"module path, p {p}, {n} {kind} mols"]
            e = dict(fused_us=f["us_per_step"], fused_spread_us=f["spread_us"], module_us=m["us_per_step"], module_spread_us=m["spread_us"],
                     speedup=round(m["us_per_step"] / f["us_per_step"], 2), route=f["route"])
            if pm:
                q = pm["results"][f"module path, p {p}, {n} {kind} mols"]
                e.update(parent_module_us=q["us_per_step"], parent_module_spread_us=q["spread_us"],
                         speedup_against_parent_module=round(q["us_per_step"] / f["us_per_step"], 2))
            sp[f"p {p}, {n} {kind} mols"] = e
    out["fused_against_module_path"] = sp
    if pm:
        out["parent_module_path"] = pm["results"]
    # the kernel time of the undirected message step: the hot builds (this tree) against the generic build (the parent commit, two runs)
    kt, kp = _load(d, "kernel_this.json"), [k for k in (_load(d, "kernel_parent_1.json"), _load(d, "kernel_parent_2.json")) if k]
    if kt and kp:
        out["undirected_message_kernel"] = dict(
            method="rocprofv3 --kernel-trace --stats, one run per library; per kernel the mean duration over its launches, in ns",
            hot_builds=kt, generic_build_runs=kp)
    # the directed guard: the default bond model's step and the headline against the parent commit, alternating processes; one entry
    # per visit (v1_..., v2_...: a visit is one GPU call, its processes in the order of their numbers, this tree and the parent in turn)
    import glob

    visits = sorted({os.path.basename(p).split("_")[0] for p in glob.glob(os.path.join(d, "v*_this_bond_*.json"))})
    guard = {}
    for v in visits:
        tb = [json.load(open(p)) for p in sorted(glob.glob(os.path.join(d, f"{v}_this_bond_*.json")))]
        pb = [json.load(open(p)) for p in sorted(glob.glob(os.path.join(d, f"{v}_parent_bond_*.json")))]
        bond = {}
        for k in tb[0]["results"]:
            pg = [x for q in pb for x in q["results"][k]["groups_us"]]
            tm = [t["results"][k]["us_per_step"] for t in tb]
            bond[k] = dict(this_tree_us=tm, this_tree_groups_us=[t["results"][k]["groups_us"] for t in tb],
                           parent_us=[q["results"][k]["us_per_step"] for q in pb], parent_groups_us=[q["results"][k]["groups_us"] for q in pb],
                           parent_groups_min_max_us=[min(pg), max(pg)], within_parent_spread=[bool(min(pg) <= t <= max(pg)) for t in tm])
        guard[v] = bond
    if guard:
        out["directed_bond_step_against_parent"] = guard
    hl = _load(d, "headline.json")
    if hl:
        out["headline_against_parent"] = hl
    with open(out_path, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps({k: out[k] for k in out if k not in ("results", "parent_module_path")}))


def kernel_csv(path, steps, warmup, out_path):
    """Per (k_segment build, grid size = shape): the durations of a `rocprofv3 --kernel-trace` csv's launches, in ns, in the runs of
    `warmup + steps` launches `--message-only` makes (warm-up dropped).  A hot build has one run per shape (its activation is in its
    name); the generic build two: `#0` tau none, `#1` ReLU on load."""
    import csv

    rows = {}
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            name = r.get("Kernel_Name") or r.get("Name") or ""
            if "k_segment" not in name:
                continue
            grid = r.get("Grid_Size") or r.get("Grid_Size_X") or "?"
            t0, t1 = int(r.get("Start_Timestamp") or r["Begin_Timestamp"]), int(r["End_Timestamp"])
            rows.setdefault((name[name.index("k_segment"):], str(grid)), []).append((t0, t1 - t0))
    res, n = {}, warmup + steps
    for (name, grid), v in sorted(rows.items()):
        v = [x[1] for x in sorted(v)]
        for i in range(0, len(v), n):
            d = v[i:i + n][warmup:]
            if d:
                res[f"{name} grid {grid} #{i // n}"] = dict(launches=len(d), mean_ns=round(sum(d) / len(d), 1), min_ns=min(d), max_ns=max(d))
    print(json.dumps(res))
    if out_path:
        with open(out_path, "w") as f:
            json.dump(res, f, indent=1)


def message_only(args, lib, engine, synth):
    """The undirected message step alone, `--steps` launches per shape and activation (for a kernel trace)."""
    dev = torch.device("cuda:0")
    for n, kind in SHAPES:
        bmg = synth.random_batch(n, kind, seed=1)
        bmg.to(dev)
        plan = engine.GraphPlan.from_bmg(bmg)
        nE, h = int(bmg.E.shape[0]), 300
        H = torch.randn(nE, h, device=dev)
        M = torch.empty(nE, h, device=dev)
        for act in (0, 1):   # (DMPNN_ACT_NONE, DMPNN_ACT_RELU)
            with engine._OnDevice(dev):
                for _ in range(args.warmup + args.steps):
                    rc = lib.dmpnn_message_fwd(plan.buf.data_ptr(), plan.n_atoms, plan.n_edges, h, H.data_ptr(), h, M.data_ptr(), h, act, 0.0, None,
                                               1, engine._stream_ptr(dev))
                    assert rc == 0, lib.dmpnn_last_error_string()
            torch.cuda.synchronize()
        print(f"message-only: {n} {kind} molecules, {nE} edges: {2 * (args.warmup + args.steps)} launches")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--groups", type=int, default=5)
    ap.add_argument("--module-only", action="store_true")
    ap.add_argument("--bond-only", action="store_true")
    ap.add_argument("--message-only", action="store_true")
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--out", default=None)
    ap.add_argument("--combine", default=None, metavar="DIR")
    ap.add_argument("--kernel-csv", default=None, metavar="FILE")
    args = ap.parse_args()
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if args.combine:
        return combine(args.combine, args.out or os.path.join(here, "profiles", "undirected_step.json"))
    if args.kernel_csv:
        return kernel_csv(args.kernel_csv, args.steps, args.warmup, args.out)
    sys.path.insert(0, os.path.abspath(args.root))
    from chemprop_amd import _lib, engine, synth
    from chemprop_amd import agg as cagg
    from chemprop_amd import distributed as ddp
    from chemprop_amd.model import MPNN, FusedTrainer, RegressionFFN
    from chemprop_amd.nn import BondMessagePassing
    from chemprop_amd.optim import FlatAdam

    if args.message_only:
        return message_only(args, _lib.load(), engine, synth)
    dev = torch.device("cuda:0")

    def model(p, undirected):
        torch.manual_seed(0)
        mp = BondMessagePassing(dropout=p, undirected=undirected)
        return MPNN(mp, cagg.NormAggregation(), RegressionFFN(n_tasks=1, input_dim=mp.output_dim), batch_norm=True).to(dev).train()

    res = {}
    for n, kind in SHAPES:
        bmg = synth.random_batch(n, kind, seed=1)
        bmg.to(dev)
        y = torch.randn(n, 1, generator=torch.Generator().manual_seed(2)).to(dev)
        configs, routes, syncs = {}, {}, []
        if args.bond_only:
            t0 = FusedTrainer(model(0.0, False), lr=1e-5)
            configs["bond model, fused, p 0"] = lambda t0=t0: t0.step(bmg, y)
            routes["bond model, fused, p 0"] = lambda t0=t0: str(t0.last_route)
        else:
            for p in (0.0, P):
                if not args.module_only:
                    tr = FusedTrainer(model(p, True), lr=1e-5, rows_dropout=True, undirected=True)
                    configs[f"fused, p {p:g}"] = lambda tr=tr: tr.step(bmg, y)
                    routes[f"fused, p {p:g}"] = lambda tr=tr: str(tr.last_route)
                m = model(p, True)
                sync = ddp.GradSync(list(m.parameters()), modules=[m])
                opt = FlatAdam(sync, lr=1e-5)
                syncs.append(sync)

                def module_step(m=m, sync=sync, opt=opt):   # (what integration.HipMPNN.training_step runs where the fused step refuses)
                    with ddp.backward_on_calling_thread():
                        sync.zero_grad()
                        m.loss(bmg, y).backward()
                    sync.allreduce()
                    opt.step()

                configs[f"module path, p {p:g}"] = module_step
                routes[f"module path, p {p:g}"] = lambda m=m: "module:" + str(m.message_passing.__dict__.get("_dmpnn_route"))
        for step in configs.values():
            run(step, args.warmup)
        per = {k: [] for k in configs}
        for _ in range(args.groups):
            for k, step in configs.items():
                per[k].append(run(step, args.steps))
        for s in syncs:
            s.wait()
        for k, v in per.items():
            res[f"{k}, {n} {kind} mols"] = dict(us_per_step=round(sorted(v)[len(v) // 2], 1), groups_us=[round(x, 1) for x in v],
                                               spread_us=round(max(v) - min(v), 1), route=routes[k](), n_atoms=int(bmg.V.shape[0]),
                                               n_edges=int(bmg.E.shape[0]))
    out = dict(steps=args.steps, warmup=args.warmup, groups=args.groups,
               device=torch.cuda.get_device_name(dev), results=res)
    print(json.dumps(out))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
