#!/usr/bin/env python
"""One validation step behind the block (depth 3, d_h 300, norm aggregation, batch norm, one hidden layer of 300 —
``scripts/bench_predict.py``'s models): the default regression model and a 12-task binary head at 512 QM9-shaped and 512 ZINC-shaped
molecules, three calls:

  (a) predict with targets   ``fused_predict(model, bmg, targets=T)``: predictions and ``val_loss`` — what both trees have
  (b) validate               ``MPNN.validate(bmg, T, stats)``: (a) and the batch's metric sums added into ``stats`` in the same C call
  (c) predict + torch sums   (a), then the same sums formed with plain torch ops written here and added into a device buffer: what a
                             caller of ``fused_predict`` does today

The protocol is ``scripts/bench_predict.py``'s (``alternate`` / ``summary`` / ``verdict`` are imported from it): one process, eval mode
under ``torch.no_grad()``, every shape warmed first, two calls ALTERNATED in blocks of ``--calls`` calls, ``--reps`` blocks each —
(a) against (b), then (b) against (c) — a block timed by the host clock with one device synchronise at each end; per call the median
block with min..max in microseconds.  The stage's cost is reported as median (b) - median (a).

``--parent TREE``: (a) on the tree at TREE as well (a built checkout of the parent commit), each tree in a process of its own (one
process cannot hold two builds of the package), the trees alternated ``--rounds`` times.  A difference is claimed only by ``verdict``'s
rule: the medians differ by more than the larger of the two spreads.

``--kernel-stats CSV``: the ``*_kernel_stats.csv`` of a separate ``rocprofv3 --kernel-trace --stats -- python scripts/time_validate_step.py
--profile`` run; the rows of the stage's kernels (``k_metric_*``) are copied into the result.  Without it the result says "not measured".

Writes ``profiles/validate_step.json`` (``--out``).  Needs a HIP device: there is nothing to measure without one."""
from __future__ import annotations

import argparse
import csv
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_predict import alternate, summary, verdict  # noqa: E402  (the protocol: not copied)

SHAPES = ((512, "qm9"), (512, "zinc"))
MODELS = ("regression", "binary12")
CALLS = ("predict with targets", "validate", "predict + torch sums")
D_H, DEPTH = 300, 3


def torch_sums(name: str, preds, T, buf) -> None:
    """The statistics of ``chemprop_amd.metrics`` formed from ``preds`` with plain torch ops (float64), added into ``buf``."""
    import torch

    m = T.isfinite()
    md = m.double()
    if name == "regression":
        y = torch.where(m, T, torch.zeros_like(T)).double()
        e = torch.where(m, preds.double() - y, torch.zeros_like(y))
        cols = (md, e * e, e.abs(), y, y * y, e * e, e.abs())   # (no bounds in this run: the bounded sums are the plain ones)
    else:
        pp, tp = preds > 0.5, T > 0.5
        cols = (md, (m & pp & tp).double(), (m & pp & ~tp).double(), (m & ~pp & ~tp).double(), (m & ~pp & tp).double())
    buf[:, :len(cols)] += torch.stack([c.sum(0) for c in cols], 1)


def measure(args) -> dict:
    """The calls of every model on the package that ``sys.path`` leads to: microseconds per call of every block."""
    import torch

    import chemprop_amd
    from bench_predict import build_model
    from chemprop_amd import _lib, synth
    from chemprop_amd.predict import fused_predict

    lib = _lib.load()
    dev = torch.device("cuda:0")
    res = dict(package=os.path.dirname(chemprop_amd.__file__), device=torch.cuda.get_device_name(0), models={})
    with torch.no_grad():
        for n, kind in SHAPES:
            bmg = synth.random_batch(n, kind, seed=1000)
            bmg.to(dev)
            for name in MODELS:
                model, _ = build_model(name, D_H, DEPTH, dev)
                t = model.predictor.n_tasks
                gen = torch.Generator().manual_seed(2)
                T = torch.randn(n, t, generator=gen) if name == "regression" else torch.rand(n, t, generator=gen).round()
                T[torch.rand(n, t, generator=gen) < 0.1] = float("nan")
                T = T.to(dev)
                have = hasattr(model, "validate")   # (the parent tree has no MPNN.validate: (a) alone)
                buf = torch.zeros(t, 8, dtype=torch.float64, device=dev)

                def predict_t():
                    return fused_predict(model, bmg, targets=T)

                def today():
                    r = fused_predict(model, bmg, targets=T)
                    torch_sums(name, r.preds, T, buf)
                    return r

                row = {"n_atoms": int(bmg.V.shape[0])}
                assert predict_t() is not None and predict_t() is not None, "the inference head must take these models"
                row["launches, predict with targets"] = int(lib.dmpnn_last_launch_count())
                if have:
                    from chemprop_amd.metrics import MetricStats

                    stats = MetricStats.for_model(model)

                    def validate():
                        return model.validate(bmg, T, stats)

                    validate()
                    row["launches, validate"] = int(lib.dmpnn_last_launch_count())
                    # the two ways to the statistics agree (the body; the torch sums keep no header)
                    stats.reset(), buf.zero_()
                    validate(), today()
                    torch.cuda.synchronize()
                    a, b = stats.stats[4:].view(t, 8).cpu(), buf.cpu()
                    row["max |validate - torch sums| / max |torch sums|"] = float((a - b).abs().max() / b.abs().max())
                if args.profile:   # (under rocprofv3: a few steady calls of (b), nothing timed)
                    for _ in range(args.calls if have else 0):
                        validate()
                    torch.cuda.synchronize()
                    res["models"][f"{name}, {n} {kind} mols"] = row
                    continue
                for _ in range(args.warmup):
                    predict_t(), today()
                    if have:
                        validate()
                torch.cuda.synchronize()
                if have:
                    ab = alternate(predict_t, validate, args.calls, args.reps, events=False)
                    bc = alternate(validate, today, args.calls, args.reps, events=False)
                    row.update({CALLS[0]: ab[0], CALLS[1]: ab[1] + bc[0], CALLS[2]: bc[1]})
                else:
                    aa = alternate(predict_t, predict_t, args.calls, args.reps, events=False)
                    row[CALLS[0]] = aa[0] + aa[1]
                res["models"][f"{name}, {n} {kind} mols"] = row
    return res


def child(tree: str, args) -> dict:
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--tree", tree, "--calls", str(args.calls), "--reps", str(args.reps),
                          "--warmup", str(args.warmup)], env=dict(os.environ, DMPNN_LIB=os.path.join(tree, "chemprop_amd", "libdmpnn_gfx950.so")),
                         capture_output=True, text=True, timeout=600)
    if out.returncode != 0:
        raise SystemExit(f"time_validate_step: the process on {tree} failed ({out.returncode})\n{out.stderr[-2000:]}")
    r = json.loads(out.stdout.strip().splitlines()[-1])
    assert os.path.abspath(r["package"]).startswith(os.path.abspath(tree) + os.sep), (r["package"], tree)
    return r


def kernel_rows(path: str) -> list:
    """The rows of a rocprofv3 kernel-stats CSV whose kernel is one of the stage's."""
    with open(path, newline="") as f:
        return [r for r in csv.DictReader(f) if "k_metric_" in (r.get("Name") or r.get("KernelName") or "")]


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit")
    ap.add_argument("--kernel-stats", default=None, help="the kernel-stats CSV of a separate rocprofv3 run of --profile")
    ap.add_argument("--profile", action="store_true", help="run --calls steady validate calls per model and exit (for rocprofv3)")
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "validate_step.json"))
    ap.add_argument("--tree", default=HERE, help=argparse.SUPPRESS)   # (the child processes: the package to import)
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child or args.profile:
        sys.path.insert(0, os.path.abspath(args.tree))
        import torch

        if not torch.cuda.is_available():
            print("time_validate_step: no HIP device — nothing is measured without one", file=sys.stderr)
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
        per = {call: summary([us for r in runs["this tree"] for us in r["models"][model][call]]) for call in CALLS}
        row.update(per)
        row["stage cost (validate - predict with targets), us"] = round(per[CALLS[1]]["median"] - per[CALLS[0]]["median"], 2)
        row["validate against predict + torch sums"] = verdict(per[CALLS[1]], per[CALLS[2]])   # (verdict(a, b): b over a)
        if args.parent:
            parent = summary([us for r in runs["parent"] for us in r["models"][model][CALLS[0]]])
            row["predict with targets on the parent"] = parent
            row["predict with targets against the parent"] = verdict(per[CALLS[0]], parent)
        results[model] = row
        print(json.dumps({model: row}), flush=True)
    stage = kernel_rows(args.kernel_stats) if args.kernel_stats else "not measured"
    out = dict(tool="scripts/time_validate_step.py", device=runs["this tree"][0]["device"], calls_per_block=args.calls, blocks_per_call=args.reps,
               rounds=args.rounds, clock="host clock, one synchronise at each end of a block", unit="microseconds per call",
               verdict="module_over_predict = the second call's median over the first's; a claim only beyond the larger of the two spreads (max - min)",
               stage_kernels_rocprofv3=stage, results=results)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(f"wrote {args.out}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
