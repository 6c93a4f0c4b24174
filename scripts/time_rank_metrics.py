#!/usr/bin/env python
"""Epoch ROC-AUC / PRC-AUC of a binary head (``chemprop_amd.metrics.RankStats``): what the append costs a validation step, and the epoch's
end against the route a caller has without it.  The 12-task binary head of ``scripts/bench_predict.py`` (depth 3, d_h 300, norm
aggregation, batch norm, one hidden layer of 300) at 512 QM9-shaped and 512 ZINC-shaped molecules.

  steps   (a) ``MPNN.validate(bmg, T, stats)`` and (b) the same call with ``ranks=`` (the buffer reset every call), ALTERNATED in blocks of
          ``--calls`` calls, ``--reps`` blocks each, a block timed by the host clock with one device synchronise at each end
          (``bench_predict.alternate``); the append's cost is median (b) - median (a).  ``--parent TREE``: (a) on a built checkout of the
          parent commit as well, each tree in a process of its own, the trees alternated ``--rounds`` times; a difference is claimed only
          beyond the larger of the two spreads (``bench_predict.verdict``).
  epoch   ``rows`` in {1 024, 8 192, 32 768, 131 072} x 12 tasks, scores with 10 % missing targets appended in batches of 512:
          ``RankStats.compute()`` (one C call, one copy of 8 (t + 1) doubles) against the route a caller has today — the per-batch
          predictions kept in a list, ``torch.cat``, and per task ``torch.sort`` + ``cumsum`` + trapezoid in float64 on the device (this
          script's restatement of torchmetrics' ``_binary_clf_curve`` / ``roc`` / ``precision_recall_curve``; torchmetrics is not
          installed), one copy of the results — with and without the pooled column where ``RANK_MAX_ROWS`` allows.  The two routes
          must agree within ``(n_ranked + 8) 2^-52`` (asserted: the tests' bar).  Each timing: ``--epoch-reps`` calls, median with min..max
          in microseconds, every call ended by its copy to the host.

``--kernel-stats CSV``: the ``*_kernel_stats.csv`` of a separate ``rocprofv3 --kernel-trace --stats -- python scripts/time_rank_metrics.py
--profile`` run (8 192 rows: appends of 512 and ``compute()``, nothing timed); the rows of ``k_rank_*`` are copied into the result.

Writes ``profiles/rank_metrics.json`` (``--out``).  Needs a HIP device: there is nothing to measure without one."""
from __future__ import annotations

import argparse
import csv
import json
import os
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_predict import alternate, summary, verdict  # noqa: E402  (the protocol: not copied)

SHAPES = ((512, "qm9"), (512, "zinc"))
ROWS = (1024, 8192, 32768, 131072)
TASKS, BATCH = 12, 512
D_H, DEPTH = 300, 3
CALLS = ("validate", "validate with ranks")


def sort_route(P, T, pooled: bool):
    """ROC-AUC and PRC-AUC per task (and of all pairs as one column) by sort + cumsum + trapezoid in float64 on the device: ``[t (+ 1),
    2]`` on the host."""
    import torch

    def column(s, y):
        ok = y.isfinite() & s.isfinite()
        s, y = s[ok].double(), (y[ok] > 0.5)
        nan = torch.full((2,), float("nan"), dtype=torch.float64, device=s.device)
        if s.numel() == 0:
            return nan
        s, order = torch.sort(s, descending=True, stable=True)
        y = y[order]
        idx = torch.cat((torch.nonzero(s[1:] != s[:-1]).reshape(-1), torch.tensor([s.numel() - 1], device=s.device)))
        tps = torch.cumsum(y.long(), 0)[idx].double()   # (exact: counts below 2^53)
        fps = (1 + idx).double() - tps
        Pn, Nn = tps[-1], fps[-1]
        zero = torch.zeros(1, dtype=torch.float64, device=s.device)
        tpr, fpr = torch.cat((zero, tps / Pn)), torch.cat((zero, fps / Nn))
        roc = ((fpr[1:] - fpr[:-1]) * (tpr[1:] + tpr[:-1]) * 0.5).sum()
        prec, rec = torch.cat((zero + 1, tps / (tps + fps))), torch.cat((zero, tps / Pn))
        prc = ((rec[1:] - rec[:-1]) * (prec[1:] + prec[:-1]) * 0.5).sum()
        return torch.where((Pn > 0) & (Nn > 0), torch.stack((roc, prc)), nan)

    cols = [column(P[:, j], T[:, j]) for j in range(P.shape[1])]
    if pooled:
        cols.append(column(P.reshape(-1), T.reshape(-1)))
    return torch.stack(cols).cpu().numpy()


def timed(f, reps: int) -> dict:
    import torch

    us = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        f()
        torch.cuda.synchronize()
        us.append((time.perf_counter() - t0) * 1e6)
    return summary(us)


def measure_steps(args) -> dict:
    import torch

    import chemprop_amd
    from bench_predict import build_model
    from chemprop_amd import _lib, synth
    from chemprop_amd.metrics import MetricStats

    try:
        from chemprop_amd.metrics import RankStats
    except ImportError:   # (the parent tree: (a) alone)
        RankStats = None
    lib, dev = _lib.load(), torch.device("cuda:0")
    res = dict(package=os.path.dirname(chemprop_amd.__file__), device=torch.cuda.get_device_name(0), shapes={})
    with torch.no_grad():
        for n, kind in SHAPES:
            bmg = synth.random_batch(n, kind, seed=1000)
            bmg.to(dev)
            model, _ = build_model("binary12", D_H, DEPTH, dev)
            gen = torch.Generator().manual_seed(2)
            T = torch.rand(n, TASKS, generator=gen).round()
            T[torch.rand(n, TASKS, generator=gen) < 0.1] = float("nan")
            T = T.to(dev)
            stats = MetricStats.for_model(model)

            def validate():
                return model.validate(bmg, T, stats)

            validate(), validate()
            row = {"n_atoms": int(bmg.V.shape[0]), "launches, validate": int(lib.dmpnn_last_launch_count())}
            if RankStats is not None:
                ranks = RankStats.for_model(model, capacity=n)

                def ranked():
                    ranks.rows = 0
                    return model.validate(bmg, T, stats, ranks=ranks)

                ranked()
                row["launches, validate with ranks"] = int(lib.dmpnn_last_launch_count())
            for _ in range(args.warmup):
                validate()
                if RankStats is not None:
                    ranked()
            torch.cuda.synchronize()
            if RankStats is not None:
                ab = alternate(validate, ranked, args.calls, args.reps, events=False)
                row.update({CALLS[0]: ab[0], CALLS[1]: ab[1]})
            else:
                aa = alternate(validate, validate, args.calls, args.reps, events=False)
                row[CALLS[0]] = aa[0] + aa[1]
            res["shapes"][f"binary12, {n} {kind} mols"] = row
    return res


def epoch_inputs(rows: int, dev):
    import torch

    gen = torch.Generator().manual_seed(rows)
    T = torch.rand(rows, TASKS, generator=gen).round()
    P = torch.sigmoid(torch.randn(rows, TASKS, generator=gen) + (T - 0.5))   # (scores that say something about the label)
    T[torch.rand(rows, TASKS, generator=gen) < 0.1] = float("nan")
    return [(P[a:a + BATCH].to(dev), T[a:a + BATCH].to(dev)) for a in range(0, rows, BATCH)]


def measure_epoch(args) -> dict:
    import numpy as np
    import torch

    from chemprop_amd import _lib
    from chemprop_amd.metrics import RankStats

    dev, out = torch.device("cuda:0"), {}
    for rows in ((8192,) if args.profile else ROWS):
        batches = epoch_inputs(rows, dev)
        ranks = RankStats(TASKS, rows, device=dev)
        for p, t in batches:
            ranks.update(p, t)
        pooled_ok = rows * TASKS <= _lib.RANK_MAX_ROWS
        if args.profile:
            for _ in range(5):
                ranks.compute(pooled=pooled_ok)
            continue
        row = {"pooled column": "inside RANK_MAX_ROWS" if pooled_ok else f"{rows * TASKS} keys: beyond RANK_MAX_ROWS, not ranked"}
        for pooled in ((False, True) if pooled_ok else (False,)):
            def sorted_today():
                return sort_route(torch.cat([p for p, _ in batches]), torch.cat([t for _, t in batches]), pooled)

            got, want = ranks.compute(pooled=pooled), sorted_today()
            mine = np.stack([np.append(got["per_task"]["roc"], got["roc-pooled"]) if pooled else got["per_task"]["roc"],
                             np.append(got["per_task"]["prc"], got["prc-pooled"]) if pooled else got["per_task"]["prc"]], 1)
            n_ranked = np.append(got["per_task"]["n_pos"] + got["per_task"]["n_neg"], rows * TASKS)[:mine.shape[0]]
            err = np.abs(mine - want).max(1)
            assert np.all(err <= (n_ranked + 8) * 2.0 ** -52), (rows, pooled, err.tolist())
            tag = "with the pooled column" if pooled else "per task"
            ranks.compute(pooled=pooled), sorted_today()
            reps = args.epoch_reps if rows <= 32768 else max(3, args.epoch_reps // 3)
            a, b = timed(lambda: ranks.compute(pooled=pooled), reps), timed(sorted_today, reps)
            row[f"RankStats.compute, {tag}"] = a
            row[f"cat + sort + cumsum, {tag}"] = b
            row[f"sort route over compute, {tag}"] = round(b["median"] / a["median"], 3)
            row[f"max |compute - sort route|, {tag}"] = float(err.max())
        out[f"{rows} rows x {TASKS} tasks"] = row
        print(json.dumps({f"{rows} rows": row}), file=sys.stderr, flush=True)
    return out


def child(tree: str, args) -> dict:
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--tree", tree, "--calls", str(args.calls), "--reps", str(args.reps),
                          "--warmup", str(args.warmup)], env=dict(os.environ, DMPNN_LIB=os.path.join(tree, "chemprop_amd", "libdmpnn_gfx950.so")),
                         capture_output=True, text=True, timeout=600)
    if out.returncode != 0:
        raise SystemExit(f"time_rank_metrics: the process on {tree} failed ({out.returncode})\n{out.stderr[-2000:]}")
    r = json.loads(out.stdout.strip().splitlines()[-1])
    assert os.path.abspath(r["package"]).startswith(os.path.abspath(tree) + os.sep), (r["package"], tree)
    return r


def kernel_rows(path: str) -> list:
    with open(path, newline="") as f:
        return [r for r in csv.DictReader(f) if "k_rank_" in (r.get("Name") or r.get("KernelName") or "")]


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--epoch-reps", type=int, default=9)
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit")
    ap.add_argument("--kernel-stats", default=None, help="the kernel-stats CSV of a separate rocprofv3 run of --profile")
    ap.add_argument("--profile", action="store_true", help="appends and compute() at 8 192 rows, nothing timed (for rocprofv3)")
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "rank_metrics.json"))
    ap.add_argument("--tree", default=HERE, help=argparse.SUPPRESS)   # (the child processes: the package to import)
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child or args.profile:
        sys.path.insert(0, os.path.abspath(args.tree))
        import torch

        if not torch.cuda.is_available():
            print("time_rank_metrics: no HIP device — nothing is measured without one", file=sys.stderr)
            return 2
        print(json.dumps(measure_epoch(args) if args.profile else measure_steps(args)))
        return 0
    trees = {"this tree": HERE}
    if args.parent:
        trees["parent"] = os.path.abspath(args.parent)
    runs = {k: [] for k in trees}
    for _ in range(args.rounds):   # (every tree in a process of its own, the trees alternated)
        for k, tree in trees.items():
            runs[k].append(child(tree, args))
    steps = {}
    for shape in runs["this tree"][0]["shapes"]:
        row = {k: v for k, v in runs["this tree"][0]["shapes"][shape].items() if k not in CALLS}
        per = {call: summary([us for r in runs["this tree"] for us in r["shapes"][shape][call]]) for call in CALLS}
        row.update(per)
        row["append cost (validate with ranks - validate), us"] = round(per[CALLS[1]]["median"] - per[CALLS[0]]["median"], 2)
        row["validate with ranks against validate"] = verdict(per[CALLS[0]], per[CALLS[1]])
        if args.parent:
            parent = summary([us for r in runs["parent"] for us in r["shapes"][shape][CALLS[0]]])
            row["validate on the parent"] = parent
            row["validate against the parent"] = verdict(per[CALLS[0]], parent)
        steps[shape] = row
        print(json.dumps({shape: row}), flush=True)
    sys.path.insert(0, HERE)
    epoch = measure_epoch(args)
    crossover = [k for k, r in epoch.items() if r.get("sort route over compute, per task", 2.0) < 1.0]
    out = dict(tool="scripts/time_rank_metrics.py", device=runs["this tree"][0]["device"], calls_per_block=args.calls, blocks_per_call=args.reps,
               rounds=args.rounds, clock="host clock, one synchronise at each end of a block / call", unit="microseconds per call",
               verdict="module_over_predict = the second call's median over the first's; a claim only beyond the larger of the two spreads (max - min)",
               rank_kernels_rocprofv3=kernel_rows(args.kernel_stats) if args.kernel_stats else "not measured", steps=steps, epoch=epoch,
               sort_route_faster_per_task_at=crossover or "nowhere within the rows measured")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(f"wrote {args.out}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
