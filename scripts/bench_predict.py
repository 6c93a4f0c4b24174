#!/usr/bin/env python
"""Inference behind the block: ``MPNN.predict`` (ONE ``dmpnn_predict_head`` call) against the module path ``model(bmg, X_d=...)``.

One process, ``model.eval()`` under ``torch.no_grad()``, every shape warmed up first.  The two paths ALTERNATE in blocks of
``--calls`` calls, ``--reps`` repetitions each; a block is timed by the host clock with one device synchronise at each end.  Reported
per path: the median block with min..max, in microseconds per call.  The tail alone — everything behind the block on a fixed
``H_v`` — is timed the same way by HIP events.  A speed-up is claimed only where the medians differ by more than the larger of the
two spreads (``max - min``); the JSON says which.

Writes ``profiles/predict_head.json`` (``--out``).  Needs a HIP device: there is nothing to measure without one.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def build_model(name: str, d_h: int, depth: int, dev):
    import torch

    from chemprop_amd import agg as cagg
    from chemprop_amd.model import MPNN, BinaryClassificationFFN, MveFFN, RegressionFFN
    from chemprop_amd.nn import BondMessagePassing

    torch.manual_seed(0)
    d_xd = 200 if name == "mve_xd200" else 0
    ffn = dict(input_dim=d_h + d_xd, hidden_dim=300, n_layers=1)
    pred = {"regression": lambda: RegressionFFN(n_tasks=1, **ffn), "binary12": lambda: BinaryClassificationFFN(n_tasks=12, **ffn),
            "mve_xd200": lambda: MveFFN(n_tasks=1, **ffn)}[name]()
    model = MPNN(BondMessagePassing(d_h=d_h, depth=depth), cagg.NormAggregation(), pred, batch_norm=True).to(dev).eval()
    with torch.no_grad():
        model.bn.running_mean.uniform_(-0.1, 0.1), model.bn.running_var.uniform_(0.5, 2.0)
    return model, d_xd


def summary(us: list) -> dict:
    return dict(median=round(statistics.median(us), 2), min=round(min(us), 2), max=round(max(us), 2))


def alternate(fa, fb, calls: int, reps: int, events: bool) -> tuple:
    """``reps`` blocks of ``calls`` calls of ``fa`` and of ``fb``, alternating; microseconds per call of every block."""
    import torch

    out = ([], [])
    for _ in range(reps):
        for f, acc in ((fa, out[0]), (fb, out[1])):
            torch.cuda.synchronize()
            if events:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(calls):
                    f()
                e1.record()
                torch.cuda.synchronize()
                acc.append(e0.elapsed_time(e1) * 1e3 / calls)
            else:
                t0 = time.perf_counter()
                for _ in range(calls):
                    f()
                torch.cuda.synchronize()
                acc.append((time.perf_counter() - t0) * 1e6 / calls)
    return out


def verdict(a: dict, b: dict) -> dict:
    """``a``: the fused path, ``b``: the module path."""
    spread = max(a["max"] - a["min"], b["max"] - b["min"])
    diff = b["median"] - a["median"]
    return dict(module_over_predict=round(b["median"] / a["median"], 3), difference_us=round(diff, 2), larger_spread_us=round(spread, 2),
                claim="faster" if diff > spread else ("slower" if -diff > spread else "no difference beyond the spread"))


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--mols", type=int, default=512)
    ap.add_argument("--hidden", type=int, default=300)
    ap.add_argument("--depth", type=int, default=3)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "predict_head.json"))
    args = ap.parse_args()

    import torch

    if not torch.cuda.is_available():
        print("bench_predict: no HIP device — nothing is measured without one", file=sys.stderr)
        return 2
    from chemprop_amd import _lib, synth
    from chemprop_amd.predict import fused_predict

    lib = _lib.load()
    dev = torch.device("cuda:0")
    results = []
    with torch.no_grad():
        for kind in ("qm9", "zinc"):
            bmg = synth.random_batch(args.mols, kind, seed=1000)
            bmg.to(dev)
            for name in ("regression", "binary12", "mve_xd200"):
                model, d_xd = build_model(name, args.hidden, args.depth, dev)
                X_d = torch.randn(args.mols, d_xd, generator=torch.Generator().manual_seed(1)).to(dev) if d_xd else None
                fused = lambda: model.predict(bmg, X_d=X_d)
                module = lambda: model(bmg, X_d=X_d)
                for _ in range(2):   # (the first call also splits the hidden layer's weight: the steady call is the second)
                    assert fused_predict(model, bmg, X_d=X_d) is not None, "the inference head refused the benchmark's model"
                launches = int(lib.dmpnn_last_launch_count())
                for _ in range(args.warmup):
                    fused(), module()
                a, b = fused(), module()
                torch.cuda.synchronize()
                rel = float((a - b).abs().max() / b.abs().max())
                whole = [summary(x) for x in alternate(fused, module, args.calls, args.reps, events=False)]
                # the tail alone: the block's output fixed, everything behind it timed by device events
                Hv = model.message_passing(bmg)
                model.message_passing.forward = lambda bmg, V_d=None, _Hv=Hv: _Hv
                try:
                    for _ in range(args.warmup):
                        fused(), module()
                    tail = [summary(x) for x in alternate(fused, module, args.calls, args.reps, events=True)]
                finally:
                    del model.message_passing.forward
                row = dict(model=name, molecules=kind, n_mols=args.mols, n_atoms=int(bmg.V.shape[0]), d_h=args.hidden, depth=args.depth, d_xd=d_xd,
                           head_launches=launches, max_rel_difference=rel,
                           predict_us=whole[0], module_us=whole[1], whole=verdict(whole[0], whole[1]),
                           tail_predict_us=tail[0], tail_module_us=tail[1], tail=verdict(tail[0], tail[1]))
                results.append(row)
                print(json.dumps(row), flush=True)
    out = dict(tool="scripts/bench_predict.py", device=torch.cuda.get_device_name(0), calls_per_block=args.calls, blocks_per_path=args.reps,
               clock="host clock, one synchronise at each end of a block (whole); HIP events (tail)", unit="microseconds per call", results=results)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(f"wrote {args.out}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
