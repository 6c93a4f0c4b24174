"""What the input gradients cost on the per-step general route: (a) ``dmpnn_backward`` alone, (b) ``dmpnn_backward_inputs`` with
``gV`` + ``gE`` (``k_input_grad_v`` for ``gV``), (c) the same two gradients composed from the entries the library already had (``gather_rows`` + ``aggregate`` + two
``linear`` on pre-transposed weights, over stand-ins of ``G0`` / ``GO`` of the same shapes).

512 ZINC-shaped and 512 QM9-shaped synthetic molecules, ``d_h`` 300, depth 3.  The three are ALTERNATED within every round (a, b,
c, a, b, c, ...), each timed as wall-clock per call over ``--calls`` calls between two device synchronisations; the result is the
median over ``--rounds`` rounds with the spread (min .. max).  Writes one JSON document (``--out``, default
``profiles/input_grad.json``)."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import torch  # noqa: E402

from chemprop_amd import _lib, engine, synth  # noqa: E402
from chemprop_amd.nn import BondMessagePassing  # noqa: E402


def workload(kind, n_mols, d_h, depth, dev):
    bmg = synth.random_batch(n_mols, kind, seed=1)
    bmg.to(dev)
    torch.manual_seed(0)
    mp = BondMessagePassing(d_v=int(bmg.V.shape[1]), d_e=int(bmg.E.shape[1]), d_h=d_h, depth=depth).to(dev)
    plan = engine.GraphPlan.from_bmg(bmg)
    out, st = engine.forward(plan, bmg.V, bmg.E, mp.W_i.weight, mp.W_h.weight, mp.W_o.weight, mp.W_o.bias, depth=depth, act="relu",
                             keep=True, route="general")
    gout = torch.randn_like(out)
    need = dict(W_i=True, W_h=True, W_o=True, b_o=True)
    lib = _lib.load()
    grads, b, refs = engine.backward(st, gout, need, launch=False)
    a = _lib.BwdInputsArgs()
    a.b = b
    nb = int(lib.dmpnn_backward_inputs_ws_bytes(C.byref(st.args)))
    ws = torch.empty(nb // 4 + 1, dtype=torch.float32, device=dev)
    a.b.ws, a.b.ws_bytes = ws.data_ptr(), nb
    nV, nE, d_v, d_e = plan.n_atoms, plan.n_edges, int(bmg.V.shape[1]), int(bmg.E.shape[1])
    gV, gE = torch.empty(nV, d_v, device=dev), torch.empty(nE, d_e, device=dev)
    a.gV, a.ldgv, a.gE, a.ldge = gV.data_ptr(), d_v, gE.data_ptr(), d_e
    stream = engine._stream_ptr(dev)
    # (c): stand-ins of the two tensors the backward pass leaves in its workspace, and the transposed weight slices made beforehand
    ldh = int(st.args.ldh)
    G0, GO = torch.randn(nE, ldh, device=dev)[:, :d_h], torch.randn(nV, ldh, device=dev)[:, :d_h]
    Wt_v = torch.cat((mp.W_o.weight[:, :d_v].t(), mp.W_i.weight[:, :d_v].t()), 1).contiguous()     # [d_v, 2 d_h]
    Wt_e = mp.W_i.weight[:, d_v:].t().contiguous()                                                  # [d_e, d_h]
    R, S = torch.empty(nE, d_h, device=dev), torch.empty(nV, d_h, device=dev)

    def run_a():
        _lib.check(lib.dmpnn_backward(C.byref(b), stream), "dmpnn_backward")

    def run_b():
        _lib.check(lib.dmpnn_backward_inputs(C.byref(a), stream), "dmpnn_backward_inputs")

    def run_c():
        engine.gather_rows(G0, plan.rev32, out=R)
        engine.aggregate(plan, R, out=S)
        engine.linear(GO, Wt_v, A2=S, out=gV, mfma="split16")
        engine.linear(G0, Wt_e, out=gE, mfma="split16")

    keep = (bmg, mp, plan, out, st, gout, grads, refs, ws, gV, gE, G0, GO, Wt_v, Wt_e, R, S)
    return dict(a=run_a, b=run_b, c=run_c), dict(n_atoms=nV, n_edges=nE, d_v=d_v, d_e=d_e, route=st.route), keep


def timed(fn, calls):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / calls * 1e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mols", type=int, default=512)
    ap.add_argument("--d-h", type=int, default=300)
    ap.add_argument("--depth", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "input_grad.json"))
    args = ap.parse_args()
    dev = torch.device("cuda")
    doc = dict(what="wall-clock us per call, median over rounds (min .. max); a: dmpnn_backward, b: dmpnn_backward_inputs (gV + gE), "
                    "c: gV + gE composed from gather_rows + aggregate + two linear (f16 pipe) on stand-in tensors",
               device=torch.cuda.get_device_name(0), mols=args.mols, d_h=args.d_h, depth=args.depth, rounds=args.rounds, calls=args.calls, workloads={})
    for kind in ("zinc", "qm9"):
        runs, shape, keep = workload(kind, args.mols, args.d_h, args.depth, dev)
        with engine._OnDevice(dev):
            for fn in runs.values():     # warm-up
                timed(fn, 5)
            t = {k: [] for k in runs}
            for _ in range(args.rounds):
                for k, fn in runs.items():   # alternated: a, b, c within every round
                    t[k].append(timed(fn, args.calls))
        res = {k: dict(median=round(statistics.median(v), 2), min=round(min(v), 2), max=round(max(v), 2)) for k, v in t.items()}
        extra = [tb - ta for ta, tb in zip(t["a"], t["b"])]
        res["b_minus_a"] = dict(median=round(statistics.median(extra), 2), min=round(min(extra), 2), max=round(max(extra), 2))
        doc["workloads"][kind] = dict(shape=shape, us=res)
        print(kind, json.dumps(dict(shape=shape, us=res)))
        del keep
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
