"""How many launches one ``dmpnn_head`` / ``dmpnn_predict_head`` call makes on each route of the head's host driver
(``csrc/dmpnn_head.hip``; its kernels: ``csrc/dmpnn_head_kernels.hpp``).  No parity test can see an extra or a lost launch: this one can.

``dmpnn_head``: the difference of ``dmpnn_last_launch_count()`` around ONE call made through ``head_harness.run_case`` (the attentive
case through ``attn_harness.run_head``, which wraps it; the dropout cases set ``ffn_dropout_p`` the same way).
``dmpnn_predict_head`` resets the counter on entry, so the counter behind the call IS the call's count (``predict_harness.Call.launches``)
— taken once with the weights' split image still to be made (``wsplit_ready = 0``) and once with it ready.

The counter counts the library's launch sites, not the device's launches: the two launches of the row kernel share one site and the
column kernel's site counts where its launch is skipped, so a figure here can differ from a profiler's by one.  It is compared with
itself only.

The expected figures are literal.  They were printed by this very module — ``pytest -s`` prints a ``LAUNCHES <case> <count>`` line per
case before it judges — run on an MI355X against the library built from the commit BEFORE the host driver was split into stages;
that run's lines are ``profiles/head_launch_counts.txt``.  Never refresh them from the code under test.

Shapes: ``d_h = 64``, one hidden layer of 36, 2 tasks, MSE, tanh, mean aggregation, batch norm, unless the case says otherwise.
"""
import pytest
import torch

import attn_harness as ah
import head_harness as hh
import predict_harness as ph
from chemprop_amd import _lib


def _case(cid, form="default", B=100, d_h=64, hidden=(36,), tasks=2, **kw):
    kw.setdefault("act", "tanh")
    return hh.HeadCase(cid, form, B, d_h, hidden, tasks, **kw)


# (case, ffn_dropout_p, launch sites counted at the parent commit)
HEAD = [
    (_case("rows-B100", "rows"), 0.0, 6),                # the four-launch form, the aggregation inside the column kernel
    (_case("rows-B600", "rows", B=600), 0.0, 7),         # ... the aggregation in front of it (beyond 512 molecules)
    (_case("cols-B100", tasks=5), 0.0, 15),              # 5 outputs: the column kernels around the chain's predictor
    (_case("chain-B100", "chain"), 0.0, 12),             # DMPNN_HEAD=chain
    (_case("default-B1100", B=1100), 0.0, 14),           # the chain by size (beyond 1 024 molecules)
    (_case("d30-B100", d_h=30), 0.0, 12),                # d_h % 4 != 0: no column kernels
    (_case("layers1-B100", hidden=()), 0.0, 5),
    (_case("layers3-B100", hidden=(36, 36)), 0.0, 16),
    (_case("xd4-B100", d_xd=4), 0.0, 6),                 # molecule descriptors (dims[0] = 68)
    (_case("no-bn-B100", bn=False), 0.0, 6),
    (_case("dropout-rows-B100", "rows"), 0.25, 6),       # predictor dropout: inside the row kernel
    (_case("dropout-chain-B100", "chain"), 0.25, 13),    # ... a kernel of its own behind each hidden layer
]
ATTENTIVE = (ah.head_case("attentive-B100", 100, 64, hidden=(36,)), 9)
# (case, launch sites with wsplit_ready = 0, with wsplit_ready = 1)
PREDICT = [
    (ph.PredictCase("predict-B100", B=100, d_h=64, hidden=(36,), tasks=2, act="tanh"), 4, 3),     # the column kernel finds the bounds itself: no table
    (ph.PredictCase("predict-B2049", B=2049, d_h=64, hidden=(36,), tasks=2, act="tanh"), 6, 5),   # beyond the column kernels: the bounds table, the chain's front
]


def _with_dropout(run, p):
    """``run()`` with ``ffn_dropout_p = p`` set on the finished argument block (at ``dmpnn_head_ws_bytes``, its first use: the way
    ``attn_harness.run_head`` sets the attention's fields)."""
    lib = _lib.load()

    class _Lib:
        def __getattr__(self, name):
            return getattr(lib, name)

        def dmpnn_head_ws_bytes(self, href):
            href._obj.ffn_dropout_p, href._obj.ffn_dropout_seed = p, 7
            return lib.dmpnn_head_ws_bytes(href)

    load = _lib.load
    try:
        _lib.load = lambda: _Lib()
        return run()
    finally:
        _lib.load = load


def _count(run):
    lib = _lib.load()
    n0 = int(lib.dmpnn_last_launch_count())
    out = run()
    return int(lib.dmpnn_last_launch_count()) - n0, out


@pytest.mark.gpu
@pytest.mark.parametrize("case,p,expected", HEAD, ids=[c[0].id for c in HEAD])
def test_head_launch_count(case, p, expected, gpu_device):
    inp = hh.build_inputs(case)
    run = lambda: hh.run_case(case, inp, gpu_device)
    n, out = _count((lambda: _with_dropout(run, p)) if p else run)
    print(f"LAUNCHES {case.id} {n}")
    assert bool(torch.isfinite(out["loss"])) and bool(torch.isfinite(out["gHv"]).all()), case.id   # (the call did run)
    assert n == expected, (case.id, n, expected)


@pytest.mark.gpu
def test_attentive_head_launch_count(gpu_device):
    case, expected = ATTENTIVE
    inp = ah.head_inputs(case)
    n, out = _count(lambda: ah.run_head(case, inp, gpu_device))
    print(f"LAUNCHES {case.id} {n}")
    assert bool(torch.isfinite(out["loss"])) and bool(torch.isfinite(out["gHv"]).all()) and bool(torch.isfinite(out["g_att_W"]).all())
    assert n == expected, (case.id, n, expected)


@pytest.mark.gpu
@pytest.mark.parametrize("case,first,ready", PREDICT, ids=[c[0].id for c in PREDICT])
def test_predict_head_launch_count(case, first, ready, gpu_device):
    call = ph.Call(case, ph.build_inputs(case), gpu_device)
    got = []
    for r in (0, 1):
        out = call.run(ready=r)
        got.append(call.launches)
        assert bool(torch.isfinite(out["preds"]).all()), (case.id, r)
    print(f"LAUNCHES {case.id} {got[0]} {got[1]}")
    assert got == [first, ready], (case.id, got, [first, ready])
