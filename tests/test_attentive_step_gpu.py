"""AttentiveAggregation behind the block on the GPU: ``dmpnn_head`` in attentive mode against the float64 restatement, the one-call
step (``FusedTrainer(model, attentive=True)``) against float64 autograd of the whole model, against a module-path twin over three
steps, the staged step, and ``HipMPNN``.

Bars: the head at ``attn_harness``'s (32 times the float32 restatement's own error, floored at 2**-23, capped by the head's caps);
the step's loss 1e-5 and every gradient 2e-5 (unfloored: over ``max|ref|``); ``agg.W.bias``'s gradient — analytically zero — absolute,
``|gb| <= 32 * 2**-23 * sum_v |dl_v|``; the trajectory within 1e-4 of ``max(1, |ref|)`` and never on ``agg.W.bias``, whose steps follow
the sign of rounding noise.  The trajectory's twins run Adam with ``eps = 1e-4`` as tests/test_undirected_step_gpu.py does: with the
default 1e-8 an entry whose gradient is noise moves by a full ``lr`` per step in either implementation.  Every figure is printed
before it is judged.
"""
import copy
import types

import pytest
import torch

import attn_harness as ah
from chemprop_amd import _lib
from conftest import parity_err, parity_err_unfloored
from test_dropout_gpu import _restated_forward
from test_multicomponent_integration import stub_chemprop  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu
F = torch.nn.functional


# ---- 1. dmpnn_head in attentive mode --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ah.head_cases(), ids=lambda c: c.id)
def test_head_in_attentive_mode_against_float64(case, gpu_device):
    inp = ah.head_inputs(case)
    r64, e32 = ah.head_yardstick(case, inp)
    got = ah.run_head(case, inp, gpu_device)
    fails = ah.compare_head(case, got, r64, e32)
    assert not fails, fails


def test_head_attentive_workspace_is_what_the_library_asks_for(gpu_device):
    """One byte less than ``dmpnn_head_ws_bytes`` is refused (ENOSPC) and nothing is written."""
    import ctypes as C

    case = ah.head_case("ws", 8, 8)
    inp = ah.head_inputs(case)
    lib = _lib.load()
    seen = {}
    real = lib.dmpnn_head

    class _Lib:
        def __getattr__(self, name):
            return getattr(lib, name)

        def dmpnn_head(self, href, Hv, ld, st):
            h = href._obj
            h.ws_bytes -= 1
            seen["rc"] = real(href, Hv, ld, st)
            h.ws_bytes += 1
            return real(href, Hv, ld, st)

    load = _lib.load
    wrapped = _Lib()
    try:
        _lib.load = lambda: wrapped
        got = ah.run_head(case, inp, gpu_device)
    finally:
        _lib.load = load
    assert seen["rc"] == -3 and bool(torch.isfinite(got["preds"]).all())


# ---- 2. the one-call step against float64 autograd ------------------------------------------------------------------------------------
def _model(dev, d_h, act="relu", bn=True, d_vd=None, seed=21, hidden=32, **mp_kw):
    from chemprop_amd import agg as cagg
    from chemprop_amd.model import MPNN, RegressionFFN
    from chemprop_amd.nn import BondMessagePassing

    torch.manual_seed(seed)
    mp = BondMessagePassing(d_h=d_h, activation=act, d_vd=d_vd, **mp_kw)
    width = int(mp.output_dim)
    return MPNN(mp, cagg.AttentiveAggregation(output_size=width), RegressionFFN(n_tasks=2, input_dim=width, hidden_dim=hidden, activation="tanh"),
                batch_norm=bn).to(dev).train()


def _batch(dev, n, kind, seed=13, d_vd=None):
    from chemprop_amd import synth

    gen = torch.Generator().manual_seed(seed)
    cpu = synth.random_batch(n, kind, seed=seed)
    V = None if d_vd is None else torch.randn(int(cpu.V.shape[0]), d_vd, generator=gen)
    y = torch.randn(n, 2, generator=gen)
    bmg = synth.random_batch(n, kind, seed=seed)
    bmg.to(dev)
    return cpu, bmg, y, V


def _float64_step(before, cpu, y, V_d):
    """Loss and gradients of the whole model in float64 on the CPU: the restated block, ``oracle.agg_torch.attentive``, batch norm on
    batch statistics, the tanh predictor, the masked MSE.  Also ``sum_v |dl_v|`` of the attention (the scale of its bias gradient)."""
    from chemprop_amd.model import criterion_loss

    ref = copy.deepcopy(before).cpu().double()
    g = types.SimpleNamespace(V=cpu.V.double(), E=cpu.E.double(), edge_index=cpu.edge_index, rev_edge_index=cpu.rev_edge_index)
    Hv = _restated_forward(g, ref.message_passing, lambda x: x, None if V_d is None else V_d.double())
    Hv.retain_grad()
    n = int(cpu.batch.max()) + 1
    A = ah.attentive(Hv, cpu.batch, ref.agg.W.weight, ref.agg.W.bias, n)
    A.retain_grad()
    Z = A
    if isinstance(ref.bn, torch.nn.BatchNorm1d):
        Z = F.batch_norm(A, None, None, ref.bn.weight, ref.bn.bias, training=True, eps=ref.bn.eps)
    lin = [m for m in ref.predictor.ffn.modules() if isinstance(m, torch.nn.Linear)]
    P = Z
    for i, m in enumerate(lin):
        P = F.linear(torch.tanh(P) if i else P, m.weight, m.bias)
    loss = criterion_loss(ref.criterion, P, y.double())
    loss.backward()
    with torch.no_grad():
        s = F.linear(Hv, ref.agg.W.weight, ref.agg.W.bias).exp().reshape(-1)
        Zs = torch.zeros(n, dtype=torch.float64).index_add(0, cpu.batch, s)
        al = s / Zs[cpu.batch]
        a = (A.grad[cpu.batch] * Hv).sum(1)
        c = torch.zeros(n, dtype=torch.float64).index_add(0, cpu.batch, al * a)
        sum_abs_dl = float((al * (a - c[cpu.batch])).abs().sum())
    return float(loss), {k: p.grad for k, p in ref.named_parameters()}, sum_abs_dl


STEP_CASES = [
    # id, molecules, kind, model keywords, the routes the block may take
    ("qm9x64-relu-h64", 64, "qm9", dict(d_h=64, act="relu"), ("mega16",)),
    ("zincx12-relu-h64", 12, "zinc", dict(d_h=64, act="relu"), None),
    # (no batch norm in the two below.  Behind a softmax-weighted mean, batch norm makes the loss invariant to a uniform shift of H_v:
    #  sum_v gH_v = 0 column by column, so the gradient of every bias in front of the aggregation is a cancelling sum — W_d.bias's is
    #  exactly zero (float64 autograd: 9.7e-17), W_o.bias's a remainder of 4.6e-3 under weight gradients of 1.3e-1 — and an unfloored
    #  bar on such a tensor measures the cancellation, not the step.  Batch norm with the attention is held by the head sweep above, by
    #  the first two cases, by the twin and by HipMPNN below)
    ("zincx8-tanh-h400", 8, "zinc", dict(d_h=400, act="tanh", bn=False), ("general16",)),
    ("qm9x24-tanh-h32-vd5", 24, "qm9", dict(d_h=32, act="tanh", d_vd=5, bn=False), None),
]


def _one_step(cid, n, kind, kw, dev, env=None, monkeypatch=None):
    from chemprop_amd.model import FusedTrainer

    model = _model(dev, **kw)
    cpu, bmg, y, V = _batch(dev, n, kind, d_vd=kw.get("d_vd"))
    before = copy.deepcopy(model)
    tr = FusedTrainer(model, lr=1e-3, attentive=True)
    loss = tr.step(bmg, y.to(dev), V_d=None if V is None else V.to(dev))
    torch.cuda.synchronize()
    grads = {k: tr._views[id(p)].detach().cpu().clone() for k, p in model.named_parameters()}
    return tr, before, cpu, y, V, float(loss[0]), grads


@pytest.mark.parametrize("cid,n,kind,kw,routes", STEP_CASES, ids=[c[0] for c in STEP_CASES])
def test_one_call_step_against_float64_autograd(cid, n, kind, kw, routes, gpu_device, monkeypatch):
    """ONE step: the loss and every gradient in the flat buffer against float64 autograd of the whole model.  The ReLU blocks get no
    allowance for decisions at the kink here: the bars are held without one."""
    from chemprop_amd.model import FusedTrainer

    monkeypatch.setenv("DMPNN_VALIDATE", "never")   # (K0 inside the call from the first step on: the attention reads the table it wrote)
    with pytest.raises(NotImplementedError):
        FusedTrainer(_model(gpu_device, **kw), lr=1e-3)
    tr, before, cpu, y, V, loss, grads = _one_step(cid, n, kind, kw, gpu_device)
    print(f"ATTNSTEP {cid} route {tr.last_route} tiles-only plan {tr._last_plan_tiles}")
    if routes is not None:
        assert tr.last_route in routes, tr.last_route
    l64, g64, sum_abs_dl = _float64_step(before, cpu, y, V)
    print(f"ATTNSTEP {cid} loss {loss:.8f} float64 {l64:.8f}")
    errs = {}
    for k, g in g64.items():
        if k == "agg.W.bias":
            v, bar = abs(float(grads[k])), ah.MARGIN * ah.EPS32 * sum_abs_dl
            print(f"ATTNSTEP {cid} agg.W.bias |g|={v:.3e} bar={bar:.3e} (float64 autograd: {abs(float(g)):.3e})")
            assert v <= bar
            continue
        errs[k] = parity_err_unfloored(grads[k].numpy(), g.numpy())
        print(f"ATTNSTEP {cid} {k} err={errs[k]:.3e} max|ref|={float(g.abs().max()):.3e}")
    assert abs(loss - l64) <= 1e-5 * max(1.0, abs(l64)), (loss, l64)
    assert len(errs) + 1 == len(grads) and max(errs.values()) <= 2e-5, errs


def test_tile_route_takes_no_aggregate_ride(gpu_device, monkeypatch):
    """On the tile route the forward tile kernel must not write aggregates in attentive mode: the step's results do not depend on
    ``DMPNN_HEAD_AGG`` (the switch of the ride and of the fused aggregation), bit for bit."""
    monkeypatch.setenv("DMPNN_VALIDATE", "never")
    cid, n, kind, kw, _ = STEP_CASES[0]
    runs = {}
    for mode in (None, "tile", "fused", "split"):
        if mode is None:
            monkeypatch.delenv("DMPNN_HEAD_AGG", raising=False)
        else:
            monkeypatch.setenv("DMPNN_HEAD_AGG", mode)
        tr, *_, loss, grads = _one_step(cid, n, kind, kw, gpu_device)
        assert tr.last_route == "mega16" and tr._last_plan_tiles
        runs[mode] = (loss, grads)
    for mode in ("tile", "fused", "split"):
        assert runs[mode][0] == runs[None][0], mode
        for k, g in runs[None][1].items():
            assert torch.equal(g.view(torch.int32), runs[mode][1][k].view(torch.int32)), (mode, k)


# ---- 3. three steps against a module-path twin ----------------------------------------------------------------------------------------
def test_three_steps_against_a_module_path_twin(gpu_device):
    """``FusedTrainer(attentive=True).step`` three times against ``MPNN.loss(...).backward()`` + ``FlatAdam`` on a twin (the path this
    model took before): the losses, every parameter but ``agg.W.bias``, and the eval-mode predictions afterwards."""
    from chemprop_amd import distributed as ddp
    from chemprop_amd.model import FusedTrainer
    from chemprop_amd.optim import FlatAdam

    dev = gpu_device
    kw = dict(d_h=64, act="tanh")
    a = _model(dev, **kw)
    b = copy.deepcopy(a)
    tr = FusedTrainer(a, lr=1e-3, eps=1e-4, attentive=True)
    sync = ddp.GradSync(list(b.parameters()), modules=[b])
    opt = FlatAdam(sync, lr=1e-3, eps=1e-4)
    for i in range(3):
        _, bmg, y, _ = _batch(dev, 48, "qm9", seed=90 + i)
        y = y.to(dev)
        la = float(tr.step(bmg, y)[0])
        lb = b.loss(bmg, y)
        lb.backward()
        sync.allreduce()
        opt.step()
        sync.zero_grad()
        lb = float(lb)
        print(f"ATTNTWIN step {i}: fused {la:.8f} module {lb:.8f}")
        assert abs(la - lb) <= 1e-4 * max(1.0, abs(lb)), (i, la, lb)
    torch.cuda.synchronize()
    for (k, pa), (kb, pb) in zip(a.named_parameters(), b.named_parameters()):
        assert k == kb
        e = parity_err(pa.detach().cpu().numpy(), pb.detach().cpu().numpy())
        print(f"ATTNTWIN {k}: {e:.2e}" + ("  (not judged: its gradient is rounding noise)" if k == "agg.W.bias" else ""))
        if k != "agg.W.bias":
            assert e <= 1e-4, f"{k}: {e:.2e}"
    # (the bias shifts every logit of a molecule alike: the predictions do not see it)
    _, bmg, _, _ = _batch(dev, 48, "qm9", seed=99)
    a.eval(), b.eval()
    with torch.no_grad():
        pa, pb = a(bmg).cpu().numpy(), b(bmg).cpu().numpy()
    e = parity_err(pa, pb)
    print(f"ATTNTWIN eval predictions: {e:.2e}")
    assert e <= 1e-4


# ---- 4. the staged step ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid,n,kind,kw,routes", [STEP_CASES[2], STEP_CASES[3]], ids=[STEP_CASES[2][0], STEP_CASES[3][0]])
def test_staged_step_equals_the_one_call_step_bit_for_bit(cid, n, kind, kw, routes, gpu_device, monkeypatch):
    """forward | backward | update as three calls (the data-parallel form, forced on one rank) against the one-call step: the same
    bits in the loss and in every parameter after three steps — the attention's gradients are final after the forward stage."""
    from chemprop_amd.model import FusedTrainer

    dev = gpu_device
    a = _model(dev, **kw)
    b = copy.deepcopy(a)
    _, bmg, y, V = _batch(dev, n, kind, d_vd=kw.get("d_vd"))
    y, V = y.to(dev), (None if V is None else V.to(dev))
    ta = FusedTrainer(a, lr=1e-3, attentive=True)
    la = [float(ta.step(bmg, y, V_d=V)[0]) for _ in range(3)]
    monkeypatch.setenv("DMPNN_FORCE_COLLECTIVE", "1")
    tb = FusedTrainer(b, lr=1e-3, attentive=True)
    lb = [float(tb.step(bmg, y, V_d=V)[0]) for _ in range(3)]
    torch.cuda.synchronize()
    print(f"ATTNSTAGED {cid} route {ta.last_route}: one call {la} staged {lb}")
    assert la == lb
    for (k, pa), (_, pb) in zip(a.named_parameters(), b.named_parameters()):
        assert torch.equal(pa.detach().view(torch.int32), pb.detach().view(torch.int32)), k


# ---- 5. HipMPNN -----------------------------------------------------------------------------------------------------------------------
def test_hip_mpnn_takes_an_attentive_model_on_the_fused_step(stub_chemprop, gpu_device):  # noqa: F811
    from chemprop_amd.model import RegressionFFN

    S = stub_chemprop
    integ = S.integration
    integ.enable()
    HipM = integ.hip_mpnn_class()[1]
    torch.manual_seed(3)
    mp = S.mods["chemprop.nn"].BondMessagePassing(d_h=64)
    agg = S.mods["chemprop.nn"].agg.AttentiveAggregation(output_size=64)
    model = HipM(mp, agg, RegressionFFN(input_dim=64), batch_norm=True, init_lr=1e-3).to(gpu_device).train()
    st = model._hip_state()
    assert st["fused"] is not None and st["why"] is None, st["why"]
    opt = model.configure_optimizers()["optimizer"]
    model._trainer = types.SimpleNamespace(optimizers=[opt], accumulate_grad_batches=1, gradient_clip_val=None, gradient_clip_algorithm=None,
                                           strategy=None)
    _, bmg, y, _ = _batch(gpu_device, 24, "qm9")
    y = y[:, :1].contiguous().to(gpu_device)
    before = {k: p.detach().clone() for k, p in model.named_parameters()}
    opt.step(lambda: model.training_step((bmg, None, None, y, None, None, None), 0))
    torch.cuda.synchronize()
    assert model.__dict__["_hip"]["route"].startswith("fused:"), model.__dict__["_hip"]
    for k in ("message_passing.W_h.weight", "agg.W.weight", "predictor.ffn.0.0.weight"):
        if k in before:
            assert not torch.equal(dict(model.named_parameters())[k].detach(), before[k]), k
    assert not torch.equal(model.agg.W.weight.detach(), before["agg.W.weight"])
