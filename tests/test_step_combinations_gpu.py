"""Every case of the pairwise grid (``tests/step_harness.py``: 82 cases, every valid pair of settings of the one-call training
step) on the GPU: three ``FusedTrainer.step`` calls — the first two inside the validation window on the full plan, the third on the
plan the steady state uses (the tile plan where the batch takes the tile kernels) — each held to the float64 restatement of the
whole step.  Teacher forcing: before every step the reference is loaded with the device model's CURRENT float32 parameters and
running statistics, so every step's loss, predictions, gradients and statistics meet float64 at the first-step bars and Adam's
amplification of rounding noise never enters; the parameters after each step are held to ``adam_replay`` — float64 Adam fed with the
gradients the device produced.  A quarter of the cases also run the staged step (forward | backward | ``opt.step``, forced on one
rank) on a copy: the same bits in every parameter after three steps.

Judged by ``step_harness.compare``: ``err = max|got - ref| / max|ref|`` within ``min(MARGIN max(e32, 2**-23), cap)``, caps 1e-5 (loss),
2e-5 (predictions, gradients), 1e-6 (running statistics), 2e-6 (parameters against ``adam_replay``); ``e32`` is the float32
restatement against the float64 one from the same parameters.  One ``STEPBAR`` line per tensor is printed before judging;
``profiles/step_combination_bars.txt`` holds, per case and step, the worst tensor's line and every tensor's ratio (the 6 570 full
lines are 750 KB).

MARGIN.  Measured on the MI355X over the 6 570 comparisons of the 82 cases: the worst ``err / max(e32, 2**-23)`` is 6.02 — the gradient
of the output layer's bias (``predictor.ffn.1.2.bias``) at step 3 of case 45 (bond, ReLU, mixed batch, shared two-component block,
Wasserstein, value clip: err 7.2e-7 against a float32 draw of 7.8e-8, floored at 2**-23), then 6.01 (the same tensor of case 24,
binary MCC) and 5.54 (case 64): sums over the batch of a few dozen terms, which the head's row kernels add in another order than
torch.  Doubled and rounded up to a power of two that is 16 = ``rows_harness.MARGIN``, which is used as it is.  No ratio is above 16.

What the grid found: ``k_adam`` forms ``1.f - beta2`` from the float32 0.999 while the host formed the bias correction from the
double (``optim.bias_corrections`` now forms both from the float32 betas; the regression test is at the end of this file).  Hand
mutations it was checked against (not committed): the gradient pointer of ``agg.W.weight`` moved by 16 bytes when attentive
aggregation and V_d are both set — caught by all ten such cases (03, 10, 17, 19, 34, 39, 47, 54, 56, 68: ``g.agg.W.weight`` off by
more than its size); ``weight_decay`` dropped from ``_optimizer_args`` — by all sixteen weight-decay cases (07, 11, 20, ...: every
``p.*`` off by 1e-2 at step 1); ``b_i`` handed over as NULL for a biased atom block — by all ten such cases (05, 27, 30, 31, 33, 43,
49, 55, 61, 67: loss, predictions and gradients at step 1)."""
import copy

import pytest
import torch

import rows_harness as rh
import step_harness as sh
from chemprop_amd import _lib

pytestmark = pytest.mark.gpu
MARGIN = rh.MARGIN
GRID = sh.grid()


def _expected_route(case, bmg, validate):
    """The route ``engine.train_route`` gives the block on this batch, with the cap ``FusedTrainer._block_plan`` puts on it (an atom
    block beyond the tile runs on the general route on the f16 pipe on demand)."""
    from chemprop_amd import engine

    n = len(bmg)
    nV, nE = int(bmg.V.shape[0]), int(bmg.E.shape[0])
    beyond = sh.beyond_the_tile(bmg)
    if case.block == "atom" and beyond:
        return "general16"
    info = engine.train_route(nV, nE, int(bmg.V.shape[1]), int(bmg.E.shape[1]), sh.D_H, case.depth, case.act, n, undirected=case.block == "undirected",
                              atom=case.block == "atom", have_batch=True, oversize=bmg.oversize, max_level=1 if beyond else 2)
    return _lib.ROUTES[info.route]


def _check_route(case, tr, bmgs, step):
    from chemprop_amd.data import merge_components

    on = [merge_components(bmgs)] if case.components == "2-shared" else bmgs
    want = [_expected_route(case, b, step < 2) for b in on]
    got = list(tr.last_route) if isinstance(tr.last_route, tuple) else [tr.last_route]
    assert [str(r).split("/")[0] for r in got] == want, (case.id, step, got, want)
    for r in got:
        r = str(r)
        if case.block == "undirected":
            assert r in ("general", "general16"), r
        elif case.graphs == "qm9":
            assert r.startswith("mega"), r   # the tile kernels
            if step == 2:
                assert tr._last_plan_tiles, "step 3 of a QM9-shaped batch runs on the tile plan"
        else:
            assert not r.startswith("mega"), r   # a per-step route


def _state(model):
    return {k: p.detach().cpu().clone() for k, p in model.named_parameters()}


def _run(case, model, inp, dev, tr, steps=sh.STEPS, observe=None):
    bmgs = [copy.deepcopy(b) for b in inp["bmgs"]]
    for b in bmgs:
        b.to(dev)
    to = lambda t: None if t is None else t.to(dev)
    T, w, lt, gt, X, V = (to(inp[k]) for k in ("T", "w", "lt", "gt", "X_d", "V_d"))
    for s in range(steps):
        before = observe(s) if observe else None
        out = tr.step(bmgs if case.n_comp > 1 else bmgs[0], T, w, lt, gt, X_d=X, V_d=V, **sh.step_kwargs(case, inp, s))
        torch.cuda.synchronize()
        if observe:
            observe(s, before, out, bmgs)


@pytest.mark.parametrize("case", GRID, ids=lambda c: c.id)
def test_three_steps_against_float64(case, gpu_device, monkeypatch):
    from chemprop_amd.model import FusedTrainer

    dev = gpu_device
    monkeypatch.delenv("DMPNN_FORCE_COLLECTIVE", raising=False)
    cpu_model, inp = sh.build(case)
    model = copy.deepcopy(cpu_model).to(dev).train()
    twin = copy.deepcopy(model) if case.staged else None
    tr = FusedTrainer(model, **sh.trainer_flags(case), **sh.optimizer_kwargs(case))
    names = [k for k, _ in model.named_parameters()]
    p0, dev_grads, fails = _state(model), [], []
    mirror = copy.deepcopy(cpu_model)

    def observe(s, before=None, out=None, bmgs=None):
        if out is None:   # before the step: the reference from the device's current parameters and running statistics
            mirror.load_state_dict({k: v.detach().cpu() for k, v in model.state_dict().items()})
            r64, r32 = sh.restate(mirror, case, inp, torch.float64), sh.restate(mirror, case, inp, torch.float32)
            if case.act in sh.KINKED:
                lo, delta = sh.kink_clearance(r64, r32)
                print(f"STEPKINK {case.id} step{s + 1} min|z|={lo:.3e} delta={delta:.3e}")
            nbt = int(model.bn.num_batches_tracked) if case.bn else None
            return r64, r32, nbt
        r64, r32, nbt = before
        _check_route(case, tr, inp["bmgs"], s)
        assert float(out[1]) == float(inp["T"].isfinite().sum())
        got = {"loss": out[:1].detach().cpu(), "preds": tr.preds.detach().cpu()}
        got.update({"g." + k: tr.sync.views[i].detach().cpu().clone() for i, k in enumerate(names)})
        if case.bn:
            got.update(running_mean=model.bn.running_mean.cpu(), running_var=model.bn.running_var.cpu())
            assert int(model.bn.num_batches_tracked) == nbt + 1
        assert set(got) == set(sh.tensor_names(r64)), set(got) ^ set(sh.tensor_names(r64))
        fails.extend(sh.compare(case.id, s + 1, got, r64, sh.yardstick(r64, r32), MARGIN, r64["scales"]))
        dev_grads.append({k: got["g." + k] for k in names})
        p64, p32 = sh.adam_replay(p0, dev_grads, case)[-1], sh.adam_replay(p0, dev_grads, case, torch.float32)[-1]
        now = _state(model)
        fails.extend(sh.compare(case.id, s + 1, {"p." + k: now[k] for k in names}, {"p." + k: p64[k] for k in names},
                                {"p." + k: sh._err(p32[k], p64[k])[0] for k in names}, MARGIN))

    assert len(list(tr.sync.params)) == len(names) and all(a is b for a, (_, b) in zip(tr.sync.params, model.named_parameters()))
    _run(case, model, inp, dev, tr, observe=observe)
    assert tr.opt.steps == sh.STEPS
    assert not fails, f"{case.id}: " + "; ".join(fails)
    if twin is None:
        return
    # the staged step on a copy: forward | backward as two calls, the clip and Adam in opt.step — the same bits
    monkeypatch.setenv("DMPNN_FORCE_COLLECTIVE", "1")
    tb = FusedTrainer(twin, **sh.trainer_flags(case), **sh.optimizer_kwargs(case))
    _run(case, twin, inp, dev, tb)
    assert tb.opt.steps == sh.STEPS
    for (k, a), (_, b) in zip(model.named_parameters(), twin.named_parameters()):
        assert torch.equal(a.detach().view(torch.int32), b.detach().view(torch.int32)), f"{case.id}: staged {k} differs from the one-call step"


def test_adam_on_a_scalar_parameter_near_1e_3_follows_float64_adam(gpu_device):
    """Regression, found by case 47 of the grid (``agg.W.bias`` = 7.8e-4 under weight decay): ``k_adam`` forms ``1.f - beta2`` from
    the float32 0.999 — 1.3e-5 off 1e-3 — while the host formed the bias correction from the double; ``v / (1 - beta2^k)`` was that
    far off, the update 6e-6 off wherever ``sqrt(v)`` is not small against ``eps``, and a parameter that is small against its own
    update left float64 Adam by 3e-6, 1.3e-5 and 3.5e-5 of its size over three steps.  ``optim.bias_corrections`` forms both from
    the float32 betas.  Three ``FlatAdam.step`` calls on four such parameters against ``torch.optim.Adam`` in float64, at the
    parameters' bar of this file: ``MARGIN 2**-23`` of ``max|p|``."""
    from chemprop_amd import distributed as ddp
    from chemprop_amd.optim import FlatAdam

    p = torch.nn.Parameter(torch.tensor([7.8e-4, -3.1e-4, 2.2e-3, 5.0e-4], device=gpu_device))
    sync = ddp.GradSync([p])
    opt = FlatAdam(sync, lr=sh.LR, betas=sh.BETAS, eps=sh.ADAM_EPS, weight_decay=sh.WEIGHT_DECAY)
    ref = torch.nn.Parameter(p.detach().cpu().double().clone())
    ropt = torch.optim.Adam([ref], lr=sh.LR, betas=sh.BETAS, eps=sh.ADAM_EPS, weight_decay=sh.WEIGHT_DECAY)
    g = torch.tensor([3.0e-9, -2.0e-5, 1.0e-4, -4.0e-5])
    for s in range(sh.STEPS):
        sync.zero_grad()
        sync.views[0].copy_((g * (1 + s)).to(gpu_device))
        opt.step()
        ref.grad = (g * (1 + s)).double()
        ropt.step()
        torch.cuda.synchronize()
        err, scale = sh._err(p.detach().cpu(), ref.detach())
        print(f"STEPBAR adam-scalar step{s + 1} p err={err:.3e} bar={MARGIN * sh.EPS32:.3e} maxref={scale:.3e}")
        assert err <= MARGIN * sh.EPS32, (s, err)
