"""A SELU predictor (``dmpnn_head_args.act = DMPNN_ACT_SELU``) through ``dmpnn_head`` in its forms — the row form, the chain, the
chain's one-launch output layer (``k_out_all``), its two-launch one (``k_out_bwd``: a criterion with several values per task) and the
generic layer backward (``k_head_act_bwd``: more than four outputs, several hidden layers) — with and without the predictor's
dropout, and through ``dmpnn_predict_head`` on the same shapes: the smallest cases of ``tests/test_head_boundaries.py``,
``tests/test_head_dropout.py`` and ``tests/test_predict_head_gpu.py`` with the activation replaced.

The harnesses' references call ``head_harness._act`` by module attribute (``predict_harness`` holds its own name for it): this file
extends both with ``"selu"`` -> ``F.selu`` at run time (``monkeypatch``).  Every case asserts that its float64 hidden pre-activations
are at least a quarter negative and a quarter positive.

Judged by the suite's rule with ``rows_harness.MARGIN``: ``err = max|got - ref| / max|ref|`` against float64 within ``min(MARGIN max(e32,
2**-23), cap)``, ``e32`` the float32 restatement's error, the caps of ``head_harness.CAP``; one ``HEADBAR`` / ``PREDBAR`` / ``SELUBAR``
line per tensor printed before judging.  Measured on the MI355X (253 comparisons): the worst ``err / max(e32, 2**-23)`` is 2.56 —
``gHv`` of ``chain-selu-mse-out-all`` (err 3.1e-7 against a float32 draw of 8.2e-8) — then 2.45 (``g_bn_bias`` of the row form and of the default
dispatch on the same shape) and 2.23 (the row form against the chain); ``tests/test_head_boundaries.py`` saw 8.39 on its own shapes, so the
rows' margin of 16 holds here with room."""
import pytest
import torch
import torch.nn.functional as F

import head_harness as hh
import predict_harness as ph
import rows_harness as rh
import test_head_dropout as thd
from conftest import parity_err_unfloored
from head_harness import HeadCase

pytestmark = pytest.mark.gpu
MARGIN = rh.MARGIN

_ORIG_ACT = hh._act


def _act(name, x):
    return F.selu(x) if name == "selu" else _ORIG_ACT(name, x)


@pytest.fixture(autouse=True)
def _selu_in_the_harnesses(monkeypatch):
    monkeypatch.setattr(hh, "_act", _act)
    monkeypatch.setattr(ph, "_act", _act)


def _spread(zs, case_id):
    assert zs, case_id
    for z in zs:
        n = z.numel()
        assert int((z < 0).sum()) * 4 >= n and int((z > 0).sum()) * 4 >= n, case_id


def _case(form, name, B=100, d_h=64, hidden=(36,), tasks=2, **kw):
    return HeadCase(f"{form}-selu-{name}", form, B, d_h, tuple(hidden), tasks, act="selu", **kw)


HEAD = [
    _case("rows", "mse"), _case("rows", "mae-bounded-sum", kind="mae", bounded=True, agg="sum"), _case("rows", "bce-nobn", kind="bce", bn=False, agg="norm"),
    _case("chain", "mse-out-all"), _case("default", "mse"),
    _case("chain", "mve-out-bwd", kind="mve"), _case("chain", "evidential-t1", kind="evidential", tasks=1, agg="norm"),
    _case("chain", "ce3", kind="ce", n_classes=3),
    _case("chain", "out5-generic", tasks=5), _case("default", "out5-cols", tasks=5),
    _case("chain", "layers3", hidden=(36, 20)), _case("default", "layers4-out5", hidden=(36, 20, 12), tasks=5),
    _case("chain", "xd3", d_xd=3),
    _case("default", "infer", mode="infer"), _case("chain", "eval-loss", mode="eval-loss"),
]


@pytest.mark.parametrize("case", HEAD, ids=lambda c: c.id)
def test_selu_head(case, gpu_device):
    inp = hh.build_inputs(case)
    ref, e32 = hh.yardstick(case, inp)
    _spread(ref["z"], case.id)
    got = hh.run_case(case, inp, gpu_device)
    fails = hh.compare(case, got, ref, e32, MARGIN)
    assert not fails, f"{case.id}: " + "; ".join(fails)


def test_selu_head_forms_agree(gpu_device):
    """The row form and the chain on one shape: every output within the bar of the float32 yardstick of each other."""
    case = HEAD[0]
    inp = hh.build_inputs(case)
    ref, e32 = hh.yardstick(case, inp)
    a = hh.run_case(case, inp, gpu_device)
    b = hh.run_case(case, inp, gpu_device, env=dict(DMPNN_HEAD="chain"))
    import dataclasses

    fails = hh.compare(dataclasses.replace(case, id=case.id + "/rows-vs-chain"), a, {k: v.double() for k, v in b.items() if torch.is_tensor(v)}, e32, MARGIN)
    assert not fails, "; ".join(fails)


# ---- with the predictor's dropout: the hash masks replayed ---------------------------------------------------------------------------
# (DMPNN_HEAD, n_components, molecules, d_h, hidden, tasks, ffn n_layers, criterion, activation, p)
DROP = {
    "rows-100-mse-selu-0.25": ("rows", 1, 100, 64, 36, 2, 1, "mse", "selu", 0.25),
    "chain-100-mse-selu-0.25": ("chain", 1, 100, 64, 36, 2, 1, "mse", "selu", 0.25),
    "chain-100-mve-selu-2-layers-0.5": ("chain", 1, 100, 64, 36, 1, 2, "mve", "selu", 0.5),
    "chain-100-ce-selu-0.1": ("chain", 1, 100, 64, 36, 2, 2, "ce", "selu", 0.1),
}


def _restate(model, Hvs, batches, n, T, w, seed, p, dtype):
    """``test_head_dropout.restate`` in ``dtype``: the head op by op on the CPU with the predictor's masks replayed -> the named
    tensors (``loss``, ``preds``, ``gHv``, every parameter gradient by its name in the model) and the hidden pre-activations."""
    from chemprop_amd.model import MODES, HeadSpec, masked_loss

    spec = HeadSpec(model, ffn_dropout=True)
    f = lambda t: t.detach().cpu().to(dtype)
    mode = {v: k for k, v in MODES.items()}[spec.agg_mode]
    names = {id(q): k for k, q in model.named_parameters()}
    (b,) = batches
    b = b.cpu()
    Hv = f(Hvs[0]).requires_grad_()
    H = torch.zeros(n, Hv.shape[1], dtype=dtype).index_add(0, b, Hv)
    if mode == "mean":
        H = H / torch.bincount(b, minlength=n).clamp(min=1).to(dtype).view(-1, 1)
    elif mode == "norm":
        H = H / spec.agg_norm
    leaves = {}
    if spec.bn is not None:
        bw, bb = f(spec.bn.weight).requires_grad_(), f(spec.bn.bias).requires_grad_()
        H = F.batch_norm(H, f(spec.bn.running_mean).clone(), f(spec.bn.running_var).clone(), bw, bb, training=True, momentum=spec.bn.momentum, eps=spec.bn.eps)
        leaves[names[id(spec.bn.weight)]], leaves[names[id(spec.bn.bias)]] = bw, bb
    Z, zs = H, []
    for i, blk in enumerate(model.predictor.ffn):
        lin = blk[-1]
        if i > 0:
            zs.append(Z.detach())
            Z = F.selu(Z) * (torch.from_numpy(thd.ffn_keep(seed, i, n, Z.shape[1], p)).to(dtype) / (1.0 - p))
        W, bias = f(lin.weight).requires_grad_(), f(lin.bias).requires_grad_()
        leaves[names[id(lin.weight)]], leaves[names[id(lin.bias)]] = W, bias
        Z = F.linear(Z, W, bias)
    if spec.kind == "ce":
        P = Z.reshape(n, -1, spec.n_classes)
    elif spec.kind == "mve":
        mean, var = torch.chunk(Z, 2, 1)
        P = torch.stack((mean, F.softplus(var)), 2)
    else:
        P = Z
    loss = masked_loss(P, f(T), f(w), None, None, None, spec.kind)
    loss.backward()
    return dict(loss=loss.detach().reshape(1), preds=Z.detach(), gHv=Hv.grad, **{k: v.grad for k, v in leaves.items()}), zs


@pytest.mark.parametrize("name", list(DROP))
def test_selu_head_with_predictor_dropout_given_the_masks(name, gpu_device, monkeypatch):
    case = DROP[name]
    monkeypatch.setenv("DMPNN_HEAD", case[0])
    model, Hvs, batches, n, T, w = thd.case_inputs(case, gpu_device)
    assert type(model.predictor.ffn[1][0]) is torch.nn.SELU
    p, seed = case[-1], 0x5E1F0000 + 77 * len(name)
    ref, zs = _restate(model, Hvs, batches, n, T, w, seed, p, torch.float64)
    _spread(zs, name)
    r32, _ = _restate(model, Hvs, batches, n, T, w, seed, p, torch.float32)
    e32 = {k: parity_err_unfloored(r32[k].double().numpy(), ref[k].numpy()) for k in ref}
    loss, P, g, gH = thd.run_head(model, Hvs, batches, n, T, w, seed)
    got = dict(loss=torch.tensor([loss], dtype=torch.float64), preds=P, gHv=gH, **{k: g[id(q)] for k, q in model.named_parameters() if id(q) in g})
    assert set(got) == set(ref), set(got) ^ set(ref)
    fails = []
    for k in ref:   # the rule of head_harness.compare, for tensors named after the model's parameters
        x, r = got[k].double().reshape(-1), ref[k].double().reshape(-1)
        assert bool(torch.isfinite(x).all()), k
        err = parity_err_unfloored(x.numpy(), r.numpy())
        bar = min(MARGIN * max(e32[k], hh.EPS32), hh.CAP["loss" if k == "loss" else "preds" if k == "preds" else "grad"])
        print(f"SELUBAR {name} {k} err={err:.3e} e32={e32[k]:.3e} ratio={err / max(e32[k], hh.EPS32):.2f} bar={bar:.3e} maxref={float(r.abs().max()):.3e}")
        if not err <= bar:
            fails.append(f"{k}: err {err:.3e} > bar {bar:.3e}")
    assert not fails, f"{name}: " + "; ".join(fails)
    _, P2, _, _ = thd.run_head(model, Hvs, batches, n, T, w, seed + 1)
    assert not torch.equal(P, P2), "the mask is live: another seed, another result"


# ---- dmpnn_predict_head --------------------------------------------------------------------------------------------------------------
PC = ph.PredictCase
PREDICT = [PC(id="selu-B5", act="selu"), PC(id="selu-B17-layers3", act="selu", B=17, hidden=(16, 8)), PC(id="selu-N5x5-fp32", act="selu", hidden=(5, 5)),
           PC(id="selu-d6-chain", act="selu", d_h=6), PC(id="selu-loss-mse-t3", act="selu", B=17, tasks=3, kind="mse"),
           PC(id="selu-loss-mve-t3", act="selu", B=17, tasks=3, kind="mve", transform="mve"), PC(id="selu-B100-d64-N36", act="selu", B=100, d_h=64, hidden=(36,), tasks=2),
           PC(id="selu-out130", act="selu", transform="none", n_out=130, unscale=False)]


@pytest.mark.parametrize("case", PREDICT, ids=lambda c: c.id)
def test_selu_predict_head(case, gpu_device):
    inp = ph.build_inputs(case)
    ref, e32 = ph.yardstick(case, inp)
    call = ph.Call(case, inp, gpu_device)
    first = call.run(0)
    assert call.untouched() == []
    fails = ph.compare(case, first, ref, e32, MARGIN)
    assert not fails, (case.id, fails)
    assert ph.same_bits(first, call.run(1)) == [], "a call on the ready split differs"
    got = ph.Call(case, inp, gpu_device, wsplit=False).run(0)   # (no split cache: every hidden layer on the fp32 contraction)
    assert not ph.compare(case, got, ref, e32, MARGIN, tag="/fp32")
