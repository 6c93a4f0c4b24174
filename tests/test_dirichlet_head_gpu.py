"""``dmpnn_head`` with ``DMPNN_LOSS_DIRICHLET`` through the C ABI: one training call (every output prefilled with NaN) against the head
restated op by op on the CPU — in float64 as the reference, in float32 as the yardstick (the scheme of
``tests/test_head_boundaries.py``; ``head_harness.build_inputs`` / ``run_case`` / ``compare`` are reused through ``DirichletCase``, the
criterion and the reference wrapper are this file's).

The definitions restated here are those of chemprop 2.3.1 (``nn/predictors.py``, ``nn/metrics.py``) as ``include/dmpnn.h`` states them
for ``DMPNN_LOSS_DIRICHLET``; ``tests/test_dirichlet_head.py`` holds them to an independent closed form.

Cases: the smallest call (K=2, t=1, B=3), ``B t > 1024`` (the strided loop of the criterion's single workgroup, both passes), a
multiclass head with 20 % missing targets, with a task without any target (its output rows' gradients exactly 0), without any finite
target (NaN loss on both sides), and an odd K beyond 4 — each without and with a hidden layer, batch norm on, and at three ranges of
evidence: the output layer is rescaled until the raw outputs have a standard deviation of 1, 8 and 25 (alpha near 1: the recurrences of
``digamma_f`` / ``trigamma_f``; alpha up to ~50: their asymptotic series; raw > 20: the linear branch of softplus).  One attentive and
one two-component case (K=3, t=2, B=12) run at the same bars.

Bar per output tensor: ``err <= min(MARGIN max(e32, 2**-23), cap)``, the caps ``head_harness.CAP``.  The caps are a condition, not a
measurement: ``prepared`` asserts on the CPU, before a device is touched, that the float32 restatement alone stays within ``cap / 8``
for every compared tensor of every case.  No element is left out of any comparison.

MARGIN, measured on the MI355X over the 38 head calls of this module (378 tensor comparisons; every line in
``profiles/dirichlet_head_bars.txt``): the worst ``err / max(e32, 2**-23)`` is 3.64 — ``g_bn_bias`` of
``strided-K2-t9-B130-hidden-std25`` (err 7.0e-7 against a float32 draw of 1.9e-7); then 3.59 (the loss of the three-molecule calls at
std 25: err 4.3e-7 and 6.6e-7, one workgroup's tree sum against torch's sequential one) and 2.85 (the loss of ``dead-...-std25``).
Per kind of tensor: batch-norm gradients 3.64, loss 3.59, weight / bias gradients 2.40, predictions 1.99, ``dl/dH_v`` 1.68, running
mean 1.16, the attention's weight gradient 0.61, running variance 0.44; per range of evidence: 2.49 (std 1), 2.40 (std 8), 3.64
(std 25) — no term of the new criterion (the series of ``trigamma_f`` / ``digamma_f``, ``lgammaf``) stands out.
2 x 3.64 = 7.3 -> MARGIN = 8, a quarter of the 32 ``tests/test_head_boundaries.py`` holds for the other criteria.
"""
import contextlib
import dataclasses
import functools
import math

import pytest
import torch

import attn_harness as ah
import head_harness as hh
from chemprop_amd import _lib
from conftest import parity_err_unfloored
from head_harness import HeadCase

F = torch.nn.functional

MARGIN = 8.0


@dataclasses.dataclass(frozen=True)
class DirichletCase(HeadCase):
    """A ``HeadCase`` of kind ``dirichlet``: ``n_classes`` raw outputs per task (the layout of cross entropy); ``scale``: the standard
    deviation the raw outputs are rescaled to."""
    scale: float = 1.0

    @property
    def per_task(self):
        return self.n_classes


def dirichlet_criterion(case, Y, T, w, tw, lt=None, gt=None, v_kl=0.2, **_):
    """``DirichletLoss`` on ``BinaryDirichletFFN`` / ``MulticlassDirichletFFN.train_step`` of the RAW outputs ``Y [B, t K]``, op by op:
    ``sum(L w_row w_task [target finite]) / #finite``."""
    K = case.n_classes
    mask = T.isfinite()
    y = F.one_hot(torch.where(mask, T, torch.zeros_like(T)).long(), K).to(Y.dtype)
    alpha = F.softplus(Y.reshape(Y.shape[0], case.tasks, K)) + 1
    S = alpha.sum(-1, keepdim=True)
    p = alpha / S
    L_mse = ((y - p) ** 2).sum(-1) + (p * (1 - p) / (S + 1)).sum(-1)
    a_t = y + (1 - y) * alpha
    S_t = a_t.sum(-1, keepdim=True)
    L_kl = (torch.lgamma(S_t).squeeze(-1) - torch.lgamma(a_t).sum(-1) - math.lgamma(K)
            + ((a_t - 1) * (torch.digamma(a_t) - torch.digamma(S_t))).sum(-1))
    L = (L_mse + v_kl * L_kl) * w.view(-1, 1) * tw.view(1, -1)
    return torch.where(mask, L, torch.zeros_like(L)).sum() / mask.sum()


@contextlib.contextmanager
def dirichlet_reference():
    """``head_harness.reference`` (and what calls it: ``yardstick``, ``attn_harness.head_reference``) with this file's criterion for
    the cases of kind ``dirichlet``."""
    orig = hh.criterion
    hh.criterion = lambda case, *a, **kw: (dirichlet_criterion if case.kind == "dirichlet" else orig)(case, *a, **kw)
    try:
        yield
    finally:
        hh.criterion = orig


SCALES = (1.0, 8.0, 25.0)
SHAPES = [   # (name, K, t, B, missing)
    ("smallest", 2, 1, 3, "none"),
    ("strided", 2, 9, 130, "some"),
    ("multiclass", 3, 4, 37, "some"),
    ("dead", 3, 4, 37, "dead"),
    ("no-target", 3, 4, 37, "all"),
    ("k7", 7, 3, 64, "some"),
]


def _build_cases():
    cs = []
    for name, K, t, B, missing in SHAPES:
        for hidden in ((), (20,)):
            for scale in SCALES:
                cs.append(DirichletCase(f"{name}-K{K}-t{t}-B{B}-{'hidden' if hidden else 'linear'}-std{scale:g}", "default", B, 24, hidden, t,
                                        kind="dirichlet", act="tanh", agg="mean", bn=True, n_classes=K, missing=missing, scale=scale))
    assert any(c.B * c.tasks > 1024 for c in cs)
    return cs


CASES = _build_cases()
IDS = [c.id for c in CASES]


def _rescale_output_layer(case, inp, raw):
    """The output layer times ``case.scale / std(raw)``: the raw outputs then have the standard deviation ``case.scale``."""
    last = len(case.dims) - 2
    s = case.scale / float(raw.double().std())
    inp[f"W{last}"], inp[f"b{last}"] = (inp[f"W{last}"].double() * s).float(), (inp[f"b{last}"].double() * s).float()


def _assert_float32_within_an_eighth_of_the_caps(cid, names, e32, ref):
    for k in names:
        if not bool(torch.isfinite(ref[k]).all()):
            continue   # (no finite target: a NaN loss and NaN gradients on both sides)
        assert e32[k] <= hh.cap_of(k) / 8, (cid, k, e32[k])


@functools.lru_cache(maxsize=None)
def prepared(case):
    """The inputs (class-index targets as ``build_inputs`` draws them for cross entropy, the output layer rescaled), the float64
    reference and the float32 yardstick; the yardstick is held to an eighth of every cap here, on the CPU."""
    for seed in range(case.seed, case.seed + 8):   # (the input seed advances until float32 itself meets the condition: the inputs change, not the cap)
        inp = hh.build_inputs(dataclasses.replace(case, kind="ce", seed=seed))
        with dirichlet_reference():
            _rescale_output_layer(case, inp, hh.reference(dataclasses.replace(case, mode="eval-loss"), inp)["preds"])
            ref, e32 = hh.yardstick(case, inp)
        assert abs(float(ref["preds"].std()) - case.scale) <= 1e-3 * case.scale
        try:
            _assert_float32_within_an_eighth_of_the_caps(case.id, hh.output_names(case), e32, ref)
            break
        except AssertionError:
            if seed == case.seed + 7:
                raise
    inp["input_seed"] = seed
    return inp, ref, e32


# ---- no GPU -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_inputs_reach_the_branches_and_float32_meets_an_eighth_of_the_caps(case):
    inp, ref, e32 = prepared(case)
    raw = ref["preds"]
    alpha = F.softplus(raw) + 1
    if case.scale == 1.0:
        assert float(alpha.min()) < 2 and float((alpha < 6).double().mean()) > 0.99   # the recurrences
    if case.scale >= 8.0 and case.B > 3:
        assert float(alpha.max()) > 12                               # the asymptotic series, alpha itself beyond 6
    if case.scale == 25.0 and case.B > 3:
        assert float(raw.max()) > 20 and float(raw.min()) < -20      # softplus's linear branch; alpha = 1 to the last bit
    if case.missing == "all":
        assert bool(torch.isnan(ref["loss"]))
    else:
        assert bool(torch.isfinite(ref["loss"])) and float(ref["gHv"].abs().max()) > 0


def test_the_criterion_here_is_masked_loss():
    """This file's op-by-op criterion on the raw outputs against ``masked_loss(kind="dirichlet")`` on ``alpha`` (float64)."""
    from chemprop_amd.model import masked_loss

    case = CASES[IDS.index("multiclass-K3-t4-B37-hidden-std8")]
    inp, ref, _ = prepared(case)
    Y = ref["preds"]
    got = dirichlet_criterion(case, Y, inp["T"].double(), inp["w"].double(), inp["tw"].double())
    want = masked_loss(F.softplus(Y.reshape(case.B, case.tasks, 3)) + 1, inp["T"].double(), inp["w"].double(), inp["tw"].double(), kind="dirichlet")
    assert abs(float(got) - float(want)) <= 1e-14 * abs(float(want)) and abs(float(got) - float(ref["loss"])) <= 1e-14 * abs(float(want))


# ---- GPU ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_dirichlet_head_matches_float64_within_the_float32_yardstick(case, gpu_device):
    inp, ref, e32 = prepared(case)
    got = hh.run_case(case, inp, gpu_device)
    fails = hh.compare(case, got, ref, e32, MARGIN)
    if got["n_finite"] != float(inp["T"].isfinite().sum()):
        fails.append(f"loss_out[1] = {got['n_finite']}: not the number of finite targets")
    if case.missing == "some":   # (a missing target: zero gradient for all K columns — the output bias's gradient sees every column)
        assert bool(torch.isfinite(got[f"gb{len(case.dims) - 2}"]).all())
    assert not fails, f"{case.id}: " + "; ".join(fails)


@pytest.mark.gpu
def test_a_class_index_outside_the_range_is_a_nan_loss(gpu_device):
    """As cross entropy does: a target of ``K`` (or a negative one) makes the loss NaN."""
    case = CASES[IDS.index("multiclass-K3-t4-B37-linear-std1")]
    inp = dict(prepared(case)[0])
    for bad in (3.0, -1.0):
        T = inp["T"].clone()
        T[0, 0] = bad
        got = hh.run_case(dataclasses.replace(case, mode="eval-loss"), dict(inp, T=T), gpu_device)
        assert bool(torch.isnan(got["loss"])), bad


@pytest.mark.gpu
def test_launch_count_equals_cross_entropys(gpu_device):
    """The Dirichlet criterion is a branch of the criterion kernel: a head call launches what the cross-entropy call of the same shape
    launches."""
    lib = _lib.load()
    for cid in ("multiclass-K3-t4-B37-hidden-std1", "strided-K2-t9-B130-linear-std1"):
        case = CASES[IDS.index(cid)]
        inp = prepared(case)[0]
        n = []
        for kind in ("dirichlet", "ce"):
            n0 = int(lib.dmpnn_last_launch_count())
            hh.run_case(dataclasses.replace(case, kind=kind), inp, gpu_device)
            n.append(int(lib.dmpnn_last_launch_count()) - n0)
        assert n[0] == n[1] > 0, (cid, n)


def _judge(cid, name, got, ref, e32, fails, report=print):
    """One tensor at the module's bar; reports before judging."""
    g, r = got.double().reshape(-1), ref.double().reshape(-1)
    assert g.shape == r.shape, (cid, name, tuple(got.shape), tuple(ref.shape))
    if not bool(torch.isfinite(g).all()):
        fails.append(f"{name}: not finite")
        return
    err = parity_err_unfloored(g.numpy(), r.numpy())
    bar = min(MARGIN * max(e32, hh.EPS32), hh.cap_of(name))
    report(f"HEADBAR {cid} {name} err={err:.3e} e32={e32:.3e} ratio={err / max(e32, hh.EPS32):.2f} bar={bar:.3e} maxref={float(r.abs().max()):.3e}")
    if not err <= bar:
        fails.append(f"{name}: err {err:.3e} > bar {bar:.3e} (fp32 yardstick {e32:.3e})")


ATT_CASE = DirichletCase("attentive-K3-t2-B12", "default", 12, 8, (16,), 2, kind="dirichlet", act="tanh", agg="sum", bn=True, n_classes=3,
                         missing="some", scale=8.0)


@functools.lru_cache(maxsize=None)
def prepared_attentive():
    case = ATT_CASE
    inp = ah.head_inputs(dataclasses.replace(case, kind="ce"))
    with dirichlet_reference():
        _rescale_output_layer(case, inp, ah.head_reference(dataclasses.replace(case, mode="eval-loss"), inp)["preds"])
        ref, e32 = ah.head_yardstick(case, inp)
    _assert_float32_within_an_eighth_of_the_caps(case.id, ah.head_output_names(case), e32, ref)
    return inp, ref, e32


def test_attentive_case_float32_meets_an_eighth_of_the_caps():
    prepared_attentive()


@pytest.mark.gpu
def test_attentive_head_with_the_dirichlet_criterion(gpu_device):
    """``agg_mode = DMPNN_MOLAGG_ATTENTIVE``: the attention stage around the same head — nothing of its own for the new criterion."""
    case = ATT_CASE
    inp, ref, e32 = prepared_attentive()
    got = ah.run_head(case, inp, gpu_device)
    fails = hh.compare(case, got, ref, e32, MARGIN)
    _judge(case.id, "g_att_W", got["g_att_W"], ref["g_att_W"], e32["g_att_W"], fails)
    v, bar = abs(float(got["g_att_b"])), MARGIN * hh.EPS32 * ref["sum_abs_dl"]   # (analytically zero: the absolute bar of attn_harness)
    print(f"HEADBAR {case.id} g_att_b |gb|={v:.3e} bar={bar:.3e}")
    if not v <= bar:
        fails.append(f"g_att_b: |gb| {v:.3e} > {bar:.3e}")
    assert not fails, f"{case.id}: " + "; ".join(fails)


# ---- two components: the mirror model through HeadSpec.fill -----------------------------------------------------------------------
def _two_component_inputs(seed=0):
    """A ``MulticomponentMPNN`` of two blocks with a ``MulticlassDirichletFFN`` (K=3, t=2) on 12 target rows, on the CPU: the model,
    the blocks' outputs ``H_v^c``, their batch vectors, targets (20 % missing) and row weights."""
    from chemprop_amd import agg as cagg
    from chemprop_amd.model import Dirichlet, MulticlassDirichletFFN, MulticomponentMPNN
    from chemprop_amd.nn import BondMessagePassing, MulticomponentMessagePassing
    from test_multicomponent import batches

    torch.manual_seed(seed + 11)
    n, d_h = 12, 24
    mp = MulticomponentMessagePassing([BondMessagePassing(72, 14, d_h=d_h, depth=2, activation="tanh") for _ in range(2)], 2, shared=False)
    pred = MulticlassDirichletFFN(3, n_tasks=2, input_dim=2 * d_h, hidden_dim=16, activation="tanh",
                                  criterion=Dirichlet(torch.tensor([0.75, 1.5]), v_kl=0.2))
    model = MulticomponentMPNN(mp, cagg.MeanAggregation(), pred, batch_norm=True).train()
    gen = torch.Generator().manual_seed(seed + 5)
    with torch.no_grad():
        model.bn.weight.uniform_(0.5, 1.5, generator=gen), model.bn.bias.uniform_(-0.5, 0.5, generator=gen)
        model.bn.running_mean.uniform_(-0.1, 0.1, generator=gen), model.bn.running_var.uniform_(0.5, 2.0, generator=gen)
    bs = batches(["qm9", "qm9"], n, seed=seed)
    Hvs = [torch.randn(int(b.V.shape[0]), d_h, generator=gen) for b in bs]
    T = torch.randint(0, 3, (n, 2), generator=gen).float()
    T[torch.rand(n, 2, generator=gen) < 0.2] = float("nan")
    return model, Hvs, [b.batch for b in bs], T, 0.5 + torch.rand(n, 1, generator=gen)


def _restate_two_components(model, Hvs, bts, T, w, dtype):
    """The head of the two-component model op by op on the CPU in ``dtype``; every output of the call by name."""
    f = lambda t: t.detach().cpu().to(dtype)
    n = T.shape[0]
    leaves, Hs = {}, []
    for c, (Hv, b) in enumerate(zip(Hvs, bts)):
        leaves[f"gHv{c}"] = f(Hv).requires_grad_()
        H = torch.zeros(n, Hv.shape[1], dtype=dtype).index_add(0, b.cpu(), leaves[f"gHv{c}"])
        Hs.append(H / torch.bincount(b.cpu(), minlength=n).clamp(min=1).to(dtype).view(-1, 1))
    bn = model.bn
    leaves["g_bn_weight"], leaves["g_bn_bias"] = f(bn.weight).requires_grad_(), f(bn.bias).requires_grad_()
    rm, rv = f(bn.running_mean).clone(), f(bn.running_var).clone()
    Z = F.batch_norm(torch.cat(Hs, 1), rm, rv, leaves["g_bn_weight"], leaves["g_bn_bias"], training=True, momentum=bn.momentum, eps=bn.eps)
    lins = [blk[-1] for blk in model.predictor.ffn]
    for l, lin in enumerate(lins):
        leaves[f"gW{l}"], leaves[f"gb{l}"] = f(lin.weight).requires_grad_(), f(lin.bias).requires_grad_()
        Z = F.linear(torch.tanh(Z) if l else Z, leaves[f"gW{l}"], leaves[f"gb{l}"])
    case = DirichletCase("two-components-K3-t2-B12", "default", n, Hvs[0].shape[1], (16,), 2, kind="dirichlet", n_classes=3)
    loss = dirichlet_criterion(case, Z, f(T), f(w), f(model.criterion.task_weights).reshape(-1))
    loss.backward()
    out = {k: v.grad for k, v in leaves.items()}
    out.update(loss=loss.detach(), preds=Z.detach(), running_mean=rm, running_var=rv)
    return case, out


@functools.lru_cache(maxsize=None)
def prepared_two_components():
    model, Hvs, bts, T, w = _two_component_inputs()
    case, r = _restate_two_components(model, Hvs, bts, T, w, torch.float64)
    with torch.no_grad():   # (raw outputs of a standard deviation of 8)
        s = 8.0 / float(r["preds"].std())
        last = model.predictor.ffn[-1][-1]
        last.weight.mul_(s), last.bias.mul_(s)
    case, r64 = _restate_two_components(model, Hvs, bts, T, w, torch.float64)
    _, r32 = _restate_two_components(model, Hvs, bts, T, w, torch.float32)
    e32 = {k: parity_err_unfloored(r32[k].double().numpy(), r64[k].numpy()) for k in r64}
    _assert_float32_within_an_eighth_of_the_caps(case.id, list(r64), e32, r64)
    return case, model, Hvs, bts, T, w, r64, e32


def test_two_component_case_float32_meets_an_eighth_of_the_caps():
    prepared_two_components()


@pytest.mark.gpu
def test_two_component_head_with_the_dirichlet_criterion(gpu_device):
    """``n_components = 2`` through ``HeadSpec.fill`` (what the one-call step and ``head_loss`` hand over): nothing of its own for the
    new criterion."""
    import copy

    from chemprop_amd.model import HeadSpec
    from test_multicomponent import run_head

    case, cpu_model, Hvs, bts, T, w, ref, e32 = prepared_two_components()
    model = copy.deepcopy(cpu_model).to(gpu_device)
    spec = HeadSpec(model)
    assert (spec.kind, spec.n_classes, spec.n_tasks, spec.n_components) == ("dirichlet", 3, 2, 2)
    to = lambda t: t.to(gpu_device)
    loss, P, g, gH = run_head(model, [to(h) for h in Hvs], [to(b) for b in bts], case.B, to(T), to(w))
    lins = [blk[-1] for blk in model.predictor.ffn]
    got = dict(loss=torch.tensor(loss), preds=P, gHv0=gH[0], gHv1=gH[1], g_bn_weight=g[id(model.bn.weight)], g_bn_bias=g[id(model.bn.bias)],
               running_mean=model.bn.running_mean.cpu(), running_var=model.bn.running_var.cpu())
    for l, lin in enumerate(lins):
        got[f"gW{l}"], got[f"gb{l}"] = g[id(lin.weight)], g[id(lin.bias)]
    fails = []
    assert set(got) == set(ref)
    for k in sorted(ref):
        _judge(case.id, k, got[k], ref[k], e32[k], fails)
    assert not fails, f"{case.id}: " + "; ".join(fails)
