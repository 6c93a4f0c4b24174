"""The one-call training step (``FusedTrainer.step`` -> ``dmpnn_train_step``) as a composition: a pairwise grid over everything the
step can be asked to do, and ONE float64 restatement of the whole step to hold every combination to.  A plain module: no fixtures,
no pytest settings.

* ``StepCase`` / ``FACTORS`` / ``valid`` / ``grid``: the factors of a step (block kind, activation, block bias, depth, atom
  descriptors, batch shape, aggregation, batch norm, molecule descriptors, predictor depth, criterion, weights, missing targets,
  optimiser options, components), which combinations the trainer refuses — restated here from ``fused_block``, ``HeadSpec.__init__``
  and ``FusedTrainer.__init__``, never derived by calling them — and a deterministic greedy covering set in which every pair of
  settings that some valid case can hold appears.
* ``build``: the model (the package's own classes) and the inputs of a case, on the CPU in float32.
* ``restate``: one training step op by op in a given dtype, from the suite's independent restatements alone —
  ``oracle.dmpnn_torch.forward`` / ``atom_forward``, ``oracle.agg_torch``, ``F.batch_norm``, ``oracle.ffn_torch.mlp_forward``,
  ``head_harness.criterion``, ``test_dirichlet_step_gpu.dirichlet_loss64``, ``test_mcc_head.mcc_criterion``,
  ``test_spectral_head.spectral_criterion`` — then Lightning's clip on the gradients.  ``chemprop_amd.model.criterion_loss`` and the
  predictors' ``train_step`` are code under test and are not used.  float64 is the reference, float32 the yardstick.
* ``adam_replay``: Adam in a given dtype fed with the gradients the device produced ("the update itself").
* ``compare``: the suite's rule, ``err = max|got - ref| / max|ref|`` within ``min(margin max(e32, 2**-23), cap)``.

Dropout (block, predictor, V_d) is out of scope: its masks are restated per site in the dropout tests; here every ``p`` is 0.

The clip and the flat gradient views.  ``dmpnn_clip_grad`` (``csrc/dmpnn_optim.hip``) scales (``k_clip_scale``) or clamps
(``k_clip_value``) the flat gradient buffer IN PLACE between the backward pass and ``k_adam``, and with one rank ``grad_scale`` is 1:
after a step the views hold the CLIPPED gradients.  ``restate`` therefore returns the clipped float64 gradients (norm: ``g *= min(1,
c / (||g||_2 + 1e-6))`` over all gradients; value: every entry clamped to ``[-c, c]`` — ``include/dmpnn.h`` at ``dmpnn_clip_grad``)
and the views are compared with those.  Weight decay enters inside ``k_adam`` (``g + wd p``), not the buffer: ``adam_replay`` adds it.

Gradients that are zero in exact arithmetic.  ``agg.W.bias`` behind an attentive aggregation (the softmax is shift invariant) and
``W_d.bias`` when a mean or attentive aggregation feeds a batch norm (a shift of every atom's row shifts every molecule's aggregate
alike, which the batch norm removes) have a float64 gradient of rounding noise: ``max|ref|`` is no scale for them.  They are judged
against the sum they are — ``sum_v |dl_v|`` of the attention logits, ``max_col sum_v |gH_v'|`` of the layer's output — in place of
``max|ref|``; ``restate`` returns those sums as ``scales``.

Adam runs with ``eps = 1e-4`` on every side, as in ``tests/test_attentive_step_gpu.py`` and ``tests/test_selu_step_gpu.py``: with
1e-8 an entry whose gradient is rounding noise moves by a full ``lr`` in the noise's direction, the device's trajectory leaves the
CPU's, and the distances from the ReLU kinks that ``find_seed`` establishes on the CPU would say nothing about the device.
"""
import copy
import dataclasses
import itertools
import math
import types
from typing import Optional

import torch

from conftest import parity_err_unfloored
import head_harness as hh

F = torch.nn.functional

HEADS = ("mse", "mae", "bounded-mse", "bounded-mae", "bce", "ce", "mve", "evidential", "quantile", "dirichlet-binary",
         "dirichlet-multiclass", "sid", "wasserstein", "mcc")
FACTORS = dict(
    block=("bond", "atom", "undirected"),
    act=("relu", "leakyrelu", "tanh", "elu", "selu"),
    bias=(False, True),
    depth=(1, 2, 3),
    d_vd=(0, 5),
    graphs=("qm9", "zinc", "mixed"),
    agg=("sum", "mean", "norm", "attentive"),
    bn=(True, False),
    d_xd=(0, 7),
    hidden=((), (32,), (32, 24)),
    head=HEADS,
    weights=(True, False),
    missing=(False, True),
    optim=("plain", "clip-norm", "clip-value", "weight-decay", "lr-override"),
    components=("1", "2-shared", "2-separate"),
)
D_H, N_CLASSES, STEPS = 64, 3, 3
# the synthetic one-hot features times 8, as in tests/test_selu_step_gpu.py: a freshly initialised block on unit features stays in the
# near-linear range of tanh / elu / selu, where a mean or attentive aggregation in front of a batch norm makes the gradient of W_o's
# bias a cancelling sum (the loss does not see a uniform shift of H_v) that float32 itself misses by more than the cap
FEATURE_SCALE = 8.0
N_MOLS = dict(qm9=16, zinc=6, mixed=16)   # (mixed: 15 QM9-shaped molecules and one of 40 atoms)
N_MOLS_2 = dict(qm9=8, zinc=6, mixed=8)   # per component of a two-component case
LR, WEIGHT_DECAY, ADAM_EPS, BETAS = 1e-3, 0.1, 1e-4, (0.9, 0.999)
LR_OVERRIDE = (5e-4, 2e-3, 1.5e-3)        # step(..., lr=...) of the three steps of an ``lr-override`` case
EPS32 = 2.0 ** -23
CAP = dict(hh.CAP, param=2e-6)
HEADROOM = 3.0   # find_seed keeps the float32 yardstick this far under every cap: a kernel three times as far off as fp32 torch still passes
KINKED = ("relu", "leakyrelu")


@dataclasses.dataclass(frozen=True)
class StepCase:
    block: str = "bond"
    act: str = "relu"
    bias: bool = False
    depth: int = 3
    d_vd: int = 0
    graphs: str = "qm9"
    agg: str = "mean"
    bn: bool = True
    d_xd: int = 0
    hidden: tuple = (32,)
    head: str = "mse"
    weights: bool = True
    missing: bool = False
    optim: str = "plain"
    components: str = "1"
    seed: int = 0
    staged: bool = False
    index: int = 0

    @property
    def id(self) -> str:
        o = lambda b: "1" if b else "0"
        return (f"{self.index:02d}-{self.block}-{self.act}-b{o(self.bias)}-d{self.depth}-vd{self.d_vd}-{self.graphs}-{self.agg}-bn{o(self.bn)}"
                f"-xd{self.d_xd}-h{len(self.hidden)}-{self.head}-w{o(self.weights)}-nan{o(self.missing)}-{self.optim}-c{self.components}"
                f"-seed{self.seed}" + ("-staged" if self.staged else ""))

    @property
    def n_comp(self) -> int:
        return 1 if self.components == "1" else 2

    @property
    def tasks(self) -> int:
        return 3 if self.head in ("bce", "mcc", "dirichlet-binary", "sid", "wasserstein") else 2

    @property
    def kind(self) -> str:
        """The criterion's kind as ``head_harness.criterion`` / ``HeadSpec`` name it."""
        return "dirichlet" if self.head.startswith("dirichlet") else self.head.replace("bounded-", "")

    @property
    def bounded(self) -> bool:
        return self.head.startswith("bounded")

    @property
    def n_classes(self) -> int:
        return {"ce": N_CLASSES, "dirichlet-multiclass": N_CLASSES, "dirichlet-binary": 2}.get(self.head, 0)

    @property
    def n_out(self) -> int:
        per = self.n_classes or {"mve": 2, "evidential": 4, "quantile": 2}.get(self.head, 1)
        return self.tasks * per


# ---- what the trainer refuses ---------------------------------------------------------------------------------------------------------
def valid(case: StepCase) -> Optional[str]:
    """Why ``FusedTrainer(model, atom_messages=..., undirected=..., attentive=...)`` refuses the case's model (a fragment of the
    message, in the order the constructor checks), or ``None``.  The sizes here never meet the other refusals: the synthetic batches
    have ``d_e = 14 <= 16``, every block is directed unless it is the ``undirected`` bond block, every criterion sits on its own
    predictor class (``pair_refusal`` restates that rule for the pairs a case never builds)."""
    multi = case.components != "1"
    if multi and case.block == "undirected":
        return "undirected blocks in a multicomponent model"
    if multi and case.block == "atom":
        return "atom blocks in a multicomponent model"
    if case.block == "atom" and case.d_vd:
        return "an atom block with atom descriptors (W_d)"
    if multi and case.d_vd:
        return "atom descriptors (V_ds) in a multicomponent model"
    if multi and case.agg == "attentive":
        return "attentive aggregation in a multicomponent model"
    return None


PREDICTOR = {"mse": "RegressionFFN", "mae": "RegressionFFN", "bounded-mse": "RegressionFFN", "bounded-mae": "RegressionFFN",
             "bce": "BinaryClassificationFFN", "mcc": "BinaryClassificationFFN", "ce": "MulticlassClassificationFFN", "mve": "MveFFN",
             "evidential": "EvidentialFFN", "quantile": "QuantileFFN", "dirichlet-binary": "BinaryDirichletFFN",
             "dirichlet-multiclass": "MulticlassDirichletFFN", "sid": "SpectralFFN", "wasserstein": "SpectralFFN"}


def pair_refusal(pred_head: str, crit_head: str) -> Optional[str]:
    """Why ``HeadSpec`` refuses the predictor class of ``pred_head`` under the criterion of ``crit_head`` (a fragment of the message),
    or ``None``: Dirichlet, spectral and chunked (MVE / evidential / quantile) criteria and their predictors only meet each other, a
    class dimension only cross entropy or Dirichlet, binary MCC only ``BinaryClassificationFFN``; one value per task is one value per
    task, whichever of MSE / MAE / BCE reads it."""
    pred = PREDICTOR[pred_head]
    kind = "dirichlet" if crit_head.startswith("dirichlet") else crit_head.replace("bounded-", "")
    if (kind == "dirichlet") != ("Dirichlet" in pred):
        return "Dirichlet"
    if (kind in ("sid", "wasserstein")) != (pred == "SpectralFFN"):
        return "SpectralFFN"
    if kind == "mcc" and pred != "BinaryClassificationFFN":
        return "binary MCC criterion"
    n_targets = {"MveFFN": 2, "EvidentialFFN": 4, "QuantileFFN": 2}.get(pred, 1)
    want = {"mve": ("MveFFN", 2), "evidential": ("EvidentialFFN", 4), "quantile": ("QuantileFFN", 2)}.get(kind, (None, 1))
    if n_targets != want[1] or (want[0] is not None and want[0] != pred):
        return "one value per task"
    if (kind in ("ce", "dirichlet")) != (pred in ("MulticlassClassificationFFN", "MulticlassDirichletFFN", "BinaryDirichletFFN")):
        return "a multiclass predictor"
    return None


def trainer_flags(case: StepCase) -> dict:
    """Exactly the opt-in flags the case needs."""
    kw = {}
    if case.block == "atom":
        kw["atom_messages"] = True
    if case.block == "undirected":
        kw["undirected"] = True
    if case.agg == "attentive":
        kw["attentive"] = True
    return kw


# ---- the grid -------------------------------------------------------------------------------------------------------------------------
_COUPLED = ("block", "d_vd", "agg", "components")   # the factors ``valid`` reads


def _feasible() -> list:
    return [c for c in (dict(zip(_COUPLED, v)) for v in itertools.product(*[FACTORS[f] for f in _COUPLED])) if valid(StepCase(**c)) is None]


def _completable(assign: dict, feasible: list) -> bool:
    return any(all(c[f] == assign[f] for f in _COUPLED if f in assign) for c in feasible)


def all_pairs() -> list:
    """Every pair of settings ``((factor A, a), (factor B, b))``, A before B in ``FACTORS``, that some valid case holds."""
    feasible, names, out = _feasible(), list(FACTORS), []
    for i, a in enumerate(names):
        for b in names[i + 1:]:
            for va in FACTORS[a]:
                for vb in FACTORS[b]:
                    if _completable({a: va, b: vb}, feasible):
                        out.append(((a, va), (b, vb)))
    return out


def pairs_of(case: StepCase) -> set:
    names = list(FACTORS)
    return {((a, getattr(case, a)), (b, getattr(case, b))) for i, a in enumerate(names) for b in names[i + 1:]}


def _greedy() -> list:
    """Deterministic greedy covering: a case starts from the first pair still uncovered; every other factor — those with the most
    settings first, then ``FACTORS`` order — takes the value that covers the most uncovered pairs with the values already set (ties:
    the value used least so far, then ``FACTORS`` order) among those a valid case can still be completed with.  82 cases: ``head`` x
    ``act`` alone needs 70, ``head`` x ``components`` another 28 of which the former can carry most."""
    feasible, names = _feasible(), list(FACTORS)
    todo = all_pairs()
    uncovered = set(todo)
    used = {(f, v): 0 for f in names for v in FACTORS[f]}
    key = lambda f, v, g, u: ((f, v), (g, u)) if names.index(f) < names.index(g) else ((g, u), (f, v))
    cases = []
    while uncovered:
        first = next(p for p in todo if p in uncovered)
        assign = dict(first)
        for f in sorted(names, key=lambda f: -len(FACTORS[f])):   # (stable: the factors with the most settings first)
            if f in assign:
                continue
            best = None
            for v in FACTORS[f]:
                if not _completable({**assign, f: v}, feasible):
                    continue
                gain = sum(key(f, v, g, u) in uncovered for g, u in assign.items())
                score = (-gain, used[(f, v)])
                if best is None or score < best[0]:
                    best = (score, v)
            assign[f] = best[1]
        case = StepCase(**assign)
        assert valid(case) is None, case
        for f in names:
            used[(f, assign[f])] += 1
        uncovered -= pairs_of(case)
        cases.append(case)
    return cases


# a seed at which ``seed_refusal`` has nothing to say, for each case of the grid in grid order — found by ``find_seed`` and kept here so that
# collecting the tests costs nothing (tests/test_step_combinations.py holds every entry to the conditions; the ZINC-shaped two-component
# ReLU cases needed thousands of draws: the kinks of three steps and a cancelling bias gradient in front of a batch norm at once)
SEEDS = (0, 739, 0, 0, 0, 0, 11, 0, 0, 0, 26, 2, 4, 1, 0, 4, 11, 0, 0, 0,
         5504, 406, 0, 0, 0, 4, 0, 7, 0, 14, 0, 0, 6, 161, 0, 5, 3, 0, 0, 0,
         3, 133, 25169, 35, 16, 8, 30, 87, 91, 3, 14, 2, 1, 0, 0, 0, 0, 0, 0, 0,
         0, 0, 0, 0, 22, 0, 0, 0, 0, 0, 294, 371, 1, 0, 0, 0, 61, 0, 26, 0,
         440, 1)


def grid() -> list:
    """The covering set with each case's seed (``SEEDS``) and index; every fourth case, which reaches all three block kinds, also
    runs the staged step."""
    cases = _greedy()
    seeds = SEEDS if len(SEEDS) == len(cases) else (0,) * len(cases)
    out = [dataclasses.replace(c, seed=s, index=i, staged=(i % 4 == 1)) for i, (c, s) in enumerate(zip(cases, seeds))]
    assert {c.block for c in out if c.staged} == set(FACTORS["block"])
    return out


# ---- the model and the inputs -----------------------------------------------------------------------------------------------------------
def _activation(name: str):
    return dict(relu=F.relu, leakyrelu=lambda x: F.leaky_relu(x, hh.LEAKY_SLOPE), tanh=torch.tanh, elu=F.elu, selu=F.selu)[name]


def make_predictor(pred_head: str, crit_head: str, tasks: int, input_dim: int, hidden: tuple, act: str):
    """The predictor class of ``pred_head`` under the criterion of ``crit_head`` (a case has the two equal), non-unit task weights."""
    from chemprop_amd import model as M

    tw = torch.tensor([0.5, 1.0, 1.5])[:tasks]
    crit = {"mse": M.MSE, "mae": M.MAE, "bounded-mse": M.MSE, "bounded-mae": M.MAE, "bce": M.BCE, "ce": M.CE, "mve": M.MVE,
            "evidential": M.Evidential, "quantile": M.Quantile, "dirichlet-binary": M.Dirichlet, "dirichlet-multiclass": M.Dirichlet,
            "sid": M.SID, "wasserstein": M.Wasserstein, "mcc": M.BinaryMCC}[crit_head](tw)
    kw = dict(n_tasks=tasks, input_dim=input_dim, hidden_dim=list(hidden), n_layers=len(hidden), activation=act, criterion=crit)
    cls = getattr(M, PREDICTOR[pred_head])
    return cls(N_CLASSES, **kw) if PREDICTOR[pred_head].startswith("Multiclass") else cls(**kw)


def make_model(case: StepCase, seed: int, crit_head: Optional[str] = None):
    from chemprop_amd import agg as cagg
    from chemprop_amd import nn as cnn
    from chemprop_amd.model import MPNN, MulticomponentMPNN

    torch.manual_seed(1000 + seed)
    cls = cnn.AtomMessagePassing if case.block == "atom" else cnn.BondMessagePassing
    block = lambda: cls(d_h=D_H, bias=case.bias, depth=case.depth, activation=case.act, undirected=case.block == "undirected",
                        d_vd=case.d_vd or None)
    if case.components == "1":
        mp = block()
    else:
        shared = case.components == "2-shared"
        mp = cnn.MulticomponentMessagePassing([block() for _ in range(1 if shared else 2)], 2, shared=shared)
    width = int(mp.output_dim)
    agg = (cagg.AttentiveAggregation(output_size=width) if case.agg == "attentive" else
           dict(sum=cagg.SumAggregation, mean=cagg.MeanAggregation, norm=cagg.NormAggregation)[case.agg]())
    pred = make_predictor(case.head, crit_head or case.head, case.tasks, width + case.d_xd, case.hidden, case.act)
    model = (MPNN if case.components == "1" else MulticomponentMPNN)(mp, agg, pred, batch_norm=case.bn)
    if case.bn:   # (batch-norm parameters and running statistics off 1 / 0)
        with torch.no_grad():
            model.bn.weight.uniform_(0.5, 1.5), model.bn.bias.uniform_(-0.5, 0.5)
            model.bn.running_mean.uniform_(-0.1, 0.1), model.bn.running_var.uniform_(0.5, 2.0)
    return model.train()


def make_batch(graphs: str, seed: int, n_comp: int = 1):
    """One component's batch.  A two-component case holds ``N_MOLS_2`` molecules per component: about the rows of a one-component
    case in all, which keeps the count of pre-activations — and with it the search for a seed off the ReLU kinks — the same."""
    from chemprop_amd import synth
    from test_spill import _mixed

    n = (N_MOLS if n_comp == 1 else N_MOLS_2)[graphs]
    bmg = _mixed(n - 1, [("synth40", seed + 1)], seed=seed, where=[n // 2])[1] if graphs == "mixed" else synth.random_batch(n, graphs, seed=seed)
    bmg.V, bmg.E = bmg.V * FEATURE_SCALE, bmg.E * FEATURE_SCALE
    return bmg


def make_targets(case: StepCase, n: int, gen) -> torch.Tensor:
    t = case.tasks
    if case.kind in ("bce", "mcc"):
        T = (torch.rand(n, t, generator=gen) < (0.5 if case.kind == "bce" else 0.4)).float()
    elif case.kind in ("ce", "dirichlet"):
        T = torch.randint(0, case.n_classes, (n, t), generator=gen).float()
    elif case.kind in ("sid", "wasserstein"):
        T = 0.05 + torch.rand(n, t, generator=gen, dtype=torch.float64)
    else:
        T = torch.randn(n, t, generator=gen)
    gone = torch.zeros(n, t, dtype=torch.bool)
    if case.missing:
        gone = torch.rand(n, t, generator=gen) < 0.15
        gone[torch.arange(n), torch.arange(n) % t] = False   # (every row keeps a target: a spectrum renormalises over its finite entries)
    if case.kind in ("sid", "wasserstein"):   # target spectra sum to 1 over their finite entries
        T = (T / torch.where(gone, torch.zeros_like(T), T).sum(1, keepdim=True)).float()
    T[gone] = float("nan")
    return T


def _build_once(case: StepCase, seed: int) -> tuple:
    model = make_model(case, seed)
    bmgs = [make_batch(case.graphs, 100 * seed + 7 * c, case.n_comp) for c in range(case.n_comp)]
    n = len(bmgs[0])
    gen = torch.Generator().manual_seed(5000 + seed)
    inp = dict(bmgs=bmgs, n_mols=n, T=make_targets(case, n, gen))
    inp["w"] = (0.5 + torch.rand(n, 1, generator=gen)) if case.weights else None
    inp["lt"] = (torch.rand(n, case.tasks, generator=gen) < 0.3) if case.bounded else None
    inp["gt"] = (torch.rand(n, case.tasks, generator=gen) < 0.3) if case.bounded else None
    inp["X_d"] = torch.randn(n, case.d_xd, generator=gen) if case.d_xd else None
    inp["V_d"] = torch.randn(int(bmgs[0].V.shape[0]), case.d_vd, generator=gen) if case.d_vd else None
    inp["clip"] = None
    if case.optim.startswith("clip"):   # half the norm / a quarter of the largest entry of the first step's float64 gradients: the clip bites
        g = [v for k, v in restate(model, case, inp, torch.float64).items() if k.startswith("g.")]
        c = 0.5 * math.sqrt(sum(float((x ** 2).sum()) for x in g)) if case.optim == "clip-norm" else 0.25 * max(float(x.abs().max()) for x in g)
        inp["clip"] = (float(f"{c:.2e}"), case.optim[5:])
    return model, inp


def step_kwargs(case: StepCase, inp: dict, step: int) -> dict:
    """The optimiser options ``FusedTrainer.step`` gets at ``step`` (0-based)."""
    kw = {}
    if case.optim == "lr-override":
        kw["lr"] = LR_OVERRIDE[step]
    if inp["clip"] is not None:
        kw["clip"] = inp["clip"]
    return kw


def beyond_the_tile(bmg) -> bool:
    """The batch cannot take the tile kernels: a molecule beyond the tile, or more than 30 directed edges per molecule on average
    (``FusedTrainer._block_plan``)."""
    return bool(bmg.oversize) or int(bmg.E.shape[0]) > 30 * len(bmg)


# ---- one step, op by op ---------------------------------------------------------------------------------------------------------------
class _Rec:
    def __init__(self, fn):
        self.fn, self.pre = fn, []

    def __call__(self, z):
        self.pre.append(z.detach())
        return self.fn(z)


def zero_gradients(case: StepCase) -> list:
    """The parameters whose gradient is zero in exact arithmetic (module docstring)."""
    out = ["agg.W.bias"] if case.agg == "attentive" else []
    if case.d_vd and case.bn and case.agg in ("mean", "attentive"):
        out.append("message_passing.W_d.bias")
    return out


def _criterion(case: StepCase, crit, Y, T, w, lt, gt):
    from test_dirichlet_step_gpu import dirichlet_loss64
    from test_mcc_head import mcc_criterion
    from test_spectral_head import spectral_criterion

    tw = crit.task_weights.reshape(-1).to(Y.dtype)
    w = torch.ones(Y.shape[0], dtype=Y.dtype) if w is None else w.reshape(-1)
    if case.kind == "dirichlet":
        return dirichlet_loss64(Y, T, w, tw, case.n_classes, float(crit.v_kl))
    if case.kind == "mcc":
        return mcc_criterion(Y, T, w, tw)
    if case.kind in ("sid", "wasserstein"):
        return spectral_criterion(case.kind, Y, T, w, tw, "softplus", crit.threshold)
    hc = types.SimpleNamespace(kind=case.kind, tasks=case.tasks, n_classes=case.n_classes)
    return hh.criterion(hc, Y, T, w, tw, lt, gt, v_kl=float(getattr(crit, "v_kl", 0.2)), eps=float(getattr(crit, "eps", 1e-8)),
                        alpha=float(getattr(crit, "alpha", 0.1)))


def restate(model, case: StepCase, inp: dict, dtype) -> dict:
    """One training step of ``model`` (a CPU module holding the parameters and running statistics the step starts from; it is not
    changed) on ``inp`` in ``dtype``.  Returns by name: ``loss`` [1], ``preds`` (the raw outputs), ``g.<parameter>`` (every gradient,
    after the case's clip), ``running_mean`` / ``running_var`` after the step, ``z`` (the pre-activations of every site: the block's,
    then the predictor's) and ``scales`` (``zero_gradients``: the sum each of them is)."""
    from oracle import agg_torch, ffn_torch
    from oracle import dmpnn_torch as od

    P = {k: p.detach().to(dtype).clone().requires_grad_(True) for k, p in model.named_parameters()}
    name_of = {id(p): k for k, p in model.named_parameters()}
    g = lambda p: None if p is None else P[name_of[id(p)]]
    rec = _Rec(_activation(case.act))
    mp = model.message_passing
    blocks = list(mp.blocks) if case.components != "1" else [mp]
    parts, keep = [], {}
    for c, bmg in enumerate(inp["bmgs"]):
        b = blocks[min(c, len(blocks) - 1)]
        w = od.MPWeights(g(b.W_i.weight), g(b.W_h.weight), g(b.W_o.weight), g(b.W_o.bias), g(b.W_i.bias), g(b.W_h.bias),
                         *((g(b.W_d.weight), g(b.W_d.bias)) if b.W_d is not None else (None, None)))
        fwd = od.atom_forward if case.block == "atom" else od.forward
        Hv = fwd(bmg.V.to(dtype), bmg.E.to(dtype), bmg.edge_index, bmg.rev_edge_index, w, depth=case.depth, activation=rec,
                 undirected=case.block == "undirected", V_d=None if inp["V_d"] is None else inp["V_d"].to(dtype))
        Hv.retain_grad()
        if case.agg == "attentive":
            A = agg_torch.attentive(Hv, bmg.batch, g(model.agg.W.weight), g(model.agg.W.bias))
            A.retain_grad()
            keep["A"] = A
        elif case.agg == "norm":
            A = agg_torch.norm(Hv, bmg.batch, float(model.agg.norm))
        else:
            A = (agg_torch.mean if case.agg == "mean" else agg_torch.sum_)(Hv, bmg.batch)
        keep["Hv"], keep["batch"] = Hv, bmg.batch
        parts.append(A)
    H = torch.cat(parts, 1) if len(parts) > 1 else parts[0]
    out = {}
    if case.bn:
        rm, rv = model.bn.running_mean.to(dtype).clone(), model.bn.running_var.to(dtype).clone()
        H = F.batch_norm(H, rm, rv, g(model.bn.weight), g(model.bn.bias), True, model.bn.momentum, model.bn.eps)
        out.update(running_mean=rm, running_var=rv)
    if inp["X_d"] is not None:
        H = torch.cat((H, model.X_d_transform(inp["X_d"]).to(dtype)), 1)
    lin = [m for m in model.predictor.ffn.modules() if isinstance(m, torch.nn.Linear)]
    frec = _Rec(_activation(getattr(case, "ffn_act", None) or case.act))   # (a golden may give its predictor another activation)
    Y = ffn_torch.mlp_forward(H, [g(m.weight) for m in lin], [g(m.bias) for m in lin], frec)
    T = inp["T"].to(dtype)
    loss = _criterion(case, model.predictor.criterion, Y, T, None if inp["w"] is None else inp["w"].to(dtype), inp["lt"], inp["gt"])
    loss.backward()
    grads = {k: (p.grad if p.grad is not None else torch.zeros_like(p)) for k, p in P.items()}
    scales = {}
    with torch.no_grad():
        if case.agg == "attentive":   # dl_v = alpha_v (a_v - sum_u alpha_u a_u), a_v = <gA_mol(v), h_v>: agg.W.bias's gradient is their sum
            Hv, b, A = keep["Hv"], keep["batch"], keep["A"]
            n = int(A.shape[0])
            s = F.linear(Hv, P["agg.W.weight"], P["agg.W.bias"]).exp().reshape(-1)
            al = s / torch.zeros(n, dtype=dtype).index_add(0, b, s)[b]
            a = (A.grad[b] * Hv).sum(1)
            cbar = torch.zeros(n, dtype=dtype).index_add(0, b, al * a)
            scales["agg.W.bias"] = float((al * (a - cbar[b])).abs().sum())
        if "message_passing.W_d.bias" in zero_gradients(case):
            scales["message_passing.W_d.bias"] = float(keep["Hv"].grad.abs().sum(0).max())
        if inp["clip"] is not None:
            c, mode = inp["clip"]
            if mode == "norm":
                total = torch.sqrt(sum((x ** 2).sum() for x in grads.values()))
                coef = min(1.0, c / (float(total) + 1e-6))
                grads = {k: x * coef for k, x in grads.items()}
                scales = {k: v * coef for k, v in scales.items()}
            else:
                grads = {k: x.clamp(-c, c) for k, x in grads.items()}
    out.update(loss=loss.detach().reshape(1), preds=Y.detach(), z=rec.pre + frec.pre, scales=scales)
    out.update({"g." + k: x.detach() for k, x in grads.items()})
    return out


def tensor_names(ref: dict) -> list:
    return [k for k in ref if k not in ("z", "scales")]


def adam_replay(p0: dict, grads_per_step: list, case: StepCase, dtype=torch.float64) -> list:
    """``torch.optim.Adam``'s arithmetic (amsgrad off) in ``dtype`` from the parameters ``p0`` over the given gradients — the ones the
    device produced, already clipped — with the case's learning rate (``LR``, or ``LR_OVERRIDE`` per step), weight decay and ``ADAM_EPS``.
    Returns the parameters after each step."""
    b1, b2 = BETAS
    wd = WEIGHT_DECAY if case.optim == "weight-decay" else 0.0
    p = {k: v.to(dtype).clone() for k, v in p0.items()}
    m = {k: torch.zeros_like(v) for k, v in p.items()}
    v = {k: torch.zeros_like(x) for k, x in p.items()}
    out = []
    for s, grads in enumerate(grads_per_step):
        lr = LR_OVERRIDE[s] if case.optim == "lr-override" else LR
        for k in p:
            gr = grads[k].to(dtype) + wd * p[k]
            m[k] = b1 * m[k] + (1 - b1) * gr
            v[k] = b2 * v[k] + (1 - b2) * gr * gr
            p[k] = p[k] - (lr / (1 - b1 ** (s + 1))) * m[k] / (v[k].sqrt() / math.sqrt(1 - b2 ** (s + 1)) + ADAM_EPS)
        out.append({k: x.clone() for k, x in p.items()})
    return out


def optimizer_kwargs(case: StepCase) -> dict:
    """What the constructor of ``FusedTrainer`` gets beside the flags."""
    return dict(lr=LR, betas=BETAS, eps=ADAM_EPS, weight_decay=WEIGHT_DECAY if case.optim == "weight-decay" else 0.0)


def load_state(model, params: dict, stats: Optional[dict] = None) -> None:
    """Parameters by name (any dtype -> float32) and, for a model with batch norm, the running statistics into ``model``."""
    with torch.no_grad():
        for k, p in model.named_parameters():
            p.copy_(params[k].to(p.dtype))
        if stats:
            model.bn.running_mean.copy_(stats["running_mean"].float())
            model.bn.running_var.copy_(stats["running_var"].float())


def cpu_trajectory(model, case: StepCase, inp: dict, steps: int = STEPS) -> list:
    """``steps`` steps on the CPU with the float32 restatement in the device's place: per step ``(ref64, ref32, p64, p32)`` — both
    restatements from the current float32 parameters, then the parameters after the step by ``adam_replay`` in float64 and in
    float32, both fed with the float32 gradients; the float32 ones are what the next step starts from."""
    m = copy.deepcopy(model)
    p0 = {k: p.detach().clone() for k, p in m.named_parameters()}
    grads, out = [], []
    for _ in range(steps):
        r64, r32 = restate(m, case, inp, torch.float64), restate(m, case, inp, torch.float32)
        grads.append({k[2:]: v for k, v in r32.items() if k.startswith("g.")})
        p64, p32 = adam_replay(p0, grads, case)[-1], adam_replay(p0, grads, case, torch.float32)[-1]
        out.append((r64, r32, p64, p32))
        load_state(m, p32, r32 if case.bn else None)
    return out


def cap_of(name: str) -> float:
    return CAP["loss" if name == "loss" else "preds" if name == "preds" else "stat" if name.startswith("running") else
               "param" if name.startswith("p.") else "grad"]


def yardstick(r64: dict, r32: dict) -> dict:
    """Per tensor the error of the float32 restatement against the float64 one, in ``compare``'s measure."""
    return {k: _err(r32[k], r64[k], r64["scales"].get(k[2:]) if k.startswith("g.") else None)[0] for k in tensor_names(r64)}


def _err(got, ref, scale=None) -> tuple:
    g, r = got.double().reshape(-1), ref.double().reshape(-1)
    assert g.shape == r.shape, (tuple(got.shape), tuple(ref.shape))
    if scale is None:
        return parity_err_unfloored(g.numpy(), r.numpy()), float(r.abs().max())
    return float((g - r).abs().max()) / scale, scale


def kink_clearance(r64: dict, r32: dict) -> tuple:
    """``(min |z64|, delta)`` of the site (one activation call of the block or the predictor) that is closest to a kink in units of
    its own ``delta``: 16 times the largest ``|z32 - z64|`` of that site's pre-activations.  Within ``delta`` of 0 a float32
    implementation may take the other branch of a ReLU.  (Per site, not one ``delta`` per case: behind a sum aggregation without batch
    norm the predictor's pre-activations are a hundred times the block's, and their float32 error says nothing about the block's
    branches.)"""
    sites = [(float(b.abs().min()), 16.0 * float((a.double() - b).abs().max())) for a, b in zip(r32["z"], r64["z"])]
    return min(sites, key=lambda t: t[0] / t[1] if t[1] > 0 else float("inf"))


def seed_refusal(case: StepCase, model, inp: dict, strict: bool = True) -> Optional[str]:
    """Why this draw of a case is not used (``None``: it is): a ZINC-shaped batch the tile kernels would take; over ``STEPS`` CPU
    steps a pre-activation of a ReLU / LeakyReLU model within ``delta`` of 0, a tensor of the float32 yardstick within ``HEADROOM`` of
    its cap, or — ``bounded-*``, ``mae``, ``quantile``, ``evidential`` — a prediction within ``delta`` of its target (the kink of
    ``|y - p|``; ``delta``: 16 times the largest ``|p32 - p64|``).  ``strict`` is how ``find_seed`` asks: 1.25 ``delta`` and ``HEADROOM``,
    so that what it settles on still holds where float32 rounds differently (another thread count regroups the CPU's sums); without
    it the conditions are the plain ones — ``delta`` and the caps — which ``tests/test_step_combinations.py`` asserts."""
    room, wide = (HEADROOM, 1.25) if strict else (1.0, 1.0)
    if case.graphs != "qm9" and not all(beyond_the_tile(b) for b in inp["bmgs"]):
        return "the batch would take the tile kernels"
    if case.graphs == "qm9" and any(beyond_the_tile(b) for b in inp["bmgs"]):
        return "the batch would not take the tile kernels"
    for s, (r64, r32, p64, p32) in enumerate(cpu_trajectory(model, case, inp)):
        lo, delta = kink_clearance(r64, r32)
        if case.act in KINKED and not lo >= wide * delta:
            return f"step {s + 1}: a pre-activation at {lo:.2e} (delta {delta:.2e})"
        if case.kind in ("mae", "quantile", "evidential") or case.bounded:
            t = case.tasks
            T = inp["T"].double()
            gaps = [(T - r64["preds"][:, i * t:(i + 1) * t]).abs() for i in range(2 if case.kind == "quantile" else 1)]
            gap = min(float(x[T.isfinite()].min()) for x in gaps)
            d = 16.0 * float((r32["preds"].double() - r64["preds"]).abs().max())
            if not gap >= wide * d:
                return f"step {s + 1}: a prediction {gap:.2e} from its target (delta {d:.2e})"
        e32 = yardstick(r64, r32)
        e32.update({"p." + k: _err(p32[k], p64[k])[0] for k in p64})
        for k, e in e32.items():
            if not e * room <= cap_of(k):
                return f"step {s + 1}: float32 {k} at {e:.2e} (cap {cap_of(k):.1e})"
    return None


def find_seed(case: StepCase, start: int = 0, limit: int = 64) -> int:
    for seed in range(start, start + limit):
        if seed_refusal(case, *_build_once(case, seed)) is None:
            return seed
    raise AssertionError(f"{case.id}: no seed in {start} .. {start + limit - 1} is usable")


def build(case: StepCase, seed: Optional[int] = None) -> tuple:
    """``(model, inp)`` on the CPU in float32 for the first usable seed from ``seed`` (default: the case's own, which
    ``tests/test_step_combinations.py`` holds to be usable itself).  ``inp``: ``bmgs`` (one CPU batch per component), ``n_mols``, ``T``,
    ``w``, ``lt`` / ``gt``, ``X_d``, ``V_d``, ``clip`` — ``None`` where the case has none."""
    seed = case.seed if seed is None else find_seed(case, seed)
    return _build_once(case, seed)


def compare(case_id: str, step: int, got: dict, ref: dict, e32: dict, margin: float, scales: Optional[dict] = None, report=print) -> list:
    """Every tensor of ``got`` against ``ref``: finite, ``err = max|got - ref| / max|ref|`` (over ``scales[name]`` for a gradient that is
    zero in exact arithmetic; exactly 0 where the scale is 0) within ``min(margin max(e32, 2**-23), cap)``.  One ``STEPBAR`` line per
    tensor BEFORE judging; returns the failures."""
    fails = []
    for k in got:
        if not bool(torch.isfinite(got[k]).all()):
            report(f"STEPBAR {case_id} step{step} {k} nonfinite")
            fails.append(f"step {step} {k}: not finite")
            continue
        err, scale = _err(got[k], ref[k], (scales or {}).get(k[2:]) if k.startswith("g.") else None)
        bar = 0.0 if scale == 0.0 else min(margin * max(e32[k], EPS32), cap_of(k))
        ratio = err / max(e32[k], EPS32)
        report(f"STEPBAR {case_id} step{step} {k} err={err:.3e} e32={e32[k]:.3e} ratio={ratio:.2f} bar={bar:.3e} maxref={scale:.3e}")
        if not err <= bar:
            fails.append(f"step {step} {k}: err {err:.3e} > bar {bar:.3e} (fp32 yardstick {e32[k]:.3e}, ratio {ratio:.1f}, scale {scale:.3e})")
    return fails
