"""The pairwise grid of ``tests/step_harness.py`` and its float64 restatement of the whole training step, without a GPU: the grid
covers every pair of settings a valid case can hold; ``valid`` and ``pair_refusal`` agree with ``FusedTrainer`` / ``HeadSpec`` (the
refusals come before ``_require_device``, so a CPU model shows them); the restatement reproduces the executed reference's first
step wherever a golden exists (``tests/golden/model/*.npz``); and on every case, over the three steps the GPU file runs, the
float32 restatement is under the caps — the bar is one a correct kernel can meet — and no ReLU pre-activation is close enough to 0
for float32 to take the other branch.

The grid has 82 cases (``head`` x ``act`` alone needs 70).  The GPU file is ``tests/test_step_combinations_gpu.py``."""
import dataclasses
import glob
import os

import pytest
import torch

import step_harness as sh
from conftest import GOLDEN_DIR, parity_err

GRID = sh.grid()


# ---- coverage -------------------------------------------------------------------------------------------------------------------------
def test_every_feasible_pair_of_settings_is_in_the_grid():
    want = set(sh.all_pairs())
    have = set().union(*[sh.pairs_of(c) for c in GRID])
    assert not want - have, sorted(want - have, key=str)[:10]
    assert all(sh.valid(c) is None for c in GRID)
    assert len({c.id for c in GRID}) == len(GRID) == 82
    # every single setting is part of some pair, and the infeasible pairs are exactly what ``valid`` names
    for f, values in sh.FACTORS.items():
        for v in values:
            assert any(getattr(c, f) == v for c in GRID), (f, v)
    gone = {(("block", "atom"), ("d_vd", 5)), (("block", "atom"), ("components", "2-shared")), (("block", "atom"), ("components", "2-separate")),
            (("block", "undirected"), ("components", "2-shared")), (("block", "undirected"), ("components", "2-separate")),
            (("d_vd", 5), ("components", "2-shared")), (("d_vd", 5), ("components", "2-separate")),
            (("agg", "attentive"), ("components", "2-shared")), (("agg", "attentive"), ("components", "2-separate"))}
    names = list(sh.FACTORS)
    every = {((a, va), (b, vb)) for i, a in enumerate(names) for b in names[i + 1:] for va in sh.FACTORS[a] for vb in sh.FACTORS[b]}
    assert every - want == gone


def test_the_grid_is_minimal_where_a_case_holds_a_pair_alone():
    """Dropping a case that is the only holder of some pair uncovers that pair: the coverage condition is a condition."""
    holders = {}
    for c in GRID:
        for p in sh.pairs_of(c):
            holders.setdefault(p, []).append(c.index)
    alone = {ix[0] for ix in holders.values() if len(ix) == 1}
    assert alone, "no case holds a pair alone"
    i = min(alone)
    rest = set().union(*[sh.pairs_of(c) for c in GRID if c.index != i])
    assert set(sh.all_pairs()) - rest


def test_the_staged_cases_reach_every_block_kind():
    staged = [c for c in GRID if c.staged]
    assert 4 * len(staged) >= len(GRID) - 3 and {c.block for c in staged} == set(sh.FACTORS["block"])


# ---- refusals -------------------------------------------------------------------------------------------------------------------------
REFUSED = [dict(block="undirected", components="2-shared"), dict(block="undirected", components="2-separate", agg="attentive"),
           dict(block="atom", components="2-separate"), dict(block="atom", components="2-shared", d_vd=5), dict(block="atom", d_vd=5),
           dict(block="atom", d_vd=5, agg="attentive"), dict(components="2-shared", d_vd=5), dict(components="2-separate", d_vd=5, agg="attentive"),
           dict(components="2-shared", agg="attentive"), dict(components="2-separate", agg="attentive", head="ce")]


def _construct(case):
    from chemprop_amd.model import FusedTrainer

    return FusedTrainer(sh.make_model(case, 0), **sh.trainer_flags(case), **sh.optimizer_kwargs(case))


@pytest.mark.parametrize("kw", REFUSED, ids=lambda kw: "-".join(f"{k}={v}" for k, v in kw.items()))
def test_the_trainer_refuses_what_valid_names_before_it_asks_for_a_device(kw):
    case = sh.StepCase(**kw)
    why = sh.valid(case)
    assert why is not None
    rng = torch.get_rng_state()
    with pytest.raises(NotImplementedError) as e:
        _construct(case)
    assert why in str(e.value), (why, str(e.value))
    del rng
    assert {sh.valid(sh.StepCase(**k)) for k in REFUSED} == {
        "undirected blocks in a multicomponent model", "atom blocks in a multicomponent model", "an atom block with atom descriptors (W_d)",
        "atom descriptors (V_ds) in a multicomponent model", "attentive aggregation in a multicomponent model"}


@pytest.mark.parametrize("case", GRID, ids=lambda c: c.id)
def test_the_trainer_takes_every_grid_case_up_to_the_device(case):
    """No grid case is refused: on a CPU model the constructor gets as far as ``_require_device`` (a ``RuntimeError``), and without
    the case's opt-in flag it refuses."""
    from chemprop_amd.model import FusedTrainer

    with pytest.raises(RuntimeError, match="HIP kernels only"):
        _construct(case)
    if sh.trainer_flags(case):
        with pytest.raises(NotImplementedError):
            FusedTrainer(sh.make_model(case, 0))


@pytest.mark.parametrize("pred_head", sh.HEADS)
def test_headspec_pairs_predictors_and_criteria_as_pair_refusal_says(pred_head):
    from chemprop_amd import agg as cagg
    from chemprop_amd.model import MPNN, HeadSpec
    from chemprop_amd.nn import BondMessagePassing

    seen = set()
    for crit_head in sh.HEADS:
        tasks = sh.StepCase(head=pred_head).tasks
        model = MPNN(BondMessagePassing(d_h=8), cagg.MeanAggregation(), sh.make_predictor(pred_head, crit_head, tasks, 8, (6,), "relu"))
        why = sh.pair_refusal(pred_head, crit_head)
        seen.add(why)
        if why is None:
            spec = HeadSpec(model)
            assert spec.kind == sh.StepCase(head=crit_head).kind
        else:
            with pytest.raises(NotImplementedError, match=why):
                HeadSpec(model)
    assert sh.pair_refusal(pred_head, pred_head) is None and len(seen) >= 2


# ---- the reference pinned to the executed reference's goldens -----------------------------------------------------------------------------
GOLDENS = sorted(glob.glob(os.path.join(GOLDEN_DIR, "model", "*.npz")))


def _golden_case(cfg):
    kind = cfg.get("criterion", "mse")
    hidden = cfg["ffn"].get("hidden_dim", 300)
    hidden = tuple(hidden) if isinstance(hidden, (list, tuple)) else (hidden,) * cfg["ffn"].get("n_layers", 1)
    act = cfg["mp"].get("activation", "relu")
    assert not cfg["mp"].get("undirected") and not cfg["mp"].get("d_vd")
    return sh.StepCase(block="bond", act=act, bias=bool(cfg["mp"].get("bias", False)), depth=cfg["mp"].get("depth", 3), agg=cfg["agg"],
                       bn=bool(cfg["bn"]), hidden=hidden, head=kind, optim="plain")


@pytest.mark.parametrize("path", GOLDENS, ids=[os.path.basename(p)[:-4] for p in GOLDENS])
def test_float32_restatement_reproduces_the_goldens_first_step(path):
    """``restate`` in float32 on a golden's own model, batch and targets: the first loss and every first gradient of the executed
    reference, at the bars ``tests/test_model.py`` holds ``oracle.model_torch`` to (1e-6)."""
    from test_model import G, build_mirror

    g = G(path)
    case = _golden_case(g.cfg)
    model = build_mirror(g.cfg).train()
    model.load_state_dict(g.state("w0."))
    targets, weights, lt, gt = g.batch_args()
    inp = dict(bmgs=[g.bmg()], n_mols=g.meta["n_mols"], T=targets, w=weights, lt=None if lt is None else lt.bool(),
               gt=None if gt is None else gt.bool(), X_d=None, V_d=None, clip=None)
    case = dataclasses.replace(case, head=g.cfg.get("criterion", "mse"))
    t = targets.shape[1]
    got = _restate_with_tasks(model, case, inp, t, g.cfg["ffn"].get("n_classes", 0) if case.kind == "ce" else 0,
                               g.cfg["ffn"].get("activation", "relu"))
    loss = float(got["loss"])
    assert abs(loss - float(g.a["loss0"])) <= 1e-6 * max(1.0, abs(loss)), (loss, float(g.a["loss0"]))
    names = [k for k, _ in model.named_parameters()]
    assert names and all("g0." + k in g.a for k in names)
    for k in names:
        assert parity_err(got["g." + k].numpy(), g.a["g0." + k]) <= 1e-6, k
    for k in ("running_mean", "running_var"):
        if case.bn:   # (after ONE step: the golden's own post-step-1 state)
            assert parity_err(got[k].numpy(), g.a["w1.bn." + k]) <= 1e-6, k


def _restate_with_tasks(model, case, inp, t, n_classes, ffn_act):
    """``restate`` for a golden, whose task and class counts are its own: ``tasks`` / ``n_classes`` are what the criterion reads."""
    class _Case:
        def __getattr__(self, k):
            return t if k == "tasks" else n_classes if k == "n_classes" else ffn_act if k == "ffn_act" else getattr(case, k)

    return sh.restate(model, _Case(), inp, torch.float32)


def test_the_goldens_cover_the_nine_configurations():
    assert len(GOLDENS) == 9
    from test_model import G

    assert {G(p).cfg.get("criterion", "mse") for p in GOLDENS} >= {"mse", "mae", "bounded-mse", "bce", "ce", "mve", "evidential", "quantile"}


# ---- the yardstick and the kinks, on every case and step -----------------------------------------------------------------------------------
def test_every_case_carries_its_recorded_seed():
    assert len(sh.SEEDS) == len(GRID) and tuple(c.seed for c in GRID) == sh.SEEDS
    c = GRID[0]
    assert sh.find_seed(c, c.seed) == c.seed and f"-seed{c.seed}" in c.id   # (the search starts where it is told and stops at a usable seed)


@pytest.mark.parametrize("case", GRID, ids=lambda c: c.id)
def test_float32_meets_the_caps_and_stays_off_the_kinks_on_every_step(case):
    """The conditions ``find_seed`` searched for hold at the case's recorded seed: over three CPU steps the float32 restatement is
    under every cap against float64; for ReLU / LeakyReLU no float64 pre-activation of the block or the predictor lies within
    ``delta`` (16 times the largest ``|z32 - z64|`` of the case) of 0; a batch is on the side of the tile its ``graphs`` names; the
    clip bites.  (``find_seed`` asked for 1.25 times the distance and three times the room: float32 sums regroup with the thread count.)"""
    model, inp = sh.build(case)
    assert sh.seed_refusal(case, model, inp, strict=False) is None
    traj = sh.cpu_trajectory(model, case, inp)
    for s, (r64, r32, p64, p32) in enumerate(traj):
        e32 = sh.yardstick(r64, r32)
        for k, e in e32.items():
            assert e < sh.cap_of(k), (s, k, e)
        for k in p64:
            assert sh._err(p32[k], p64[k])[0] < sh.CAP["param"], (s, k)
        if case.act in sh.KINKED:
            lo, delta = sh.kink_clearance(r64, r32)
            assert lo >= delta > 0, (s, lo, delta)
        assert set(r64["scales"]) == set(sh.zero_gradients(case))
        for k, scale in r64["scales"].items():   # (zero in exact arithmetic: float64 leaves rounding noise)
            assert float(r64["g." + k].abs().max()) <= 1e-12 * scale, (k, float(r64["g." + k].abs().max()), scale)
    if inp["clip"] is not None:   # the clip changes the first step's gradients
        free = sh.restate(model, case, dict(inp, clip=None), torch.float64)
        assert any(not torch.equal(free[k], traj[0][0][k]) for k in free if k.startswith("g."))


def test_bias_corrections_come_from_the_float32_betas():
    """``k_adam`` holds the betas as float32 and forms ``1.f - beta`` itself: the host's bias corrections are formed from the same
    numbers, so that at step 1 ``(1 - beta) / (1 - beta^1)`` is 1 for both moments (the GPU file has the regression this closes)."""
    import ctypes

    from chemprop_amd.optim import bias_corrections

    for betas in (sh.BETAS, (0.8, 0.99), (0.5, 0.75)):
        b1, b2 = (ctypes.c_float(b).value for b in betas)
        for k in (1, 2, 7):
            bc1, sbc2 = bias_corrections(betas, k)
            assert bc1 == 1.0 - b1 ** k and sbc2 == (1.0 - b2 ** k) ** 0.5
        assert bias_corrections(betas, 1) == (1.0 - b1, (1.0 - b2) ** 0.5)
    assert abs(bias_corrections(sh.BETAS, 1)[1] ** 2 / 1e-3 - 1) > 1e-5   # (the float32 0.999 is not the double's)
