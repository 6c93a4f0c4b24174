"""``dmpnn_head`` (``csrc/dmpnn_head.hip``) through the C ABI at the edges of its dispatch: every output of the call — loss, raw
predictions, ``dl/dH_v``, every ``gW[l]`` / ``gb[l]``, the batch-norm gradients, the running statistics — against a float64
restatement on the CPU in a metric WITHOUT a floor, ``max|got - ref| / max|ref|`` (``conftest.parity_err_unfloored``).

Why: the loss is a mean over the batch, so the head's gradients are tiny (``max|dl/dH_v|`` ~ 1e-4 at 512 molecules) and the floored
bar of 2e-5 the other head tests hold is an ABSOLUTE one there — ``dl/dH_v`` could be wrong by 16 % and pass.

The bar is what float32 itself does: ``head_harness.yardstick`` runs the same restatement in float32 on the CPU, ``e32_k`` is its
unfloored error against float64 for output ``k`` of that very case, and the kernels are held to
``err_k <= min(MARGIN * max(e32_k, 2**-23), cap_k)`` with the caps the floored bars of the suite (1e-5 loss, 2e-5 predictions and
gradients, 1e-6 running statistics).  MARGIN is one number for the module: the worst ``err_k / max(e32_k, 2**-23)`` observed on the
MI355X over every case and tensor, doubled (row blocks of 16, quads, the 3-term f16 split of W0 sum in other orders than torch)
and rounded up to a power of two.

Measured on the MI355X over the 302 GPU tests of this module (2 854 tensor comparisons): the worst ``err_k / max(e32_k, 2**-23)`` is
8.39 — ``gb1`` of ``chain-at-size-B512-mean`` (7.05 on the row form of the same case): the output bias gradient of a one-task head is
ONE number, a cancelling sum of 512 signed residuals, err 1.3e-6 against a float32 draw of 1.6e-7; the next are 4.28 (``gb0``, a
head without hidden layer) and 3.86 (predictions at 511 molecules); per kind of tensor: weight / bias gradients 8.39, predictions
3.86, batch-norm weight gradient 3.38, ``dl/dH_v`` 2.67, batch-norm bias gradient 2.61, loss 2.22, running mean 1.55, running
variance 1.45 — none stands out by an order of magnitude.  2 x 8.39 = 16.8 -> MARGIN = 32.  With ``e32`` of 2e-7 .. 5e-7 on the
gradients that is a relative bar of ~1e-5 where the floored one allowed 16 % on ``dl/dH_v`` at 512 molecules.
Wall time of the module's GPU tests on the MI355X: 5.6 s (9.3 s on a cold box); ``tests/test_model.py`` on the same box: 7.7 s.

Which form runs is pinned: ``rows-*`` cases under ``DMPNN_HEAD=rows`` (a shape that would fall to the chain is an error there),
``chain-*`` under ``DMPNN_HEAD=chain``, ``default-*`` without the variable (the size rules decide: the boundary pairs).  ``cols-*``
are default cases the row kernel does not take (5 outputs) on at most 1 024 molecules: the column kernels around the chain's
predictor.  The inputs are kink-free by construction (``head_harness.build_inputs``: hidden biases shifted off the ReLU masks,
target seeds advanced off ``|y - p| = 0``), asserted on the CPU; no element is excluded from any comparison.

Left out: ``n_atoms * ld >= 2**29`` (the 32-bit offset guard of ``cols_fused``) needs a 2 GB input.
"""
import dataclasses
import functools

import pytest
import torch

import head_harness as hh
from head_harness import HeadCase

MARGIN = 32.0


# ---- the shape list ---------------------------------------------------------------------------------------------------------------
# flavours: activation, aggregation, batch norm, criterion — one per boundary GROUP, so a pair "last inside / first outside" differs in
# nothing else; every flavour is one the row form implements (MSE / MAE / BCE, bounded or not)
FLAVOURS = [
    dict(act="relu", agg="mean", bn=True, kind="mse"),
    dict(act="leakyrelu", agg="sum", bn=True, kind="mae"),
    dict(act="tanh", agg="norm", bn=False, kind="bce"),
    dict(act="elu", agg="mean", bn=True, kind="mse", bounded=True),
    dict(act="relu", agg="norm", bn=False, kind="mae", bounded=True),
    dict(act="leakyrelu", agg="sum", bn=True, kind="bce"),
    dict(act="relu", agg="norm", bn=True, kind="mse"),
]
ROWS_MAX_B, ROWS_MAX_W = 1024, 320   # kRowsMaxB, kRowsMaxWidth


def _case(form, name, B=100, d_h=64, hidden=(36,), tasks=2, **kw):
    return HeadCase(f"{form}-{name}", form, B, d_h, tuple(hidden), tasks, **kw)


def _rows_ok(B, d_h, hidden, tasks, d_xd=0):
    return (len(hidden) == 1 and tasks <= 4 and B <= ROWS_MAX_B and d_h <= ROWS_MAX_W and hidden[0] <= ROWS_MAX_W
            and d_h + d_xd <= (512 if d_xd else ROWS_MAX_W) and (d_h + d_xd) % 4 == 0)


def _build_cases():
    cs = []

    def sweep(groups, name, fixed, forms=("rows", "chain", "default")):
        for gi, group in enumerate(groups):
            for v in group:
                for form in forms:
                    kw = dict(FLAVOURS[gi % len(FLAVOURS)], **fixed(v))
                    full = dict(B=100, d_h=64, hidden=(36,), tasks=2)
                    full.update({k: kw[k] for k in full if k in kw})
                    if form == "rows" and not _rows_ok(full["B"], full["d_h"], full["hidden"], full["tasks"]):
                        continue
                    cs.append(_case(form, f"{name}{v}", **kw))

    # molecules per batch: HeadRoute::qpw (256), kFuseAggMols and k_bn_fwd/bwd<REG> (512), kRowsMaxB / kOutAllMaxRows (1 024), row blocks of 16,
    # the row-split weight gradients (2 048)
    B_GROUPS = [(2,), (15, 16, 17), (255, 256, 257), (511, 512, 513), (1009,), (1023, 1024, 1025), (2047, 2048, 2049)]
    sweep(B_GROUPS, "B", lambda v: dict(B=v))
    # the same edges on the column kernels around the chain's predictor (5 outputs: k_loss, the generic output layer)
    sweep([(16, 17), (255, 256, 257), (511, 512, 513), (1023, 1024, 1025)], "B", lambda v: dict(B=v, tasks=5), forms=("cols",))
    # the block's width: k_head_rows<2, .> / <5, .> (128), kRowsMaxWidth (320), 64-column slices, 16-column tiles
    sweep([(4,), (60, 64, 68), (124, 128, 132), (300,), (316, 320, 324)], "dh", lambda v: dict(d_h=v))
    sweep([(60, 64, 68), (316, 320, 324)], "dh", lambda v: dict(d_h=v, tasks=5), forms=("cols",))
    # d_h % 4 != 0: no column kernels — k_bn_fwd/bwd<true | false> and the row aggregation kernels on both sides of 512 molecules
    for B in (100, 600):
        for d_h in (30, 301):
            for form, fl in (("default", 0), ("chain", 1)):
                cs.append(_case(form, f"dh{d_h}-B{B}", B=B, d_h=d_h, **FLAVOURS[fl]))
    # the hidden layer's width (odd widths included)
    sweep([(1, 2), (15, 16, 17), (36,), (63, 64, 65), (127, 128, 129), (300,), (319, 320, 321)], "N", lambda v: dict(hidden=(v,)))
    # outputs: kOutMaxTasks (4 | 5): the dot-product output layer / k_out_all against the generic contraction / k_loss
    sweep([(1,), (2, 3), (4, 5), (12,)], "out", lambda v: dict(tasks=v, missing="none" if v == 1 else "some"))
    for form in ("chain", "default"):
        for nc in (2, 3):
            cs.append(_case(form, f"ce{nc}", kind="ce", n_classes=nc, act="relu"))
        for kind in ("mve", "quantile", "evidential"):
            for t in (1, 3):
                cs.append(_case(form, f"{kind}-t{t}", kind=kind, tasks=t, act="leakyrelu" if t == 1 else "elu", agg="norm"))
        # every criterion of k_out_all's kind in k_loss as well (5 outputs)
        for gi, fl in enumerate(FLAVOURS[:6]):
            cs.append(_case(form, f"kloss-{fl['kind']}{'-bounded' if fl.get('bounded') else ''}-{fl['act']}", tasks=5, **fl))
        # linear layers: 1 (no hidden layer), 3, DMPNN_MAX_FFN_LAYERS (2 is everywhere else)
        for hidden, act in (((), "relu"), ((36, 20), "relu"), ((36, 20), "tanh"), ((40, 36, 33, 32, 20, 17, 16), "leakyrelu"), ((36,) * 7, "elu")):
            cs.append(_case(form, f"layers{len(hidden) + 1}-{act}", hidden=hidden, act=act))
    # ragged batch vectors: empty molecules (start, middle, behind batch[-1]), single atoms, one molecule with most of the atoms;
    # n_atoms == n_mols; more than 32 768 atoms (k_mol_bounds in several blocks)
    for form, B in (("rows", 100), ("rows", 600), ("chain", 100), ("chain", 600), ("cols", 100), ("cols", 600), ("default", 100)):
        t = 5 if form == "cols" else 2
        for agg in ("mean", "sum"):   # (sum: without batch norm — a 1 700-term fp32 sum in ONE row would own the column's variance)
            cs.append(_case(form, f"ragged-{agg}-B{B}", B=B, tasks=t, layout="ragged", agg=agg, act="relu", bn=agg != "sum"))
        cs.append(_case(form, f"one-each-B{B}", B=B, tasks=t, layout="one-each", agg="mean", act="leakyrelu"))
    cs.append(_case("default", "huge-B1000", B=1000, layout="huge", agg="norm"))
    cs.append(_case("cols", "huge-B1000", B=1000, tasks=5, layout="huge", agg="mean"))
    cs.append(_case("chain", "huge-B1000", B=1000, layout="huge", agg="mean"))
    # the template instances the size rules do not pick
    for qpw, B in (("4", 600), ("4", 1024), ("2", 100), ("2", 256)):
        cs.append(_case("rows", f"qpw{qpw}-B{B}", B=B, env=(("DMPNN_HEAD_QPW", qpw),)))
    for aggenv, B in (("fused", 1000), ("split", 100)):
        cs.append(_case("rows", f"agg-{aggenv}-B{B}", B=B, agg="sum", env=(("DMPNN_HEAD_AGG", aggenv),)))
    # targets: a task column without a finite target, no finite target at all
    for form in ("rows", "chain", "cols"):
        cs.append(_case(form, "dead-task", tasks=5 if form == "cols" else 3, missing="dead"))
        cs.append(_case(form, "no-target", tasks=5 if form == "cols" else 2, missing="all"))
    cs.append(_case("chain", "dead-task-ce", kind="ce", n_classes=3, tasks=2, missing="dead"))
    cs.append(_case("chain", "dead-task-mve", kind="mve", tasks=2, missing="dead", act="elu"))
    # inference (batch norm on its running statistics), the loss alone, frozen first layer, constant columns under batch norm
    for form, B in (("default", 100), ("chain", 100), ("default", 2000), ("default", 600)):
        cs.append(_case(form, f"infer-B{B}", B=B, mode="infer"))
        cs.append(_case(form, f"eval-loss-B{B}", B=B, mode="eval-loss"))
    for form in ("rows", "chain", "cols"):
        cs.append(_case(form, "frozen", tasks=5 if form == "cols" else 2, frozen=True))
        cs.append(_case(form, "const-col", tasks=5 if form == "cols" else 2, const_col=True, agg="mean"))
    # molecule descriptors: kRowsMaxK (512 | 516), dims[0] % 4 (76 | 77)
    for form in ("rows", "default", "chain"):
        for d_xd in (212, 216):
            if form != "rows" or d_xd == 212:
                cs.append(_case(form, f"xd{d_xd}", d_h=300, d_xd=d_xd, hidden=(64,)))
    for d_xd in (12, 13):
        cs.append(_case("default", f"xd{d_xd}", d_xd=d_xd))
    # the default head at size (d_h 300, one hidden layer of 300, one task)
    for B, agg in ((512, "norm"), (512, "mean"), (1000, "mean"), (77, "sum")):
        for form in ("rows", "chain"):
            cs.append(_case(form, f"at-size-B{B}-{agg}", B=B, d_h=300, hidden=(300,), tasks=1, agg=agg, missing="none"))
    cs.append(_case("default", "at-size-B2048-norm", B=2048, d_h=300, hidden=(300,), tasks=1, agg="norm", missing="none"))
    out = []
    for c in cs:   # `cols`: the default dispatch on a shape the row form does not take
        if c.form == "cols":
            assert not _rows_ok(c.B, c.d_h, c.hidden, c.tasks, c.d_xd) and c.B <= ROWS_MAX_B + 1, c.id
            c = dataclasses.replace(c, form="default", id=c.id)
        out.append(c)
    assert len({c.id for c in out}) == len(out), "case ids must be unique"
    return out


CASES = _build_cases()
IDS = [c.id for c in CASES]


@functools.lru_cache(maxsize=4)
def prepared(case):
    inp = hh.build_inputs(case)
    ref, e32 = hh.yardstick(case, inp)
    return inp, ref, e32


# ---- no GPU: the inputs and the yardstick -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_case_inputs_are_kink_free_and_float32_meets_the_caps(case):
    """Every case's inputs on the CPU: the kink assertions of ``build_inputs`` hold, the float64 reference is finite (the loss is NaN
    exactly when no target is finite) and plain float32 PyTorch itself stays within the capped bars against it — so the bar
    ``MARGIN * e32`` is one a correct fp32 kernel can meet."""
    inp, ref, e32 = prepared(case)
    if case.act in hh.KINKED_ACT and case.hidden:
        assert len(inp["z_delta"]) == len(case.hidden)
    for k in hh.output_names(case):
        if case.missing == "all" and k != "preds" and not k.startswith("running"):
            assert not torch.isfinite(ref[k]).any() if k == "loss" else True
            continue
        assert torch.isfinite(ref[k]).all(), k
        assert e32[k] <= hh.cap_of(k), (k, e32[k])
    if case.mode == "train" and case.missing != "all":
        assert float(ref["gHv"].abs().max()) > 0


def test_the_shape_list_holds_every_boundary_pair():
    """Each rule of the dispatch has its last value inside and its first value outside in the list, everything else equal."""
    by_id = {c.id: c for c in CASES}

    def same_but(a, b, field):
        ca, cb = by_id[a], by_id[b]
        da, db = dataclasses.asdict(ca), dataclasses.asdict(cb)
        for k in ("id", field):
            da.pop(k), db.pop(k)
        return da == db

    for form in ("chain", "default"):
        for a, b in ((16, 17), (256, 257), (512, 513), (1024, 1025), (2048, 2049)):
            assert same_but(f"{form}-B{a}", f"{form}-B{b}", "B")
        for a, b in ((128, 132), (320, 324)):
            assert same_but(f"{form}-dh{a}", f"{form}-dh{b}", "d_h")
        for a, b in ((16, 17), (64, 65), (128, 129), (320, 321)):
            assert same_but(f"{form}-N{a}", f"{form}-N{b}", "hidden")
        assert same_but(f"{form}-out4", f"{form}-out5", "tasks")
    for a, b in ((16, 17), (256, 257), (512, 513), (1023, 1024)):
        assert same_but(f"rows-B{a}", f"rows-B{b}", "B")
    assert same_but("rows-dh128", "rows-dh132", "d_h") and same_but("rows-N128", "rows-N129", "hidden")
    assert "rows-dh324" not in by_id and "rows-N321" not in by_id and "rows-B1025" not in by_id and "rows-out5" not in by_id
    assert same_but("default-xd212", "default-xd216", "d_xd") and same_but("default-xd12", "default-xd13", "d_xd")
    for form in ("rows", "chain"):
        assert {c.act for c in CASES if c.form == form} >= {"relu", "leakyrelu", "tanh", "elu"}
        assert {c.agg for c in CASES if c.form == form} == {"mean", "sum", "norm"}
        assert {(c.kind, c.bounded) for c in CASES if c.form == form} >= {("mse", False), ("mae", False), ("bce", False), ("mse", True), ("mae", True)}
        assert {c.bn for c in CASES if c.form == form} == {True, False}
    assert {c.kind for c in CASES if c.form == "chain"} == set(hh.PER_TASK)


# ---- GPU ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_head_matches_float64_within_the_float32_yardstick(case, gpu_device):
    inp, ref, e32 = prepared(case)
    got = hh.run_case(case, inp, gpu_device)
    fails = hh.compare(case, got, ref, e32, MARGIN)
    if case.bn:
        want = 5 + (1 if case.mode != "infer" else 0)
        if int(got["num_batches_tracked"]) != want:
            fails.append(f"num_batches_tracked {int(got['num_batches_tracked'])} != {want}")
        if case.mode == "infer":   # (eval mode leaves the running statistics alone)
            for k in ("running_mean", "running_var"):
                if not torch.equal(got[k], inp[k]):
                    fails.append(f"{k} changed by an inference call")
    if case.mode != "infer" and got["n_finite"] != float(inp["T"].isfinite().sum()):
        fails.append(f"loss_out[1] = {got['n_finite']}: not the number of finite targets")
    assert not fails, f"{case.id}: " + "; ".join(fails)


@pytest.mark.gpu
@pytest.mark.parametrize("name,shape", [("dh324", dict(d_h=324)), ("B1025", dict(B=1025)), ("N321", dict(hidden=(321,))), ("out5", dict(tasks=5)),
                                        ("dh30", dict(d_h=30)), ("layers3", dict(hidden=(36, 20))), ("ce", dict(kind="ce", n_classes=2))])
def test_rows_form_refuses_the_first_value_outside_each_rule(name, shape, gpu_device):
    """``DMPNN_HEAD=rows`` on the first shape outside each rule of ``rows_shape``: an error, not a silent chain — so the ``rows-*``
    cases above did run the row kernels."""
    case = _case("rows", name, **shape)
    with pytest.raises(RuntimeError, match="DMPNN_HEAD=rows"):
        hh.run_case(case, hh.build_inputs(case), gpu_device)


def _by_id(cid):
    return next(c for c in CASES if c.id == cid)


CROSS = [   # (case, environment A, environment B, identical arithmetic promised)
    ("rows-B16", dict(DMPNN_HEAD="rows"), dict(DMPNN_HEAD="chain"), False),
    ("rows-B257", dict(DMPNN_HEAD="rows"), dict(DMPNN_HEAD="chain"), False),
    ("rows-B513", dict(DMPNN_HEAD="rows"), dict(DMPNN_HEAD="chain"), False),
    ("rows-B1024", dict(DMPNN_HEAD="rows"), dict(DMPNN_HEAD="chain"), False),
    ("rows-dh132", dict(DMPNN_HEAD="rows"), dict(DMPNN_HEAD="chain"), False),
    ("rows-N320", dict(DMPNN_HEAD="rows"), dict(DMPNN_HEAD="chain"), False),
    ("rows-at-size-B512-norm", dict(DMPNN_HEAD="rows"), dict(DMPNN_HEAD="chain"), False),
    ("rows-B256", dict(DMPNN_HEAD_QPW="4"), dict(DMPNN_HEAD_QPW="2"), False),
    ("rows-B512", dict(DMPNN_HEAD_QPW="4"), dict(DMPNN_HEAD_QPW="2"), False),
    ("rows-B1024", dict(DMPNN_HEAD_QPW="4"), dict(DMPNN_HEAD_QPW="2"), False),
    ("rows-B512", dict(DMPNN_HEAD_AGG="fused"), dict(DMPNN_HEAD_AGG="split"), False),
    ("rows-ragged-sum-B600", dict(DMPNN_HEAD_AGG="fused"), dict(DMPNN_HEAD_AGG="split"), False),
    # without batch norm the aggregate feeds the predictor as it is: k_agg_bn_fwd and dmpnn_molagg_fwd promise the same sequential sums
    ("default-B257", dict(DMPNN_HEAD_AGG="fused"), dict(DMPNN_HEAD_AGG="split"), True),
    ("default-B1009", dict(DMPNN_HEAD_AGG="fused"), dict(DMPNN_HEAD_AGG="split"), True),
]


@pytest.mark.gpu
@pytest.mark.parametrize("cid,env_a,env_b,exact", CROSS, ids=[f"{c[0]}-{'-'.join(c[1].values())}-vs-{'-'.join(c[2].values())}" for c in CROSS])
def test_forms_and_instances_agree_without_a_floor(cid, env_a, env_b, exact, gpu_device):
    """Two forms / template instances on one boundary shape: every output of A against B unfloored, within the bar of the float32
    yardstick (``MARGIN * e32``, capped); bit for bit where the code promises identical arithmetic."""
    case = _by_id(cid)
    assert not exact or not case.bn
    inp, ref, e32 = prepared(case)
    a, b = hh.run_case(case, inp, gpu_device, env_a), hh.run_case(case, inp, gpu_device, env_b)
    if exact:
        for k in hh.output_names(case):
            assert torch.equal(a[k], b[k]), k
        return
    fails = hh.compare(dataclasses.replace(case, id=case.id + "/cross"), a, {k: v.double() for k, v in b.items() if torch.is_tensor(v)}, e32, MARGIN)
    assert not fails, f"{cid}: " + "; ".join(fails)


@pytest.mark.gpu
@pytest.mark.parametrize("form,tasks,B", [("rows", 2, 100), ("chain", 2, 100), ("chain", 5, 100), ("chain", 2, 1100)])
@pytest.mark.parametrize("kind", ["mse", "mae"])
def test_bounded_criteria_at_equality_use_the_strict_comparisons(kind, form, tasks, B, gpu_device):
    """``p == y`` exactly on every entry (output weights 0, output bias = the task's target, both masks set everywhere): the
    reference's ``p < y`` / ``p > y`` are strict, so nothing is clamped, the loss is 0 and every gradient is EXACTLY 0 — in the row
    kernel, ``k_out_all`` (<= 4 outputs, <= 1 024 molecules) and ``k_loss``."""
    case = _case(form, f"equal-{kind}", B=B, tasks=tasks, kind=kind, bounded=True, missing="none", act="tanh")
    inp = hh.build_inputs(case)
    y = torch.tensor([0.75, -1.5, 0.375, 2.0, -0.0625])[:tasks]
    inp["W1"], inp["b1"] = torch.zeros_like(inp["W1"]), y.clone()
    inp["T"] = y.expand(B, tasks).contiguous()
    inp["lt"] = inp["gt"] = torch.ones(B, tasks, dtype=torch.bool)
    ref = hh.reference(case, inp)
    assert float(ref["loss"]) == 0.0 and all(float(ref[k].abs().max()) == 0.0 for k in hh.output_names(case) if k.startswith("g"))
    got = hh.run_case(case, inp, gpu_device)
    assert torch.equal(got["preds"], inp["T"])
    assert float(got["loss"]) == 0.0
    for k in hh.output_names(case):
        if k.startswith("g"):
            assert bool((got[k] == 0).all()), k
