"""``dmpnn_head`` with ``DMPNN_LOSS_SID`` / ``DMPNN_LOSS_WASSERSTEIN`` through the C ABI: one training call per case (every output
prefilled with NaN) against the head restated op by op on the CPU — in float64 as the reference, in float32 as the yardstick (the
scheme of ``tests/test_dirichlet_head_gpu.py``: ``head_harness.build_inputs`` / ``run_case`` / ``compare`` through ``SpectralCase``;
the criterion is ``tests/test_spectral_head.py``'s restatement of ``include/dmpnn.h``).  ``run_case`` knows nothing of
``spectral_act`` / ``spectral_threshold``: ``spectral_fields`` presets them on the ``HeadArgs`` it creates.

The kernel's constants (``csrc/dmpnn_head_kernels.hpp``): ``kSpecCols = 256`` columns per pass = threads per workgroup, four waves
of 64; ONE molecule row per workgroup (no packing of rows, so no row-count boundary).  ``test_the_shapes_straddle_the_kernels_
boundaries`` reads ``kSpecCols`` from the source and asserts the shapes lie one below, at and one above it and the wave.

Cases ``(t, B)``: (1, 3) — loss and gradients analytically 0: every gradient at the absolute bar ``MARGIN 2**-23 sum|w tw| / sum m``
— (2, 3), (63 | 64 | 65, 5), (255 | 256 | 257, 3), (130, 37), (1801, 9), each for both criteria, without and with a hidden layer of
20 (batch norm on, tanh, row and task weights, strictly positive targets renormalised over their finite entries, 20 % missing).
Missing targets at (65, 5) and (257, 3): none, first column, last column, a middle column (``task``: for SID without a threshold the
output layer's row of that task has a gradient of exactly 0 in the kernel — held at the absolute bar — for Wasserstein it has not),
all (NaN loss on both sides).  Ranges at (65, 5) and (257, 3): the output layer rescaled to a raw standard deviation of 8 and 25
for softplus, 1 and 4 for exp, and exp with the raw outputs shifted by +100.  Threshold ``0.5 / t`` at (2, 3), (65, 5) and (257, 3:
two passes), softplus and exp: between 10 % and 90 % of the entries clamped, none within 1e-3 relative of the threshold (asserted on
the CPU; the input seed advances until it holds — among the 16 209 entries of (1801, 9) one always lies that close).  One
attentive and one two-component case.  The ABI has no row stride for ``targets``; ``test_a_strided_targets_view`` hands a view into
a wider table through the harness, which makes it contiguous.

Bar per output tensor: ``err <= min(MARGIN max(e32, 2**-23), cap)``, the caps ``head_harness.CAP``; ``prepared`` asserts on the
CPU, before a device is touched, that the float32 restatement alone stays within ``cap / 8`` for every compared tensor of every case
(the input seed advances up to 8 times until it does).  No element is left out.

The shifted cases: raw outputs ``100 + N(0, 1)`` per column from an output layer with zero weights and that bias, so that every
side — float64, float32, the device — starts from the very same ``x``; what is held is the criterion at ``x ~ 100`` (``exp(x)`` alone
overflows float32 beyond 88.7).  Through an output layer with weights the shift does not reach the criterion intact: the
contraction kernel starts its accumulators from the bias, so a raw output near 100 takes a rounding of 2**-18 per accumulation step
(measured: ``preds`` 3.0e-5 absolute off float64, eight times plain float32's 3.8e-6 — inside that tensor's own bar at a ratio of
3.0), ``exp`` turns that into a relative error of ``p``, and the gradients came out 6.0e-6 .. 5.9e-5 off, 3 .. 17 times the float32
restatement's own 1.2e-6 .. 7.1e-6 and above the cap of 2e-5 in 5 of 8 such cases.  That is the contraction kernel's term, not the
criterion's; its accumulation order is not this feature's to change.

MARGIN, measured on the MI355X with 32 — the value ``tests/test_head_boundaries.py`` holds — over the 158 GPU tests of this module
(1 395 comparisons with a ratio; every line in ``profiles/spectral_head_bars.txt``): the worst ``err / max(e32, 2**-23)`` is 4.93 —
``gHv`` of ``wasserstein-t255-B3-linear-some-softplus-std1`` (err 3.1e-6 against a float32 draw of 6.2e-7: the weighted signs of
the running sums, one rounding away from torch's ``cumsum`` order) — then 3.30 (the loss of ``wasserstein-t257-B3-hidden-some-exp-
std4``) and 3.24 (``gHv`` of ``wasserstein-t257-B3-linear-some-exp-std1``).  Per kind of tensor: ``dl/dH_v`` 4.93, loss 3.30,
batch-norm gradients 2.88, weight / bias gradients 2.86, predictions 1.77, running mean 1.16, running variance 0.48, the attention's
weight gradient 0.46.  Per family: Wasserstein 4.93, SID 2.88; the 20 %-missing shapes 4.93, exp 3.30, a missing task 2.88, std 25
2.86, the +100 shift 2.67, first column missing 2.46, threshold 2.33, std 8 2.27, none missing 2.17, last column missing 2.14, two
components 1.56, attentive 1.33.  No ratio comes near 16; 2 x 4.93 = 9.9 -> MARGIN = 16, half of the 32 the other criteria hold.
"""
import contextlib
import dataclasses
import functools
import re
from pathlib import Path

import pytest
import torch

import attn_harness as ah
import head_harness as hh
from chemprop_amd import _lib
from conftest import parity_err_unfloored
from head_harness import HeadCase
from test_spectral_head import spectral_criterion, spectral_p, spectral_targets

MARGIN = 16.0

SPEC_COLS, WAVE = 256, 64


@dataclasses.dataclass(frozen=True)
class SpectralCase(HeadCase):
    """A ``HeadCase`` of kind ``sid`` / ``wasserstein``: one output per task.  ``sact``: ``softplus`` / ``exp``; ``thr``: the
    criterion's threshold or ``None``; ``scale``: the standard deviation the raw outputs are rescaled to; ``shift``: added to the
    raw outputs (the module's docstring says how).  ``missing``: ``test_spectral_head.spectral_targets``'s."""
    sact: str = "softplus"
    thr: float = None
    scale: float = 1.0
    shift: float = 0.0

    @property
    def per_task(self):
        return 1


def _crit(case, Y, T, w, tw, lt=None, gt=None, **_):
    return spectral_criterion(case.kind, Y, T, w, tw, case.sact, case.thr)


@contextlib.contextmanager
def spectral_reference():
    """``head_harness.reference`` (and what calls it) with the spectral restatement for the cases of this file."""
    orig = hh.criterion
    hh.criterion = lambda case, *a, **kw: (_crit if case.kind in ("sid", "wasserstein") else orig)(case, *a, **kw)
    try:
        yield
    finally:
        hh.criterion = orig


@contextlib.contextmanager
def spectral_fields(case):
    """``_lib.HeadArgs()`` — as ``run_case`` creates it — with ``spectral_act`` / ``spectral_threshold`` of ``case`` already set."""
    orig = _lib.HeadArgs

    def make():
        h = orig()
        h.spectral_act, h.spectral_threshold = _lib.SPECTRAL_ACT[case.sact], float(case.thr or 0.0)
        return h

    _lib.HeadArgs = make
    try:
        yield
    finally:
        _lib.HeadArgs = orig


def run(case, inp, dev, env=None):
    with spectral_fields(case):
        return hh.run_case(case, inp, dev, env)


SHAPES = [(1, 3), (2, 3), (63, 5), (64, 5), (65, 5), (SPEC_COLS - 1, 3), (SPEC_COLS, 3), (SPEC_COLS + 1, 3), (130, 37), (1801, 9)]
KINDS = ("sid", "wasserstein")


def _case(kind, t, B, hidden, missing="some", sact="softplus", thr=None, scale=1.0, shift=0.0, tag=""):
    name = f"{kind}-t{t}-B{B}-{'hidden' if hidden else 'linear'}-{missing}-{sact}-std{scale:g}" + ("-thr" if thr else "") + ("-shift" if shift else "") + tag
    return SpectralCase(name, "default", B, 24, hidden, t, kind=kind, act="tanh", agg="mean", bn=True, missing=missing, sact=sact, thr=thr,
                        scale=scale, shift=shift)


def _build_cases():
    cs = []
    for kind in KINDS:
        for hidden in ((), (20,)):
            for t, B in SHAPES:
                cs.append(_case(kind, t, B, hidden, missing="some" if t > 1 else "none"))
            for t, B in ((65, 5), (SPEC_COLS + 1, 3)):
                for missing in ("none", "first", "last", "task", "all"):
                    cs.append(_case(kind, t, B, hidden, missing=missing))
            cs.append(_case(kind, 1, 3, hidden, missing="all"))
            # (shapes of a few hundred entries: at a standard deviation of 25 the smallest of thousands of raw outputs lies below -87, where
            #  softplus — and with it p — leaves float32's normal range and SID's log(q) has no digits left on either side)
            for t, B in ((65, 5), (SPEC_COLS + 1, 3)):
                for sact, scale, shift in (("softplus", 8.0, 0.0), ("softplus", 25.0, 0.0), ("exp", 1.0, 0.0), ("exp", 4.0, 0.0), ("exp", 1.0, 100.0)):
                    cs.append(_case(kind, t, B, hidden, sact=sact, scale=scale, shift=shift))
            for t, B in ((2, 3), (65, 5), (SPEC_COLS + 1, 3)):   # (at 1801 x 9 entries some p always lies within 1e-3 of the threshold)
                for sact in ("softplus", "exp"):
                    cs.append(_case(kind, t, B, hidden, sact=sact, thr=0.5 / t))
    return cs


CASES = _build_cases()
IDS = [c.id for c in CASES]
assert len(set(IDS)) == len(IDS)


def test_the_shapes_straddle_the_kernels_boundaries():
    src = (Path(__file__).resolve().parents[1] / "chemprop_amd" / "csrc" / "dmpnn_head_kernels.hpp").read_text()
    assert int(re.search(r"constexpr int kSpecCols = (\d+);", src).group(1)) == SPEC_COLS
    assert "dim3((unsigned)h.n_mols), dim3(kSpecCols)" in (Path(__file__).resolve().parents[1] / "chemprop_amd" / "csrc" / "dmpnn_head.hip").read_text()   # (one row per workgroup)
    ts = {c.tasks for c in CASES}
    assert {WAVE - 1, WAVE, WAVE + 1, SPEC_COLS - 1, SPEC_COLS, SPEC_COLS + 1} <= ts and max(ts) > 4 * SPEC_COLS and {1, 2} <= ts
    assert all(c.thr is None or c.tasks >= 2 for c in CASES)


def _rescale_output_layer(case, inp, raw):
    last = len(case.dims) - 2
    s = case.scale / float(raw.double().std()) if raw.numel() > 1 and float(raw.double().std()) > 0 else 1.0
    inp[f"W{last}"], inp[f"b{last}"] = (inp[f"W{last}"].double() * s).float(), (inp[f"b{last}"].double() * s).float()


def _within_an_eighth_of_the_caps(cid, names, e32, ref):
    for k in names:
        if not bool(torch.isfinite(ref[k]).all()):
            continue   # (no finite target: a NaN loss and NaN gradients on both sides)
        if float(ref[k].abs().max()) == 0.0 or (k != "preds" and "-t1-" in cid):
            continue   # (t = 1: loss and gradients analytically 0 — held to the absolute bar, not to a relative one)
        assert e32[k] <= hh.cap_of(k) / 8, (cid, k, e32[k])


def _threshold_splits_the_entries(case, ref, inp):
    p = spectral_p(ref["preds"], case.sact)
    clamped = float((p < case.thr).double().mean())
    assert 0.1 <= clamped <= 0.9, (case.id, clamped)
    assert float(((p - case.thr).abs() / case.thr).min()) > 1e-3, case.id


@functools.lru_cache(maxsize=None)
def prepared(case):
    """The inputs (spectral targets, the output layer rescaled and shifted), the float64 reference and the float32 yardstick; the
    conditions on the inputs are asserted here, on the CPU: the input seed advances (up to 8 times) until they hold."""
    for seed in range(case.seed, case.seed + 8):
        inp = hh.build_inputs(dataclasses.replace(case, kind="mse", seed=seed, missing="some"))
        inp["T"] = spectral_targets(case.B, case.tasks, case.missing, seed)
        with spectral_reference():
            if case.shift:   # (the module's docstring: zero weights, the bias 100 + N(0, scale) — the same x on every side)
                last = len(case.dims) - 2
                inp[f"W{last}"] = torch.zeros_like(inp[f"W{last}"])
                inp[f"b{last}"] = (case.shift + case.scale * torch.randn(case.tasks, generator=torch.Generator().manual_seed(31 + seed))).float()
            elif case.tasks > 1:
                _rescale_output_layer(case, inp, hh.reference(dataclasses.replace(case, mode="eval-loss"), inp)["preds"])
            ref, e32 = hh.yardstick(case, inp)
        try:
            if case.tasks > 1 and not case.shift:
                assert abs(float(ref["preds"].std()) - case.scale) <= 1e-3 * case.scale
            if case.thr:
                _threshold_splits_the_entries(case, ref, inp)
            _within_an_eighth_of_the_caps(case.id, hh.output_names(case), e32, ref)
            break
        except AssertionError:
            if seed == case.seed + 7:
                raise
    inp["input_seed"] = seed
    return inp, ref, e32


def _grad_names(case):
    return [k for k in hh.output_names(case) if k.startswith("g")]


def _zero_bar(inp):
    """The absolute bar of a gradient that is analytically zero: ``MARGIN 2**-23 sum|w tw| / sum m``."""
    return MARGIN * hh.EPS32 * float(inp["w"].double().abs().sum() * inp["tw"].double().abs().sum()) / max(float(inp["T"].isfinite().sum()), 1.0)


# ---- no GPU -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_inputs_meet_their_conditions_and_float32_an_eighth_of_the_caps(case):
    inp, ref, e32 = prepared(case)
    raw = ref["preds"]
    if case.missing == "all":
        assert bool(torch.isnan(ref["loss"]))
        return
    assert bool(torch.isfinite(ref["loss"]))
    if case.tasks == 1:
        assert float(ref["loss"]) == 0.0 and all(float(ref[k].abs().max()) <= _zero_bar(inp) for k in _grad_names(case))
        return
    last = len(case.dims) - 2
    assert float(ref[f"gW{last}"].abs().max()) > 0 and (case.shift or float(ref["gHv"].abs().max()) > 0)
    if case.sact == "softplus" and case.scale == 25.0 and case.B * case.tasks > 500:
        assert float(raw.max()) > 20      # softplus's linear branch
    if case.shift:
        assert float(raw.min()) > 89      # exp(x) alone overflows float32
    if case.missing == "task" and case.thr is None:
        row = ref[f"gW{last}"][case.tasks // 2].abs().max()
        if case.kind == "sid":
            assert float(row) <= _zero_bar(inp)
        else:
            assert float(row) > _zero_bar(inp)


# ---- GPU ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_spectral_head_matches_float64_within_the_float32_yardstick(case, gpu_device):
    inp, ref, e32 = prepared(case)
    got = run(case, inp, gpu_device)
    fails = []
    if got["n_finite"] != float(inp["T"].isfinite().sum()):
        fails.append(f"loss_out[1] = {got['n_finite']}: not the number of finite targets")
    last = len(case.dims) - 2
    if case.tasks == 1 and case.missing != "all":
        # loss and every gradient analytically 0: the absolute bar (a relative error against a reference of rounding noise says nothing)
        bar = _zero_bar(inp)
        print(f"HEADBAR {case.id} loss |loss|={abs(float(got['loss'])):.3e} bar={bar:.3e}")
        if not abs(float(got["loss"])) <= bar:
            fails.append(f"loss: |{float(got['loss']):.3e}| > {bar:.3e}")
        for k in _grad_names(case):
            v = float(got[k].abs().max())
            print(f"HEADBAR {case.id} {k} |g|={v:.3e} bar={bar:.3e}")
            if not v <= bar:
                fails.append(f"{k}: |g| {v:.3e} > {bar:.3e}")
        sub = dataclasses.replace(case, mode="infer")   # (preds, and nothing else, at the relative bar)
        fails += hh.compare(sub, got, ref, e32, MARGIN)
    else:
        fails += hh.compare(case, got, ref, e32, MARGIN)
    if case.missing == "task" and case.thr is None:
        row = float(got[f"gW{last}"][case.tasks // 2].abs().max())
        print(f"HEADBAR {case.id} gW{last}[masked task] |g|={row:.3e} bar={_zero_bar(inp):.3e}")
        if case.kind == "sid" and not row <= _zero_bar(inp):
            fails.append(f"gW{last}: the row of the task without targets is {row:.3e} > {_zero_bar(inp):.3e}")
        if case.kind == "wasserstein" and not row > _zero_bar(inp):
            fails.append(f"gW{last}: Wasserstein's masked column has no gradient ({row:.3e})")
    if case.shift and not all(bool(torch.isfinite(got[k]).all()) for k in hh.output_names(case)):
        fails.append("shifted exp: not finite")
    assert not fails, f"{case.id}: " + "; ".join(fails)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
def test_a_row_without_targets_among_others_is_a_nan_loss(kind, gpu_device):
    case = CASES[IDS.index(f"{kind}-t65-B5-linear-none-softplus-std1")]
    inp = dict(prepared(case)[0])
    T = inp["T"].clone()
    T[2] = float("nan")
    got = run(dataclasses.replace(case, mode="eval-loss"), dict(inp, T=T), gpu_device)
    assert bool(torch.isnan(got["loss"])) and got["n_finite"] == 4 * 65


@pytest.mark.gpu
@pytest.mark.parametrize("cid", ["sid-t1801-B9-hidden-some-softplus-std1", "wasserstein-t257-B3-hidden-some-exp-std1-thr",
                                 "wasserstein-t257-B3-linear-some-softplus-std25"])
def test_the_same_call_twice_is_bit_identical(cid, gpu_device):
    case = CASES[IDS.index(cid)]
    inp = prepared(case)[0]
    a, b = run(case, inp, gpu_device), run(case, inp, gpu_device)
    last = len(case.dims) - 2
    # (gb of the output layer is the column sum of gP; gHv carries every row of it)
    for k in ("loss", f"gb{last}", f"gW{last}", "gHv"):
        assert torch.equal(a[k], b[k]), (cid, k)


@pytest.mark.gpu
def test_a_strided_targets_view(gpu_device):
    """``targets`` as a view into a wider table (row stride > t): the ABI takes contiguous rows, the harness hands them over so."""
    case = CASES[IDS.index("wasserstein-t65-B5-hidden-some-softplus-std1")]
    inp, ref, e32 = prepared(case)
    wide = torch.full((case.B, case.tasks + 7), 3.0)
    wide[:, 3:3 + case.tasks] = inp["T"]
    view = wide[:, 3:3 + case.tasks]
    assert view.stride(0) == case.tasks + 7 and not view.is_contiguous()
    got = run(case, dict(inp, T=view), gpu_device)
    assert not hh.compare(case, got, ref, e32, MARGIN)


@pytest.mark.gpu
def test_launch_count_is_at_most_one_more_than_mses(gpu_device):
    """The spectral stage is two launches where ``k_loss`` is one.  Same shape and route: beyond ``kOutMaxTasks`` outputs both calls
    take the chain with the criterion as a stage of its own (up to ``kOutMaxTasks`` outputs the MSE call fuses its criterion into the
    output layer's backward or takes the four-launch form, which the spectral criteria are not part of)."""
    lib = _lib.load()
    for cid in ("sid-t65-B5-linear-some-softplus-std1", "wasserstein-t130-B37-hidden-some-softplus-std1", "wasserstein-t1801-B9-hidden-some-softplus-std1"):
        case = CASES[IDS.index(cid)]
        inp = prepared(case)[0]
        n = []
        for kind in (case.kind, "mse"):
            n0 = int(lib.dmpnn_last_launch_count())
            (run if kind != "mse" else hh.run_case)(dataclasses.replace(case, kind=kind), inp, gpu_device)
            n.append(int(lib.dmpnn_last_launch_count()) - n0)
        assert 0 < n[1] <= n[0] <= n[1] + 1, (cid, n)


@pytest.mark.gpu
def test_argument_checks_return_codes(gpu_device):
    import ctypes as C

    case = CASES[IDS.index("sid-t65-B5-linear-some-softplus-std1")]
    inp = prepared(case)[0]

    def code(**fields):
        orig = _lib.HeadArgs

        def make():
            h = orig()
            for k, v in fields.items():
                setattr(h, k, v)
            return h

        _lib.HeadArgs = make
        try:
            hh.run_case(case, inp, gpu_device)
        except Exception as e:   # (_lib.check raises with the library's message)
            return str(e)
        finally:
            _lib.HeadArgs = orig
        return None

    assert code() is None
    assert "spectral_act" in code(spectral_act=2)
    for bad in (-0.1, float("inf"), float("nan")):
        assert "spectral_threshold" in code(spectral_threshold=bad)


# ---- attentive aggregation and two components ---------------------------------------------------------------------------------------
ATT_CASE = SpectralCase("attentive-wasserstein-t65-B12", "default", 12, 8, (16,), 65, kind="wasserstein", act="tanh", agg="sum", bn=True,
                        missing="some", sact="exp", thr=0.5 / 65, scale=1.0)


@functools.lru_cache(maxsize=None)
def prepared_attentive():
    case = ATT_CASE
    inp = ah.head_inputs(dataclasses.replace(case, kind="mse"))
    inp["T"] = spectral_targets(case.B, case.tasks, case.missing, 0)
    with spectral_reference():
        _rescale_output_layer(case, inp, ah.head_reference(dataclasses.replace(case, mode="eval-loss"), inp)["preds"])
        ref, e32 = ah.head_yardstick(case, inp)
    _within_an_eighth_of_the_caps(case.id, ah.head_output_names(case), e32, ref)
    return inp, ref, e32


def test_attentive_case_float32_meets_an_eighth_of_the_caps():
    prepared_attentive()


@pytest.mark.gpu
def test_attentive_head_with_a_spectral_criterion(gpu_device):
    case = ATT_CASE
    inp, ref, e32 = prepared_attentive()
    with spectral_fields(case):
        got = ah.run_head(case, inp, gpu_device)
    fails = hh.compare(case, got, ref, e32, MARGIN)
    g, r = got["g_att_W"].double().reshape(-1), ref["g_att_W"].double().reshape(-1)
    err = parity_err_unfloored(g.numpy(), r.numpy())
    bar = min(MARGIN * max(e32["g_att_W"], hh.EPS32), hh.cap_of("g_att_W"))
    print(f"HEADBAR {case.id} g_att_W err={err:.3e} e32={e32['g_att_W']:.3e} ratio={err / max(e32['g_att_W'], hh.EPS32):.2f} bar={bar:.3e}")
    if not err <= bar:
        fails.append(f"g_att_W: err {err:.3e} > bar {bar:.3e}")
    assert not fails, f"{case.id}: " + "; ".join(fails)


def _two_component_inputs(seed=0):
    from chemprop_amd import agg as cagg
    from chemprop_amd.model import SID, MulticomponentMPNN, SpectralFFN
    from chemprop_amd.nn import BondMessagePassing, MulticomponentMessagePassing
    from test_multicomponent import batches

    torch.manual_seed(seed + 11)
    n, d_h, t = 12, 24, 65
    mp = MulticomponentMessagePassing([BondMessagePassing(72, 14, d_h=d_h, depth=2, activation="tanh") for _ in range(2)], 2, shared=False)
    gen = torch.Generator().manual_seed(seed + 5)
    pred = SpectralFFN(n_tasks=t, input_dim=2 * d_h, hidden_dim=16, activation="tanh", criterion=SID(0.5 + torch.rand(t, generator=gen)))
    model = MulticomponentMPNN(mp, cagg.MeanAggregation(), pred, batch_norm=True).train()
    with torch.no_grad():
        model.bn.weight.uniform_(0.5, 1.5, generator=gen), model.bn.bias.uniform_(-0.5, 0.5, generator=gen)
        model.bn.running_mean.uniform_(-0.1, 0.1, generator=gen), model.bn.running_var.uniform_(0.5, 2.0, generator=gen)
    bs = batches(["qm9", "qm9"], n, seed=seed)
    Hvs = [torch.randn(int(b.V.shape[0]), d_h, generator=gen) for b in bs]
    return model, Hvs, [b.batch for b in bs], spectral_targets(n, t, "some", seed), 0.5 + torch.rand(n, 1, generator=gen)


def _restate_two_components(model, Hvs, bts, T, w, dtype):
    F = torch.nn.functional
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
    from chemprop_amd.ffn import mlp_blocks

    for l, blk in enumerate(mlp_blocks(model.predictor.ffn)):
        lin = blk[-1]
        leaves[f"gW{l}"], leaves[f"gb{l}"] = f(lin.weight).requires_grad_(), f(lin.bias).requires_grad_()
        Z = F.linear(torch.tanh(Z) if l else Z, leaves[f"gW{l}"], leaves[f"gb{l}"])
    loss = spectral_criterion("sid", Z, f(T), f(w).reshape(-1), f(model.predictor.criterion.task_weights).reshape(-1))
    loss.backward()
    out = {k: v.grad for k, v in leaves.items()}
    out.update(loss=loss.detach(), preds=Z.detach(), running_mean=rm, running_var=rv)
    return out


@functools.lru_cache(maxsize=None)
def prepared_two_components():
    model, Hvs, bts, T, w = _two_component_inputs()
    r64 = _restate_two_components(model, Hvs, bts, T, w, torch.float64)
    r32 = _restate_two_components(model, Hvs, bts, T, w, torch.float32)
    e32 = {k: parity_err_unfloored(r32[k].double().numpy(), r64[k].numpy()) for k in r64}
    _within_an_eighth_of_the_caps("two-components-sid-t65-B12", list(r64), e32, r64)
    return model, Hvs, bts, T, w, r64, e32


def test_two_component_case_float32_meets_an_eighth_of_the_caps():
    prepared_two_components()


@pytest.mark.gpu
def test_two_component_head_with_a_spectral_criterion(gpu_device):
    """``n_components = 2`` through ``HeadSpec.fill`` — which hands ``spectral_act`` / ``spectral_threshold`` over itself."""
    import copy

    from chemprop_amd.ffn import mlp_blocks
    from chemprop_amd.model import HeadSpec
    from test_multicomponent import run_head

    cid = "two-components-sid-t65-B12"
    cpu_model, Hvs, bts, T, w, ref, e32 = prepared_two_components()
    model = copy.deepcopy(cpu_model).to(gpu_device)
    spec = HeadSpec(model)
    assert (spec.kind, spec.n_tasks, spec.n_components, spec.spectral_act) == ("sid", 65, 2, "softplus")
    to = lambda t: t.to(gpu_device)
    loss, P, g, gH = run_head(model, [to(h) for h in Hvs], [to(b) for b in bts], 12, to(T), to(w))
    got = dict(loss=torch.tensor(loss), preds=P, gHv0=gH[0], gHv1=gH[1], g_bn_weight=g[id(model.bn.weight)], g_bn_bias=g[id(model.bn.bias)],
               running_mean=model.bn.running_mean.cpu(), running_var=model.bn.running_var.cpu())
    for l, blk in enumerate(mlp_blocks(model.predictor.ffn)):
        got[f"gW{l}"], got[f"gb{l}"] = g[id(blk[-1].weight)], g[id(blk[-1].bias)]
    assert set(got) == set(ref)
    fails = []
    for k in sorted(ref):
        a, r = got[k].double().reshape(-1), ref[k].double().reshape(-1)
        assert a.shape == r.shape and bool(torch.isfinite(a).all()), (cid, k)
        err = parity_err_unfloored(a.numpy(), r.numpy())
        bar = min(MARGIN * max(e32[k], hh.EPS32), hh.cap_of(k))
        print(f"HEADBAR {cid} {k} err={err:.3e} e32={e32[k]:.3e} ratio={err / max(e32[k], hh.EPS32):.2f} bar={bar:.3e} maxref={float(r.abs().max()):.3e}")
        if not err <= bar:
            fails.append(f"{k}: err {err:.3e} > bar {bar:.3e} (fp32 yardstick {e32[k]:.3e})")
    assert not fails, f"{cid}: " + "; ".join(fails)
