"""Epoch metric statistics on the host (no GPU): the two new argument structs as a C compiler lays them out, ``MetricStats.compute``'s
formulas against metrics computed directly from the raw arrays, the CPU ``update`` against an independent numpy restatement (and
against deliberately wrong ones), accumulation over uneven batches, ``merge``, and every refusal of ``dmpnn_metric_stats`` /
``dmpnn_validate_head`` — codes before any device work, ``dmpnn_last_launch_count()`` as it was.

Tolerance of the formula comparisons: 1e-9 relative.  The sums and the direct computations differ by float64 summation error, about
``2^-53 n``; only R2 amplifies it — the one-pass ``sum t^2 - (sum t)^2 / n`` cancels by ``mean^2 / var``, here 0.25 (targets ``2 N(0, 1)
+ 1``; the bar allows 1e3): at ``n = 300`` about ``3e-14 (1 + 0.25)``, five orders inside the bar."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import metric_harness as mh
from chemprop_amd import _lib
from chemprop_amd.metrics import MetricStats

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = (("regression", 1, 0), ("regression", 2, 0), ("regression", 4, 0), ("binary", 1, 0), ("binary", 2, 0), ("multiclass", 3, 3), ("multiclass", 16, 16))
IDS = [f"{k}-w{w}" for k, w, _ in KINDS]


def _stats(kind, t, nc, inp, **kw):
    s = MetricStats(kind, t, nc)
    s.update(inp["P"], inp["T"], inp.get("lt"), inp.get("gt"), **kw)
    return s


def _ref(kind, nc, inp, **kw):
    return mh.ref_stats(kind, inp["P"].numpy(), inp["T"].numpy(), None if "lt" not in inp else inp["lt"].numpy(),
                        None if "gt" not in inp else inp["gt"].numpy(), nc=nc, **kw)


def test_new_structs_match_a_c_compiler_and_the_abi_version_stays(tmp_path):
    """sizeof / offsetof of dmpnn_metric_args and dmpnn_validate_args as gcc lays out include/dmpnn.h == the ctypes mirrors
    (tests/test_abi.py's method); v15 growth: the version does not move."""
    import shutil
    import subprocess

    lib = _lib.load()
    assert lib.dmpnn_version() == 15 == _lib.ABI_VERSION
    if not shutil.which("gcc"):
        pytest.skip("no gcc")
    mirrors = dict(dmpnn_metric_args=_lib.MetricArgs, dmpnn_validate_args=_lib.ValidateArgs)
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "dmpnn.h"', "int main(void) {"]
    for name, m in mirrors.items():
        lines.append(f'printf("{name} %zu\\n", sizeof({name}));')
        for f in m._fields_:
            lines.append(f'printf("{name}.{f[0]} %zu\\n", offsetof({name}, {f[0]}));')
    lines += ['printf("kinds %d %d %d %d %d %d\\n", DMPNN_METRIC_NONE, DMPNN_METRIC_REGRESSION, DMPNN_METRIC_BINARY, DMPNN_METRIC_MULTICLASS, '
              'DMPNN_METRIC_MAX_CLASSES, DMPNN_METRIC_HEADER);', "return 0; }"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    rows = [l.split() for l in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines()]
    out = {r[0]: r[1:] for r in rows}
    for name, m in mirrors.items():
        assert int(out[name][0]) == C.sizeof(m), name
        for f in m._fields_:
            assert int(out[f"{name}.{f[0]}"][0]) == getattr(m, f[0]).offset, f"{name}.{f[0]}"
    assert [int(x) for x in out["kinds"]] == [_lib.METRIC[k] for k in ("none", "regression", "binary", "multiclass")] + [_lib.METRIC_MAX_CLASSES, _lib.METRIC_HEADER]
    assert _lib.ValidateArgs.predict.offset == 0   # (dmpnn_predict_args comes first)


def test_sizes_are_shape_rules():
    lib = _lib.load()
    R, B, M = (_lib.METRIC[k] for k in ("regression", "binary", "multiclass"))
    assert lib.dmpnn_metric_stats_doubles(R, 3, 0) == 4 + 24 == lib.dmpnn_metric_stats_doubles(B, 3, 0)
    assert lib.dmpnn_metric_stats_doubles(M, 2, 3) == 4 + 18 and lib.dmpnn_metric_stats_doubles(0, 7, 0) == 4
    assert lib.dmpnn_metric_stats_doubles(9, 3, 0) == 0 and lib.dmpnn_metric_stats_doubles(M, 2, 17) == 0 and lib.dmpnn_metric_stats_doubles(M, 2, 1) == 0
    assert lib.dmpnn_metric_stats_doubles(R, -1, 0) == 0
    for kind, t, nc in (("regression", 3, 0), ("multiclass", 2, 3), ("none", 5, 0)):
        assert MetricStats(kind, t, nc).stats.numel() == lib.dmpnn_metric_stats_doubles(_lib.METRIC[kind], t, nc)
    a = _lib.MetricArgs()
    a.kind, a.n_mols, a.n_tasks = R, 300, 3
    assert lib.dmpnn_metric_stats_ws_bytes(C.byref(a)) == 768      # 3 row blocks of 128 x 3 tasks x 8 doubles, in 256-byte units
    a.n_mols = 128
    assert lib.dmpnn_metric_stats_ws_bytes(C.byref(a)) == 256
    a.kind = 0
    assert lib.dmpnn_metric_stats_ws_bytes(C.byref(a)) == 0 and lib.dmpnn_metric_stats_ws_bytes(None) == 0


@pytest.mark.parametrize("kind,width,nc", KINDS, ids=IDS)
def test_cpu_update_writes_the_layout_the_numpy_restatement_writes(kind, width, nc):
    """Counts exact, sums within 1e-12 of the sum of the absolute terms; and the self-check — the restatement with ONE deliberate
    mistake (``>=`` at the threshold, the masks ignored, the highest index among equal maxima) must NOT pass the same comparison."""
    t = 5
    inp = mh.make_inputs(kind, 300, t, width, seed=3)
    loss = torch.tensor([0.75, float(inp["T"].isfinite().sum())])
    got = _stats(kind, t, nc, inp, loss=loss).stats.numpy()
    ref, scale = _ref(kind, nc, inp, loss=loss.numpy()), _ref(kind, nc, inp, loss=loss.numpy(), abs_terms=True)
    same = lambda a, b: bool(np.all(np.abs(a - b) <= 1e-12 * scale))
    assert same(got, ref), np.abs(got - ref).max()
    body = got[4:].reshape(t, -1)
    if kind == "multiclass":
        assert np.array_equal(got, ref)                                  # counts: exact
        assert body[1].sum() == 0                                        # the all-NaN column
        assert 0 < body.sum() < inp["T"].isfinite().sum()                # out-of-range classes were skipped
    else:
        assert np.array_equal(body[:, 0], ref[4:].reshape(t, -1)[:, 0]) and body[1, 0] == 0
        assert np.all(body[:, 7 if kind == "regression" else 5:] == 0)   # the reserved slots
        if kind == "binary":
            assert np.array_equal(got, ref) and np.array_equal(body[:, 1:5].sum(1), body[:, 0])
    assert got[0] == 0.75 * float(loss[1]) and got[1] == float(loss[1]) and got[2] == 1 and got[3] == 300
    wrong = _ref(kind, nc, inp, loss=loss.numpy(), wrong=mh.WRONG[kind])
    assert not same(got, wrong), f"the comparison does not see {mh.WRONG[kind]}"


@pytest.mark.parametrize("kind,width,nc", KINDS, ids=IDS)
def test_compute_on_a_hand_built_buffer_equals_the_metrics_of_the_raw_arrays(kind, width, nc):
    t = 6
    inp = mh.make_inputs(kind, 300, t, width, seed=5)
    T = inp["T"]
    # degenerate tasks: column 1 is all NaN (make_inputs); one class only; one finite target
    T[:, 2] = torch.where(T[:, 2].isfinite(), torch.ones(300), T[:, 2])
    T[1:, 3] = float("nan")
    T[0, 3] = 1.0
    s = MetricStats(kind, t, nc)
    s.stats.copy_(torch.from_numpy(_ref(kind, nc, inp, loss=np.array([1.25, 40.0]))))
    got = s.compute()
    ref = mh.direct_metrics(kind, inp["P"].numpy(), T.numpy(), None if "lt" not in inp else inp["lt"].numpy(),
                            None if "gt" not in inp else inp["gt"].numpy(), nc=nc)
    assert set(ref) <= set(got) and got["val_loss"] == 1.25 and got["n_calls"] == 1 and got["n_mols"] == 300
    for k, v in ref.items():
        print(f"METRIC {kind}-w{width} {k} got={got[k]!r} direct={v!r}")
        assert mh.close(got[k], v), (k, got[k], v)
    per = got["per_task"]
    assert per["n"][1] == 0 and all(len(v) == t for v in per.values())
    if kind == "regression":
        assert np.isnan(per["mse"][1]) and np.isnan(per["r2"][1]) and np.isnan(per["r2"][2]) and np.isnan(per["r2"][3]) and per["n"][3] == 1
        assert np.isfinite(per["r2"][0]) and got["bounded-mse"] < got["mse"]
    elif kind == "binary":
        assert per["binary-mcc"][1] == 0 and per["binary-mcc"][2] == 0 and per["accuracy"][1] == 0
    else:
        assert per["multiclass-mcc"][1] == 0 and per["multiclass-mcc"][2] == 0


def test_compute_without_a_finite_target():
    s = MetricStats("regression", 2)
    s.update(torch.zeros(4, 2), torch.full((4, 2), float("nan")), loss=torch.tensor([float("nan"), 0.0]))
    got = s.compute()
    assert all(np.isnan(got[k]) for k in ("val_loss", "mse", "mae", "rmse", "r2", "bounded-mse")) and got["n_mols"] == 4
    assert MetricStats("none", 3).compute()["per_task"] == {}


@pytest.mark.parametrize("kind,width,nc", KINDS, ids=IDS)
def test_three_uneven_batches_accumulate_to_the_concatenation_and_merge_is_addition(kind, width, nc):
    t = 4
    inp = mh.make_inputs(kind, 300, t, width, seed=7)
    cuts = ((0, 1), (1, 130), (130, 300))
    losses = [torch.tensor([0.5 + i, float(inp["T"][a:b].isfinite().sum())]) for i, (a, b) in enumerate(cuts)]
    part = lambda a, b: {k: v[a:b] for k, v in inp.items()}
    acc = MetricStats(kind, t, nc)
    singles = []
    for (a, b), l in zip(cuts, losses):
        acc.update(part(a, b)["P"], part(a, b)["T"], part(a, b).get("lt"), part(a, b).get("gt"), loss=l)
        singles.append(_stats(kind, t, nc, part(a, b), loss=l))
    acc.update(inp["P"][:0], inp["T"][:0])   # an empty batch: nothing, not even a call
    n_fin = sum(float(l[1]) for l in losses)
    mean_loss = sum(float(l[0]) * float(l[1]) for l in losses) / n_fin
    whole = _stats(kind, t, nc, inp, loss=torch.tensor([mean_loss, n_fin], dtype=torch.float64))   # (float32 would round the mean at 6e-8)
    scale = _ref(kind, nc, inp, loss=np.array([mean_loss, n_fin]), abs_terms=True)
    a, w = acc.stats.numpy(), whole.stats.numpy()
    assert a[2] == 3 and a[3] == 300 and w[2] == 1
    assert np.all(np.abs(a[4:] - w[4:]) <= 1e-12 * scale[4:]) and abs(a[0] - w[0]) <= 1e-12 * abs(w[0]) and a[1] == w[1]
    ga, gw = acc.compute(), whole.compute()
    for k in gw:
        if k not in ("per_task", "n_calls"):
            assert mh.close(ga[k], gw[k]), (k, ga[k], gw[k])
    merged = MetricStats(kind, t, nc)
    for s in singles:
        merged.merge(s)
    assert torch.equal(merged.stats, singles[0].stats + singles[1].stats + singles[2].stats)
    assert np.all(np.abs(merged.stats.numpy() - a) <= 1e-12 * np.maximum(scale, 1))
    with pytest.raises(ValueError):
        merged.merge(MetricStats(kind, t + 1, nc))
    merged.reset()
    assert float(merged.stats.abs().sum()) == 0


def test_update_refuses_misshapen_batches():
    s = MetricStats("multiclass", 2, 3)
    with pytest.raises(ValueError):
        s.update(torch.zeros(4, 2, 4), torch.zeros(4, 2))
    with pytest.raises(ValueError):
        s.update(torch.zeros(4, 2, 3), torch.zeros(4, 3))
    with pytest.raises(ValueError):
        MetricStats("multiclass", 2, 17)
    with pytest.raises(ValueError):
        MetricStats("auroc", 2)


def test_for_model_reads_the_kind_off_the_predictor():
    from chemprop_amd import agg as cagg
    from chemprop_amd import model as cm
    from chemprop_amd.nn import BondMessagePassing

    def stats(pred):
        return MetricStats.for_model(cm.MPNN(BondMessagePassing(d_h=16, depth=2), cagg.MeanAggregation(), pred), device="cpu")

    kw = dict(input_dim=16, hidden_dim=8)
    for pred, want in ((cm.RegressionFFN(n_tasks=3, **kw), ("regression", 3, 0)), (cm.MveFFN(n_tasks=2, **kw), ("regression", 2, 0)),
                       (cm.BinaryClassificationFFN(n_tasks=4, **kw), ("binary", 4, 0)), (cm.BinaryDirichletFFN(n_tasks=2, **kw), ("binary", 2, 0)),
                       (cm.MulticlassClassificationFFN(5, n_tasks=2, **kw), ("multiclass", 2, 5)),
                       (cm.MulticlassDirichletFFN(3, n_tasks=2, **kw), ("multiclass", 2, 3)),
                       (cm.SpectralFFN(n_tasks=7, criterion=cm.SID(), **kw), ("none", 7, 0))):
        s = stats(pred)
        assert (s.kind, s.n_tasks, s.n_classes) == want, type(pred).__name__


# ---- refusals: codes before any device work ------------------------------------------------------------------------------------------
P = 4096   # a non-NULL dummy address: every rule must hold before anything is dereferenced


def _metric_args(**kw):
    a = _lib.MetricArgs()
    a.kind, a.n_mols, a.n_tasks, a.group, a.threshold = _lib.METRIC["regression"], 10, 3, 1, 0.5
    a.preds, a.ld_p, a.targets, a.ld_t, a.stats, a.stats_bytes = P, 3, P, 3, P, 8 * 28
    a.ws, a.ws_bytes = None, 0   # (the LAST rule: a call that passes every other one ends here, DMPNN_ENOSPC, nothing launched)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_metric_stats_refusals_are_codes_and_launch_nothing():
    lib = _lib.load()
    n0 = lib.dmpnn_last_launch_count()
    assert lib.dmpnn_metric_stats(None, None) == -1
    assert lib.dmpnn_metric_stats(C.byref(_metric_args()), None) == -3 and b"workspace" in lib.dmpnn_last_error_string()
    M, B = _lib.METRIC["multiclass"], _lib.METRIC["binary"]
    bad = [dict(kind=7), dict(kind=-1), dict(n_mols=-1), dict(n_tasks=-1), dict(group=3), dict(group=0), dict(preds=None), dict(targets=None),
           dict(ld_p=2), dict(ld_t=2), dict(group=2, ld_p=5), dict(stats=None), dict(stats=P + 4), dict(stats_bytes=8 * 28 - 1),
           dict(kind=B, threshold=float("nan")), dict(kind=B, threshold=float("inf")),
           dict(kind=M, n_classes=1, ld_p=3), dict(kind=M, n_classes=17, ld_p=51, stats_bytes=1 << 20), dict(kind=M, n_classes=3, ld_p=8, stats_bytes=1 << 20),
           dict(kind=M, n_classes=3, ld_p=9, stats_bytes=8 * (4 + 27) - 1)]
    for kw in bad:
        assert lib.dmpnn_metric_stats(C.byref(_metric_args(**kw)), None) == -1, kw
        assert lib.dmpnn_last_error_string() != b""
    assert lib.dmpnn_metric_stats(C.byref(_metric_args(ws=P, ws_bytes=255)), None) == -3
    assert lib.dmpnn_metric_stats(C.byref(_metric_args(kind=M, n_classes=3, ld_p=9, stats_bytes=8 * (4 + 27))), None) == -3   # (valid but for ws)
    assert lib.dmpnn_metric_stats(C.byref(_metric_args(n_mols=0)), None) == 0      # an empty batch: OK, nothing launched, nothing read
    assert lib.dmpnn_last_launch_count() == n0


def _validate_args(transform="unscale", n_out=3, loss="mse", n_classes=0, kind="regression", **kw):
    v = _lib.ValidateArgs()
    h = v.predict.head
    h.n_atoms, h.n_mols, h.d_h, h.batch = 40, 10, 8, P
    h.n_layers, h.dims[0], h.dims[1], h.W[0] = 1, 8, n_out, P
    h.loss, h.n_classes, h.quantile_alpha = _lib.LOSS[loss], n_classes, 0.1
    h.preds, h.targets, h.loss_out = P, P, P
    v.predict.transform = _lib.PT_SPECTRAL if transform == "spectral" else _lib.PREDICT_TRANSFORM[transform]
    v.predict.preds = P
    v.metric_kind, v.threshold, v.stats, v.stats_bytes = _lib.METRIC[kind], 0.5, P, 1 << 20
    for k, val in kw.items():
        obj, name = (h, k[5:]) if k.startswith("head_") else ((v.predict, k[8:]) if k.startswith("predict_") else (v, k))
        setattr(obj, name, val)
    return v


def test_validate_head_refusals_are_codes_and_launch_nothing():
    lib = _lib.load()
    n0 = lib.dmpnn_last_launch_count()
    call = lambda v: lib.dmpnn_validate_head(C.byref(v), P, 8, None)
    assert lib.dmpnn_validate_head(None, P, 8, None) == -1
    # what passes every argument rule ends at the workspace rule (no workspace given): DMPNN_ENOSPC, nothing launched
    ok = [_validate_args(), _validate_args("none"), _validate_args("mve", 6, "mve"), _validate_args("evidential", 12, "evidential"),
          _validate_args("quantile", 6, "quantile"), _validate_args("sigmoid", 3, "bce", kind="binary"),
          _validate_args("softmax", 6, "ce", 3, kind="multiclass"), _validate_args("softmax", 32, "ce", 16, kind="multiclass"),
          _validate_args("spectral", 9, "sid", kind="none"), _validate_args(kind="none"), _validate_args(metric_targets=P, ld_mt=3)]
    for v in ok:
        assert call(v) == -3 and b"validate_head: workspace" in lib.dmpnn_last_error_string()
        assert lib.dmpnn_validate_head_ws_bytes(C.byref(v)) >= lib.dmpnn_predict_head_ws_bytes(C.byref(v.predict)) > 0
    v = _validate_args()
    assert lib.dmpnn_validate_head_ws_bytes(C.byref(v)) == lib.dmpnn_predict_head_ws_bytes(C.byref(v.predict)) + 256   # one row block x 3 tasks x 8 doubles
    v = _validate_args(kind="none")
    assert lib.dmpnn_validate_head_ws_bytes(C.byref(v)) == lib.dmpnn_predict_head_ws_bytes(C.byref(v.predict))
    bad = [_validate_args(head_targets=None), _validate_args(head_loss_out=None), _validate_args(predict_preds=None),
           _validate_args(kind="binary"), _validate_args(kind="multiclass"), _validate_args("sigmoid", 3, "bce"),
           _validate_args("sigmoid", 3, "bce", kind="multiclass"), _validate_args("mve", 6, "mve", kind="binary"),
           _validate_args("softmax", 6, "ce", 3), _validate_args("softmax", 6, "ce", 3, kind="binary"),
           _validate_args("softmax", 34, "ce", 17, kind="multiclass"),                      # n_classes beyond DMPNN_METRIC_MAX_CLASSES
           _validate_args("spectral", 9, "sid"), _validate_args("spectral", 9, "sid", kind="binary"), _validate_args("spectral", 9, "wasserstein", kind="multiclass"),
           _validate_args(stats_bytes=8 * 28 - 1), _validate_args(stats=None), _validate_args(metric_kind=4), _validate_args(metric_kind=-1),
           _validate_args(metric_targets=P, ld_mt=2), _validate_args("sigmoid", 3, "bce", kind="binary", threshold=float("nan")),
           _validate_args(head_gHv=P), _validate_args(predict_transform=7)]                  # (dmpnn_predict_head's own rules still hold)
    for i, v in enumerate(bad):
        assert call(v) == -1, i
    assert lib.dmpnn_validate_head_ws_bytes(None) == 0
    assert lib.dmpnn_last_launch_count() == n0
