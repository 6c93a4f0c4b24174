"""Epoch rank metrics on the host (no GPU): ``RankStats`` on CPU tensors — ``rank_keys`` and the float64 numpy ``rank_column`` — against
``rank_harness``'s sort-based curves and all-pairs ``U2`` (and scikit-learn where it is installed), the three new argument structs as a C
compiler lays them out, every refusal of ``dmpnn_rank_append`` / ``dmpnn_validate_head_ranked`` / ``dmpnn_rank_metrics`` — codes before any
device work, ``dmpnn_last_launch_count()`` as it was — and the bookkeeping: ``merge``, uneven ``update`` pieces, ``for_model``, ``reset``.

Conditions: ``n_pos`` / ``n_neg`` / ``n_skipped`` / ``n_thresholds`` / ``U2`` exact; ``roc`` bit-equal to ``U2 / (2.0 P N)``; ``roc`` and ``prc``
within ``(n_ranked + 8) 2^-52`` absolute of the curves (``rank_harness.bar``: derived from the number of terms, not measured); NaN exactly
where a class is absent."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import rank_harness as rh
from chemprop_amd import _lib
from chemprop_amd.metrics import RankStats

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(n, t) for n in (1, 2, 65, 257, 1025) for t in (1, 3, 5)]


def _seed(n, t):
    return 3 * n + t   # (over SHAPES every one of the ten column patterns comes up)


def _filled(S, T, cap=None):
    r = RankStats(S.shape[1], cap if cap is not None else S.shape[0])
    r.update(torch.from_numpy(S), torch.from_numpy(T))
    return r


def _judge(tag, row, S, T, fails, all_pairs=True):
    """One row of ``dmpnn_rank_metrics``' ``out`` layout (n_pos, n_neg, n_skipped, n_thresholds, U2, roc, prc, 0) against the references."""
    ref = rh.ref_curves(S, T)
    want = [ref["P"], ref["N"], ref["n_skipped"], ref["n_thresholds"], ref["U2"]]
    if [float(x) for x in want] != [float(x) for x in row[:5]]:
        fails.append(f"{tag}: counts {row[:5].tolist()} != {want}")
    if all_pairs and rh.ref_u2(S, T) != row[4]:
        fails.append(f"{tag}: U2 {row[4]} != all-pairs {rh.ref_u2(S, T)}")
    if row[7] != 0:
        fails.append(f"{tag}: slot 7 is {row[7]}")
    both = ref["P"] > 0 and ref["N"] > 0
    b = rh.bar(ref["n_ranked"])
    for name, k in (("roc", 5), ("prc", 6)):
        print(f"RANKBAR {tag} {name} got={row[k]!r} want={ref[name]!r} bar={b:.3e}")
        if not both:
            if not np.isnan(row[k]):
                fails.append(f"{tag}: {name} = {row[k]} without both classes")
        elif not abs(row[k] - ref[name]) <= b:
            fails.append(f"{tag}: {name} {row[k]!r} vs {ref[name]!r}, bar {b:.3e}")
    if both and row[5] != row[4] / (2.0 * row[0] * row[1]):
        fails.append(f"{tag}: roc is not U2 / (2 P N) bit for bit")
    return both


@pytest.mark.parametrize("n,t", SHAPES)
def test_cpu_rank_stats_against_the_sorted_curves_and_the_all_pairs_count(n, t):
    S, T = rh.make_inputs(n, t, _seed(n, t))
    got = _filled(S, T).compute()
    per, fails, both = got["per_task"], [], []
    for j in range(t):
        row = np.array([per["n_pos"][j], per["n_neg"][j], per["n_skipped"][j], per["n_thresholds"][j], per["U2"][j], per["roc"][j], per["prc"][j], 0.0])
        both.append(_judge(f"n{n}-t{t}-col{j}-pattern{rh.pattern_of(j, _seed(n, t))}", row, S[:, j], T[:, j], fails))
    pl = got["pooled"]
    row = np.array([pl["n_pos"], pl["n_neg"], pl["n_skipped"], pl["n_thresholds"], pl["U2"], got["roc-pooled"], got["prc-pooled"], 0.0])
    _judge(f"n{n}-t{t}-pooled", row, S.reshape(-1), T.reshape(-1), fails)
    assert not fails, fails
    both = np.array(both)
    for name in ("roc", "prc"):
        if both.any():
            assert got[name] == float(per[name][both].mean())
        else:
            assert np.isnan(got[name])
    assert got["n_mols"] == n and "roc-pooled" not in _filled(S, T).compute(pooled=False)


def test_every_column_pattern_is_met_and_the_keys_follow_the_rules():
    seen = {rh.pattern_of(j, _seed(n, t)) for n, t in SHAPES for j in range(t)}
    assert seen == set(range(rh.N_PATTERNS))
    from chemprop_amd.metrics import rank_keys

    s = torch.tensor([0.0, -0.0, 1e-40, 2e-40, -1e-40, 1.0, -1.0, float("inf"), float("nan"), 0.5, 3.4e38, -3.4e38])
    t = torch.tensor([1.0, 0.0, 0.5, 0.51, 1.0, 0.0, 1.0, 1.0, 0.0, float("nan"), 0.0, float("-inf")])
    k, l = rank_keys(s, t)
    ku = k.numpy().view(np.uint32)
    assert l.tolist() == [1, 0, 0, 1, 1, 0, 1, 3, 3, 2, 0, 2]
    assert ku[0] == ku[1] == 0x80000000 and ku[7] == ku[8] == ku[9] == ku[11] == 0
    ranked = [0, 2, 3, 4, 5, 6, 10]
    assert all(ku[i] != 0 for i in ranked)
    order = sorted(ranked, key=lambda i: float(s[i].double()))
    assert [int(ku[i]) for i in order] == sorted(int(ku[i]) for i in ranked) and len({int(ku[i]) for i in ranked}) == len(ranked)


@pytest.mark.parametrize("n,t", [(65, 3), (1025, 5)])
def test_against_scikit_learn(n, t):
    skm = pytest.importorskip("sklearn.metrics")
    S, T = rh.make_inputs(n, t, _seed(n, t))
    per = _filled(S, T).compute()["per_task"]
    for j in range(t):
        ok = np.isfinite(T[:, j]) & np.isfinite(S[:, j])
        y, s = T[ok, j] > 0.5, S[ok, j].astype(np.float64)
        if y.all() or not y.any():
            assert np.isnan(per["roc"][j]) and np.isnan(per["prc"][j])
            continue
        precision, recall, _ = skm.precision_recall_curve(y, s)
        b = rh.bar(int(ok.sum()))
        assert abs(per["roc"][j] - skm.roc_auc_score(y, s)) <= b and abs(per["prc"][j] - skm.auc(recall, precision)) <= b


def test_new_structs_match_a_c_compiler_and_the_abi_version_stays(tmp_path):
    import shutil
    import subprocess

    lib = _lib.load()
    assert lib.dmpnn_version() == 15 == _lib.ABI_VERSION
    assert _lib.ValidateRankArgs.validate.offset == 0 and C.sizeof(_lib.ValidateRankArgs) == C.sizeof(_lib.ValidateArgs) + 32
    if not shutil.which("gcc"):
        pytest.skip("no gcc")
    mirrors = dict(dmpnn_rank_append_args=_lib.RankAppendArgs, dmpnn_validate_rank_args=_lib.ValidateRankArgs, dmpnn_rank_args=_lib.RankArgs)
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "dmpnn.h"', "int main(void) {"]
    for name, m in mirrors.items():
        lines.append(f'printf("{name} %zu\\n", sizeof({name}));')
        for f in m._fields_:
            lines.append(f'printf("{name}.{f[0]} %zu\\n", offsetof({name}, {f[0]}));')
    lines += ['printf("consts %d %d %d\\n", DMPNN_RANK_MAX_ROWS, DMPNN_RANK_TILE, DMPNN_RANK_OUT);', "return 0; }"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = {r[0]: r[1:] for r in (l.split() for l in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())}
    for name, m in mirrors.items():
        assert int(out[name][0]) == C.sizeof(m), name
        for f in m._fields_:
            assert int(out[f"{name}.{f[0]}"][0]) == getattr(m, f[0]).offset, f"{name}.{f[0]}"
    assert [int(x) for x in out["consts"]] == [_lib.RANK_MAX_ROWS, _lib.RANK_TILE, _lib.RANK_OUT] == [262144, _lib.RANK_TILE, 8]
    assert 1024 <= _lib.RANK_TILE <= 4096


# ---- refusals: codes before any device work ------------------------------------------------------------------------------------------
P = 4096   # a non-NULL dummy address: every rule must hold before anything is dereferenced


def _append_args(**kw):
    a = _lib.RankAppendArgs()
    a.n_mols, a.n_tasks, a.group, a.preds, a.ld_p, a.targets, a.ld_t = 10, 3, 1, P, 3, P, 3
    a.keys, a.labels, a.capacity, a.row0 = P, P, 9, 0   # (the LAST rule: what passes every other one ends here, DMPNN_ENOSPC, nothing launched)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_rank_append_refusals_are_codes_and_launch_nothing():
    lib = _lib.load()
    n0 = lib.dmpnn_last_launch_count()
    assert lib.dmpnn_rank_append(None, None) == -1
    for kw in (dict(), dict(capacity=20, row0=11), dict(capacity=20, row0=21), dict(group=2, ld_p=6), dict(capacity=(1 << 62), row0=(1 << 62) - 9)):
        assert lib.dmpnn_rank_append(C.byref(_append_args(**kw)), None) == -3, kw
        assert b"do not fit" in lib.dmpnn_last_error_string()
    bad = [dict(n_mols=-1), dict(n_tasks=-1), dict(capacity=-1), dict(row0=-1), dict(group=3), dict(group=0), dict(group=4, ld_p=12), dict(preds=None),
           dict(targets=None), dict(keys=None), dict(labels=None), dict(ld_p=2), dict(ld_t=2), dict(group=2, ld_p=5), dict(n_mols=1 << 31),
           dict(n_mols=1 << 29, n_tasks=8, ld_p=8, ld_t=8)]
    for kw in bad:
        assert lib.dmpnn_rank_append(C.byref(_append_args(**{**dict(capacity=1 << 40), **kw})), None) == -1, kw
        assert lib.dmpnn_last_error_string() != b""
    assert lib.dmpnn_rank_append(C.byref(_append_args(n_mols=0)), None) == 0       # an empty batch: OK, nothing launched, nothing read
    assert lib.dmpnn_rank_append(C.byref(_append_args(n_mols=0, row0=9)), None) == 0
    assert lib.dmpnn_last_launch_count() == n0


def _rank_args(**kw):
    a = _lib.RankArgs()
    a.keys, a.labels, a.rows, a.n_tasks, a.pooled, a.out = P, P, 300, 3, 1, P
    a.ws, a.ws_bytes = None, 0   # (the LAST rule)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_rank_metrics_refusals_are_codes_and_launch_nothing():
    lib = _lib.load()
    n0 = lib.dmpnn_last_launch_count()
    cap = _lib.RANK_MAX_ROWS
    assert lib.dmpnn_rank_metrics(None, None) == -1 and lib.dmpnn_rank_metrics_ws_bytes(None) == 0
    # the partials: 6 words of 8 bytes per workgroup of 256 rows — 2 x 3 per task, 4 pooled — in 256-byte units
    assert lib.dmpnn_rank_metrics_ws_bytes(C.byref(_rank_args())) == 512 and lib.dmpnn_rank_metrics_ws_bytes(C.byref(_rank_args(pooled=0))) == 512
    assert lib.dmpnn_rank_metrics_ws_bytes(C.byref(_rank_args(rows=256, n_tasks=1, pooled=0))) == 256
    assert lib.dmpnn_rank_metrics_ws_bytes(C.byref(_rank_args(rows=0))) == 0
    for kw in (dict(), dict(ws=P, ws_bytes=511), dict(pooled=0), dict(rows=cap, n_tasks=1), dict(rows=cap, pooled=0), dict(rows=cap // 4, n_tasks=4)):
        assert lib.dmpnn_rank_metrics(C.byref(_rank_args(**kw)), None) == -3, kw
        assert b"workspace" in lib.dmpnn_last_error_string()
    bad = [dict(rows=-1), dict(n_tasks=0), dict(n_tasks=-2), dict(n_tasks=1 << 16), dict(pooled=2), dict(pooled=-1), dict(keys=None), dict(labels=None),
           dict(out=None), dict(out=P + 4), dict(ws=P + 4, ws_bytes=1 << 20)]
    for kw in bad:
        assert lib.dmpnn_rank_metrics(C.byref(_rank_args(**kw)), None) == -1, kw
    for kw in (dict(rows=cap + 1, n_tasks=1), dict(rows=cap + 1, pooled=0), dict(rows=cap // 4 + 1, n_tasks=4), dict(rows=cap, n_tasks=2)):
        assert lib.dmpnn_rank_metrics(C.byref(_rank_args(ws=P, ws_bytes=1 << 40, **kw)), None) == -1, kw   # more keys than the cap
        assert b"DMPNN_RANK_MAX_ROWS" in lib.dmpnn_last_error_string()
    assert lib.dmpnn_last_launch_count() == n0


def _ranked_args(transform="sigmoid", n_out=3, loss="bce", kind="binary", **kw):
    r = _lib.ValidateRankArgs()
    v = r.validate
    h = v.predict.head
    h.n_atoms, h.n_mols, h.d_h, h.batch = 40, 10, 8, P
    h.n_layers, h.dims[0], h.dims[1], h.W[0] = 1, 8, n_out, P
    h.loss, h.quantile_alpha = _lib.LOSS[loss], 0.1
    h.preds, h.targets, h.loss_out = P, P, P
    v.predict.transform = _lib.PT_DIRICHLET_BINARY if transform == "dirichlet" else _lib.PREDICT_TRANSFORM[transform]
    v.predict.preds = P
    v.metric_kind, v.threshold, v.stats, v.stats_bytes = _lib.METRIC[kind], 0.5, P, 1 << 20
    r.keys, r.labels, r.capacity, r.row0 = P, P, 100, 0
    for k, val in kw.items():
        obj, name = (h, k[5:]) if k.startswith("head_") else ((v, k[9:]) if k.startswith("validate_") else (r, k))
        setattr(obj, name, val)
    return r


def test_validate_head_ranked_refusals_are_codes_and_launch_nothing():
    lib = _lib.load()
    n0 = lib.dmpnn_last_launch_count()
    call = lambda r: lib.dmpnn_validate_head_ranked(C.byref(r), P, 8, None)
    assert lib.dmpnn_validate_head_ranked(None, P, 8, None) == -1 and lib.dmpnn_validate_head_ranked_ws_bytes(None) == 0
    # what passes every argument rule ends at the workspace rule (none given): DMPNN_ENOSPC, nothing launched
    for r in (_ranked_args(), _ranked_args("dirichlet", 6, "dirichlet", head_n_classes=2), _ranked_args(capacity=10), _ranked_args(capacity=30, row0=20)):
        assert call(r) == -3 and b"workspace" in lib.dmpnn_last_error_string()
        assert lib.dmpnn_validate_head_ranked_ws_bytes(C.byref(r)) == lib.dmpnn_validate_head_ws_bytes(C.byref(r.validate)) > 0
    # ... and with a workspace, at the buffer rule: DMPNN_ENOSPC again (a capacity overflow)
    for kw in (dict(capacity=9), dict(capacity=30, row0=21), dict(capacity=30, row0=31)):
        assert call(_ranked_args(head_ws=P, head_ws_bytes=1 << 30, **kw)) == -3, kw
        assert b"do not fit" in lib.dmpnn_last_error_string()
    bad = [_ranked_args("unscale", 3, "mse", kind="regression"), _ranked_args("softmax", 6, "ce", kind="multiclass", head_n_classes=3),
           _ranked_args("sigmoid", 3, "bce", kind="none"), _ranked_args(kind="regression"), _ranked_args(keys=None), _ranked_args(labels=None),
           _ranked_args(capacity=-1), _ranked_args(row0=-1), _ranked_args(head_targets=None), _ranked_args(validate_stats=None),
           _ranked_args(validate_threshold=float("nan")), _ranked_args(validate_metric_targets=P, validate_ld_mt=2), _ranked_args(head_gHv=P)]
    for i, r in enumerate(bad):
        r.validate.predict.head.ws, r.validate.predict.head.ws_bytes = P, 1 << 30
        assert call(r) == -1, i
    assert lib.dmpnn_last_launch_count() == n0


# ---- bookkeeping ---------------------------------------------------------------------------------------------------------------------
def _same(a: RankStats, b: RankStats):
    return a.rows == b.rows and torch.equal(a.keys[:a.rows], b.keys[:b.rows]) and torch.equal(a.labels[:a.rows], b.labels[:b.rows])


def test_three_uneven_pieces_and_merge_equal_one_buffer_of_the_concatenation():
    S, T = rh.make_inputs(300, 4, seed=2)
    whole = _filled(S, T, cap=320)
    cuts = ((0, 1), (1, 130), (130, 300))
    acc, parts = RankStats(4, 300), []
    for a, b in cuts:
        acc.update(torch.from_numpy(S[a:b]), torch.from_numpy(T[a:b]))
        parts.append(_filled(S[a:b], T[a:b]))
    acc.update(torch.from_numpy(S[:0]), torch.from_numpy(T[:0]))   # an empty batch: nothing
    assert _same(acc, whole) and acc.rows == 300
    merged = RankStats(4, 300)
    for p in parts:
        merged.merge(p)
    assert _same(merged, whole)
    ga, gw = merged.compute(), whole.compute()
    assert ga["roc"] == gw["roc"] and ga["prc"] == gw["prc"] and ga["roc-pooled"] == gw["roc-pooled"] and ga["prc-pooled"] == gw["prc-pooled"]
    for k in gw["per_task"]:
        assert np.array_equal(ga["per_task"][k], gw["per_task"][k], equal_nan=True), k
    with pytest.raises(ValueError):
        merged.merge(parts[0])                                    # full
    with pytest.raises(ValueError):
        RankStats(3, 300).merge(parts[0])                         # another number of tasks
    with pytest.raises(ValueError):
        acc.update(torch.from_numpy(S[:1]), torch.from_numpy(T[:1]))   # does not fit
    assert acc.rows == 300
    with pytest.raises(ValueError):
        RankStats(4, 10).update(torch.zeros(4, 3), torch.zeros(4, 3))  # misshapen
    # a group of two: element 0 is the score
    two = RankStats(4, 300)
    two.update(torch.stack((torch.from_numpy(S), torch.full((300, 4), 9.0)), -1), torch.from_numpy(T))
    assert _same(two, whole)
    merged.reset()
    assert merged.rows == 0
    z = merged.compute()
    assert np.isnan(z["roc"]) and np.isnan(z["prc-pooled"]) and z["per_task"]["n_pos"].tolist() == [0, 0, 0, 0] and z["n_mols"] == 0
    merged.update(torch.from_numpy(S[:7]), torch.from_numpy(T[:7]))
    assert _same(merged, _filled(S[:7], T[:7]))


def test_compute_names_the_cap():
    cap = _lib.RANK_MAX_ROWS
    r = RankStats(2, cap // 2 + 1)
    r.rows = cap // 2 + 1           # (the rows as allocated: not ranked, label 2)
    with pytest.raises(ValueError, match="RANK_MAX_ROWS"):
        r.compute()
    got = r.compute(pooled=False)   # each task alone is inside the cap
    assert got["per_task"]["n_pos"].tolist() == [0, 0] and np.isnan(got["roc"])
    r = RankStats(1, cap + 1)
    r.rows = cap + 1
    with pytest.raises(ValueError, match=str(cap)):
        r.compute(pooled=False)


def test_for_model_takes_binary_predictors_only():
    from chemprop_amd import agg as cagg
    from chemprop_amd import model as cm
    from chemprop_amd.nn import BondMessagePassing

    def ranks(pred):
        return RankStats.for_model(cm.MPNN(BondMessagePassing(d_h=16, depth=2), cagg.MeanAggregation(), pred), capacity=50, device="cpu")

    kw = dict(input_dim=16, hidden_dim=8)
    for pred, t in ((cm.BinaryClassificationFFN(n_tasks=4, **kw), 4), (cm.BinaryDirichletFFN(n_tasks=2, **kw), 2)):
        r = ranks(pred)
        assert (r.n_tasks, r.capacity, r.rows, r.device.type) == (t, 50, 0, "cpu")
    for pred in (cm.RegressionFFN(n_tasks=3, **kw), cm.MulticlassClassificationFFN(5, n_tasks=2, **kw), cm.MveFFN(n_tasks=2, **kw)):
        with pytest.raises(NotImplementedError):
            ranks(pred)

