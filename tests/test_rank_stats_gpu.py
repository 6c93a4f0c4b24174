"""``dmpnn_rank_append`` / ``dmpnn_rank_metrics`` / ``dmpnn_validate_head_ranked`` on the MI355X against ``rank_harness``'s float64 references.

Shapes — the seams of the layout (workgroups of 256 rows, waves of 64, LDS tiles of ``RANK_TILE`` pairs): ``n`` in {1, 2, 63, 64, 65, 255, 256,
257, ``RANK_TILE`` - 1, ``RANK_TILE``, ``RANK_TILE`` + 1, 2 ``RANK_TILE`` + 3} x ``t`` in {1, 3, 5}; the groups 1 / 2 and one, two or three
append calls of uneven sizes rotate over them (a call of one row; a last call that ends exactly at ``capacity``).  ``preds`` / ``targets``
are views into wider tables whose pad columns — and, with group 2, the second element of every group — hold values that would change the
result if read.  Inputs: ``rank_harness.make_inputs`` (ties, denormals, signed zeros, saturation, NaN targets, one-class columns, targets
of exactly 0.5, two predictions that are not finite).

Conditions: ``keys`` / ``labels`` after the appends equal the torch restatement (``metrics.rank_keys``) and rows beyond ``rows`` are as they
were; ``n_pos``, ``n_neg``, ``n_skipped``, ``n_thresholds`` and ``U2`` are EXACT, per task and pooled; ``roc`` equals ``U2 / (2.0 P N)`` evaluated in
float64 on the host bit for bit (two correctly rounded operations on exact integers); ``roc`` and ``prc`` lie within ``(n_ranked + 8) 2^-52``
absolute of the sorted curves — each is a sum of at most ``n_ranked`` non-negative terms that totals at most 1, each term formed with a
handful of roundings: derived, not measured; NaN exactly where a class is absent; two runs from the same buffer give identical bits;
guards behind ``out``, the workspace, ``keys`` and ``labels`` are intact.  One ``RANKBAR`` line is printed before each judgement."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import rank_harness as rh
from chemprop_amd import _lib, engine
from chemprop_amd.metrics import MetricStats, RankStats, rank_keys
from predict_harness import same_bits

pytestmark = pytest.mark.gpu
TILE = _lib.RANK_TILE
N_ROWS = (1, 2, 63, 64, 65, 255, 256, 257, TILE - 1, TILE, TILE + 1, 2 * TILE + 3)
N_TASKS = (1, 3, 5)
GUARD, PAD_P, PAD_T = 5, 3, 2
KEY_GUARD, LAB_GUARD = 0x5A5A5A5A, 0xA5


@functools.lru_cache(maxsize=None)
def _inputs(n, t, seed):
    return rh.make_inputs(n, t, seed)


@functools.lru_cache(maxsize=None)
def _reference(n, t, seed):
    """Per column and pooled: the sorted curves and the all-pairs ``U2`` (computed once, shared, never changed)."""
    S, T = _inputs(n, t, seed)
    cols = [(rh.ref_curves(S[:, j], T[:, j]), rh.ref_u2(S[:, j], T[:, j])) for j in range(t)]
    pooled = (rh.ref_curves(S.reshape(-1), T.reshape(-1)), rh.ref_u2(S.reshape(-1), T.reshape(-1)) if n * t <= 2 * TILE + 3 else None)
    return cols, pooled


def _cuts(n, calls):
    """``calls`` uneven pieces of ``[0, n)``: two — a call of one row first; three — a call of one row last."""
    if calls == 1 or n < 2:
        return [(0, n)]
    if calls == 2 or n < 3:
        return [(0, 1), (1, n)]
    return [(0, n // 3), (n // 3, n - 1), (n - 1, n)]


class Buffer:
    """One shape on the device: the wide input tables, the epoch's buffer with guard elements behind it (and ``spare`` unused rows
    inside it), ``out`` with NaN guard doubles and the workspace with guard bytes."""

    def __init__(self, n, t, group, spare, dev):
        self.n, self.t, self.group, self.cap, self.dev, self.lib = n, t, group, n + spare, dev, _lib.load()
        self.keys = torch.full((self.cap * t + GUARD,), KEY_GUARD, dtype=torch.int32, device=dev)
        self.labels = torch.full((self.cap * t + GUARD,), LAB_GUARD, dtype=torch.uint8, device=dev)
        a = self._rank_args(1)
        self.ws_bytes = int(self.lib.dmpnn_rank_metrics_ws_bytes(C.byref(a)))
        self.ws = torch.full((self.ws_bytes + 64,), LAB_GUARD, dtype=torch.uint8, device=dev)
        self.out = torch.full(((t + 1) * 8 + GUARD,), float("nan"), dtype=torch.float64, device=dev)

    def append(self, S, T):
        """The rows of ``S`` / ``T`` through 1, 2 or 3 ``dmpnn_rank_append`` calls; returns the launches of each."""
        n, t, g = self.n, self.t, self.group
        self.Pbuf = torch.full((n, t * g + PAD_P), 1e30, device=self.dev)
        self.Tbuf = torch.full((n, t + PAD_T), 7.0, device=self.dev)
        Sd = torch.from_numpy(S).to(self.dev)
        self.Pbuf[:, 0:t * g:g] = Sd
        if g == 2:
            self.Pbuf[:, 1:t * g:g] = 1.0 - Sd.nan_to_num(0.5, 0.5, 0.5)   # (the other class: the opposite order)
        self.Tbuf[:, :t] = torch.from_numpy(T).to(self.dev)
        launches = []
        for a0, a1 in self.cuts:
            a = _lib.RankAppendArgs()
            a.n_mols, a.n_tasks, a.group = a1 - a0, t, g
            a.preds, a.ld_p = self.Pbuf[a0:].data_ptr(), self.Pbuf.stride(0)
            a.targets, a.ld_t = self.Tbuf[a0:].data_ptr(), self.Tbuf.stride(0)
            a.keys, a.labels, a.capacity, a.row0 = self.keys.data_ptr(), self.labels.data_ptr(), self.cap, a0
            with engine._OnDevice(self.dev):
                rc = self.lib.dmpnn_rank_append(C.byref(a), engine._stream_ptr(self.dev))
            launches.append(int(self.lib.dmpnn_last_launch_count()))
            _lib.check(rc, "dmpnn_rank_append")
        return launches

    def _rank_args(self, pooled):
        a = _lib.RankArgs()
        a.keys, a.labels, a.rows, a.n_tasks, a.pooled = self.keys.data_ptr(), self.labels.data_ptr(), self.n, self.t, pooled
        return a

    def metrics(self, pooled=1):
        self.out[:(self.t + 1) * 8] = 123.0
        a = self._rank_args(pooled)
        a.out, a.ws, a.ws_bytes = self.out.data_ptr(), self.ws.data_ptr(), self.ws_bytes
        with engine._OnDevice(self.dev):
            rc = self.lib.dmpnn_rank_metrics(C.byref(a), engine._stream_ptr(self.dev))
        self.launches = int(self.lib.dmpnn_last_launch_count())
        _lib.check(rc, "dmpnn_rank_metrics")
        torch.cuda.synchronize()
        return self.out[:(self.t + 1) * 8].cpu().reshape(self.t + 1, 8)

    def untouched(self):
        n, t, bad = self.n, self.t, []
        if not bool((self.keys[n * t:] == KEY_GUARD).all()) or not bool((self.labels[n * t:] == LAB_GUARD).all()):
            bad.append("rows beyond `rows` or the guards behind keys / labels written")
        if not bool(torch.isnan(self.out[(t + 1) * 8:]).all()):
            bad.append("guard doubles behind out written")
        if not bool((self.ws[self.ws_bytes:] == LAB_GUARD).all()):
            bad.append("guard bytes behind the workspace written")
        if not bool((self.Pbuf[:, t * self.group:] == 1e30).all()) or not bool((self.Tbuf[:, t:] == 7.0).all()):
            bad.append("inputs written")
        return bad


def _judge(tag, row, ref, u2_pairs, fails):
    """One row of ``out`` against one column's references."""
    row = row.numpy()
    want = [ref["P"], ref["N"], ref["n_skipped"], ref["n_thresholds"], ref["U2"]]
    exact = [float(x) for x in want] == row[:5].tolist() and (u2_pairs is None or float(u2_pairs) == row[4]) and row[7] == 0
    both = ref["P"] > 0 and ref["N"] > 0
    b = rh.bar(ref["n_ranked"])
    for name, k in (("roc", 5), ("prc", 6)):
        print(f"RANKBAR {tag} {name} got={row[k]!r} want={ref[name]!r} bar={b:.3e} counts_exact={exact}")
    if not exact:
        fails.append(f"{tag}: counts {row[:5].tolist()} / slot 7 {row[7]} != {want} (all-pairs U2 {u2_pairs})")
    for name, k in (("roc", 5), ("prc", 6)):
        if not both:
            if not np.isnan(row[k]):
                fails.append(f"{tag}: {name} = {row[k]} without both classes")
        elif not abs(row[k] - ref[name]) <= b:
            fails.append(f"{tag}: {name} {row[k]!r} vs {ref[name]!r}: {abs(row[k] - ref[name]):.3e} beyond the bar {b:.3e}")
    if both and row[5] != row[4] / (2.0 * row[0] * row[1]):
        fails.append(f"{tag}: roc {row[5]!r} is not U2 / (2 P N) = {row[4] / (2.0 * row[0] * row[1])!r} bit for bit")


@pytest.mark.parametrize("t", N_TASKS)
def test_every_seam_through_the_c_abi(t, gpu_device):
    dev, fails = gpu_device, []
    ti = N_TASKS.index(t)
    combos = set()
    for i, n in enumerate(N_ROWS):
        group, calls = 1 + (i + ti) % 2, 1 + (i + 2 * ti) % 3
        spare = 0 if calls >= 2 and i % 2 == 0 else 3   # (0: the last call ends exactly at capacity)
        seed = 7 * i + ti
        tag = f"n{n}-t{t}-g{group}-calls{calls}-spare{spare}"
        S, T = _inputs(n, t, seed)
        cols, pooled = _reference(n, t, seed)
        buf = Buffer(n, t, group, spare, dev)
        buf.cuts = _cuts(n, calls)
        combos.add((group, len(buf.cuts), spare == 0))
        launches = buf.append(S, T)
        if launches != [1] * len(buf.cuts):
            fails.append(f"{tag}: launches of the appends {launches}")
        wk, wl = rank_keys(torch.from_numpy(S), torch.from_numpy(T))
        if not torch.equal(buf.keys[:n * t].cpu(), wk.reshape(-1)) or not torch.equal(buf.labels[:n * t].cpu(), wl.reshape(-1)):
            fails.append(f"{tag}: keys / labels differ from the restatement")
        got = buf.metrics(1)
        if buf.launches != 4:
            fails.append(f"{tag}: {buf.launches} launches with the pooled row")
        again = buf.metrics(1)
        if not torch.equal(got.view(torch.int64), again.view(torch.int64)):
            fails.append(f"{tag}: two runs from the same buffer differ in bits")
        for j in range(t):
            _judge(f"{tag}-col{j}-pattern{rh.pattern_of(j, seed)}", got[j], cols[j][0], cols[j][1], fails)
        _judge(f"{tag}-pooled", got[t], pooled[0], pooled[1], fails)
        if pooled[0]["n_skipped"] != sum(c[0]["n_skipped"] for c in cols):
            fails.append(f"{tag}: the harness' pooled n_skipped is not the sum over tasks")
        alone = buf.metrics(0)
        if buf.launches != 2 or not torch.equal(alone[:t].view(torch.int64), got[:t].view(torch.int64)) or not bool((alone[t] == 123.0).all()):
            fails.append(f"{tag}: pooled = 0 — {buf.launches} launches, other per-task bits or a written pooled row")
        fails += [f"{tag}: {b}" for b in buf.untouched()]
    assert {(g, c) for g, c, _ in combos} >= {(g, c) for g in (1, 2) for c in (1, 2, 3)} and any(e for _, c, e in combos if c > 1)
    assert not fails, fails


def test_an_empty_epoch_launches_nothing(gpu_device):
    buf = Buffer(0, 3, 1, 4, gpu_device)
    buf.Pbuf = buf.Tbuf = torch.zeros(0, 8, device=gpu_device)
    got = buf.metrics(1).numpy()
    assert buf.launches == 0 and np.all(got[:, :5] == 0) and np.all(np.isnan(got[:, 5:7])) and np.all(got[:, 7] == 0)
    buf.group, buf.Pbuf, buf.Tbuf = 1, torch.full((0, 3), 1e30, device=gpu_device), torch.full((0, 3), 7.0, device=gpu_device)
    assert not buf.untouched()


def test_rank_stats_on_device_tensors_is_the_abi(gpu_device):
    """``RankStats.update`` / ``merge`` / ``compute`` on device tensors — also on views into wider tables — against the CPU ``RankStats``."""
    dev, n, t, seed = gpu_device, 300, 3, 5
    S, T = rh.make_inputs(n, t, seed)
    cpu = RankStats(t, n)
    cpu.update(torch.from_numpy(S), torch.from_numpy(T))
    wide_p, wide_t = torch.full((n, t + 4), 1e30, device=dev), torch.full((n, t + 2), 7.0, device=dev)
    wide_p[:, :t], wide_t[:, :t] = torch.from_numpy(S).to(dev), torch.from_numpy(T).to(dev)
    a, b = RankStats(t, n, device=dev), RankStats(t, 170, device=dev)
    a.update(wide_p[:130, :t], wide_t[:130, :t])
    b.update(torch.stack((wide_p[130:, :t], wide_p[130:, :t] * 0 + 9), -1).contiguous(), wide_t[130:, :t].contiguous())   # a group of two
    a.merge(b)
    assert a.rows == n and torch.equal(a.keys.cpu(), cpu.keys) and torch.equal(a.labels.cpu(), cpu.labels)
    with pytest.raises(ValueError):
        a.update(wide_p[:1, :t], wide_t[:1, :t])
    with pytest.raises(ValueError):
        a.update(torch.from_numpy(S[:1]), torch.from_numpy(T[:1]))   # a batch on another device
    _compare(a.compute(), cpu.compute(), n * t)
    assert "roc-pooled" not in a.compute(pooled=False)


def _compare(got, want, n_ranked):
    """Two ``RankStats.compute()`` dictionaries: counts and ``U2`` exact, ``roc`` bit-equal, ``prc`` within the bar."""
    b = rh.bar(n_ranked)
    for k in ("n_pos", "n_neg", "n_thresholds", "n_skipped", "U2"):
        assert np.array_equal(got["per_task"][k], want["per_task"][k]), k
        assert got["pooled"][k] == want["pooled"][k], k
    assert np.array_equal(got["per_task"]["roc"], want["per_task"]["roc"], equal_nan=True)
    for g, w in zip(list(got["per_task"]["prc"]) + [got["prc-pooled"], got["prc"]], list(want["per_task"]["prc"]) + [want["prc-pooled"], want["prc"]]):
        print(f"RANKBAR compute prc got={g!r} want={w!r} bar={b:.3e}")
        assert (np.isnan(g) and np.isnan(w)) or abs(g - w) <= b
    assert got["roc-pooled"] == want["roc-pooled"] or (np.isnan(got["roc-pooled"]) and np.isnan(want["roc-pooled"]))


@pytest.mark.parametrize("head", ["binary", "dirichlet-binary"])
def test_validate_with_ranks_is_validate_plus_one_launch(head, gpu_device):
    """Three validation batches through ``MPNN.validate(..., stats=, ranks=)`` on ``tests/test_validate_gpu.py``'s tiny models."""
    from test_validate_gpu import HEADS, N_MOLS, _batch, _FixedBlock, _model, _result_dict

    dev, lib = gpu_device, _lib.load()
    t = HEADS[head][1]
    model = _model(head, None, dev)
    plain, with_ranks, warm = (MetricStats.for_model(model) for _ in range(3))
    ranks, flipped = RankStats.for_model(model, capacity=3 * N_MOLS), RankStats.for_model(model, capacity=3 * N_MOLS)
    assert (ranks.n_tasks, ranks.capacity, ranks.device.type) == (t, 3 * N_MOLS, "cuda")
    cpu, cpu_flipped, batches = RankStats(t, 3 * N_MOLS), RankStats(t, 3 * N_MOLS), []
    for seed in range(3):
        bmg, kw = _batch(head, None, seed, dev)
        batches.append((bmg, kw))
        with _FixedBlock(model, bmg):
            model.validate(bmg, stats=warm, **kw)                      # (the split images are ready now)
            ref = model.validate(bmg, stats=plain, **kw)
            n_plain = int(lib.dmpnn_last_launch_count())
            got = model.validate(bmg, stats=with_ranks, ranks=ranks, **kw)
            assert int(lib.dmpnn_last_launch_count()) == n_plain + 1
            assert same_bits(_result_dict(ref), _result_dict(got)) == []
            assert ranks.rows == (seed + 1) * N_MOLS
            other = torch.where(kw["targets"].isfinite(), 1.0 - kw["targets"], kw["targets"])
            model.validate(bmg, stats=warm, ranks=flipped, metric_targets=other, **kw)
        cpu.update(got.preds.cpu(), kw["targets"].cpu())
        cpu_flipped.update(got.preds.cpu(), other.cpu())
    assert torch.equal(plain.stats.cpu().view(torch.int64), with_ranks.stats.cpu().view(torch.int64))
    assert torch.equal(ranks.keys.cpu(), cpu.keys) and torch.equal(ranks.labels.cpu(), cpu.labels)
    _compare(ranks.compute(), cpu.compute(), 3 * N_MOLS * t)
    _compare(flipped.compute(), cpu_flipped.compute(), 3 * N_MOLS * t)
    assert not torch.equal(flipped.labels, ranks.labels)
    # a batch that does not fit: refused before any launch, the counter as it was
    small = RankStats.for_model(model, capacity=N_MOLS + 5)
    bmg, kw = batches[0]
    with _FixedBlock(model, bmg):
        model.validate(bmg, stats=warm, ranks=small, **kw)
        n0 = int(lib.dmpnn_last_launch_count())
        with pytest.raises(ValueError):
            model.validate(bmg, stats=warm, ranks=small, **kw)
        assert small.rows == N_MOLS and int(lib.dmpnn_last_launch_count()) == n0
    with pytest.raises(ValueError):
        model.validate(bmg, stats=warm, ranks=RankStats(t + 1, 100, device=dev), **kw)
    # ranks on another device: the one-call path steps aside (None), and the module path refuses the append
    from chemprop_amd.predict import fused_validate

    elsewhere = RankStats(t, 100)
    with torch.no_grad(), _FixedBlock(model, bmg):
        assert fused_validate(model, bmg, stats=warm, ranks=elsewhere, **kw) is None and elsewhere.rows == 0
        assert fused_validate(model, bmg, stats=warm, ranks=None, **kw) is not None
    with pytest.raises(ValueError):
        model.validate(bmg, stats=warm, ranks=elsewhere, **kw)
    # training mode takes the module path: the same counts come out
    model.train()
    module_path = RankStats.for_model(model, capacity=3 * N_MOLS)
    for bmg, kw in batches:
        model.validate(bmg, stats=warm, ranks=module_path, **kw)
    want, got = cpu.compute()["per_task"], module_path.compute()["per_task"]
    for k in ("n_pos", "n_neg", "n_skipped"):
        assert np.array_equal(got[k], want[k]), k
