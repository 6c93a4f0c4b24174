"""``dmpnn_metric_stats`` on the MI355X against the CPU float64 ``MetricStats.update`` on the same tensors.

Shapes — the seams of the layout (row blocks of 128 molecules, column blocks of 256 tasks, the power-of-two column count ``C`` below
them): ``n_mols`` in {1, 127, 128, 129, 300} x ``n_tasks`` in {1, 3, 64, 65, 257}, the groups 1 / 2 / 4 and the class counts 2 / 3 / 16
rotating over them, ``ld_p`` and ``ld_t`` wider than the row.  Inputs (``metric_harness.make_inputs``): 10 % NaN targets and one all-NaN
column, both bounds, predictions exactly at the threshold and exactly equal to their target, two equal maxima, classes out of range.

Conditions: counts (``n``, the confusion cells, TP / FP / TN / FN, the header's calls and molecules) are EXACT; sums are within ``1e-12
sum |x|`` of the reference — double summation in any order errs by at most ``(n - 1) 2^-53 sum |x|``, and at most 300 terms meet per
slot and call, about ``3.3e-14 sum |x|``: derived, not measured (the scale is the sum of the absolute terms plus the magnitude the
buffer started from); two runs from the same starting buffer give identical bits; NaN guard doubles behind ``stats`` and guard bytes
behind the workspace are intact.  Every comparison prints one ``STATBAR`` line before it is judged."""
import ctypes as C

import numpy as np
import pytest
import torch

import metric_harness as mh
from chemprop_amd import _lib, engine
from chemprop_amd.metrics import MetricStats

pytestmark = pytest.mark.gpu
N_MOLS, N_TASKS = (1, 127, 128, 129, 300), (1, 3, 64, 65, 257)
WIDTHS = dict(regression=(1, 2, 4), binary=(1, 2), multiclass=(2, 3, 16))
GUARD, PAD_P, PAD_T = 3, 5, 3
THR = 0.5


def _scale(kind, nc, inp, loss):
    return mh.ref_stats(kind, inp["P"].numpy(), inp["T"].numpy(), None if "lt" not in inp else inp["lt"].numpy(),
                        None if "gt" not in inp else inp["gt"].numpy(), THR, nc, loss, abs_terms=True)


class Stage:
    """One shape on the device: ``preds`` / ``targets`` as views into wider tables (the pad columns hold values that would be seen if
    read), ``stats`` with NaN guard doubles behind it, the workspace with guard bytes behind it."""

    def __init__(self, kind, n, t, width, dev, n_cap=None):
        self.kind, self.t, self.width, self.nc, self.dev, self.lib = kind, t, width, (width if kind == "multiclass" else 0), dev, _lib.load()
        n_cap = n_cap or n
        self.Pbuf = torch.full((n_cap, t * width + PAD_P), 1e30, device=dev)
        self.Tbuf = torch.full((n_cap, t + PAD_T), 7.0, device=dev)
        self.lt = torch.zeros(n_cap, t, dtype=torch.uint8, device=dev)
        self.gt = torch.zeros(n_cap, t, dtype=torch.uint8, device=dev)
        self.nd = int(self.lib.dmpnn_metric_stats_doubles(_lib.METRIC[kind], t, self.nc))
        self.stats = torch.full((self.nd + GUARD,), float("nan"), dtype=torch.float64, device=dev)
        self.loss = torch.zeros(2, device=dev)
        a = _lib.MetricArgs()
        a.kind, a.n_mols, a.n_tasks, a.n_classes, a.group = _lib.METRIC[kind], n_cap, t, self.nc, (1 if kind == "multiclass" else width)
        self.ws_bytes = int(self.lib.dmpnn_metric_stats_ws_bytes(C.byref(a)))
        self.ws = torch.full((self.ws_bytes + 64,), 0xA5, dtype=torch.uint8, device=dev)

    def run(self, inp, start, loss=None, n=None):
        """One call on the rows of ``inp`` from the starting contents ``start`` (``None``: keep the buffer); returns the buffer on the CPU."""
        n = int(inp["T"].shape[0]) if n is None else n
        t, w = self.t, self.width
        if n:
            self.Pbuf[:n, :t * w] = inp["P"].reshape(n, t * w).to(self.dev)
            self.Tbuf[:n, :t] = inp["T"].to(self.dev)
            if "lt" in inp:
                self.lt[:n], self.gt[:n] = inp["lt"].to(torch.uint8).to(self.dev), inp["gt"].to(torch.uint8).to(self.dev)
        if start is not None:
            self.stats[:self.nd] = start.to(self.dev)
        a = _lib.MetricArgs()
        a.kind, a.n_mols, a.n_tasks, a.n_classes, a.threshold = _lib.METRIC[self.kind], n, t, self.nc, THR
        a.group = 1 if self.kind == "multiclass" else w
        a.preds, a.ld_p, a.targets, a.ld_t = self.Pbuf.data_ptr(), self.Pbuf.stride(0), self.Tbuf.data_ptr(), self.Tbuf.stride(0)
        if "lt" in inp:
            # (the masks are [n, t] bytes without a stride of their own)
            self._m = (self.lt[:n].contiguous(), self.gt[:n].contiguous())
            a.lt_mask, a.gt_mask = self._m[0].data_ptr(), self._m[1].data_ptr()
        if loss is not None:
            self.loss.copy_(torch.as_tensor(loss, dtype=torch.float32))
            a.loss = self.loss.data_ptr()
        a.stats, a.stats_bytes, a.ws, a.ws_bytes = self.stats.data_ptr(), self.nd * 8, self.ws.data_ptr(), self.ws_bytes
        with engine._OnDevice(self.dev):
            rc = self.lib.dmpnn_metric_stats(C.byref(a), engine._stream_ptr(self.dev))
        self.launches = int(self.lib.dmpnn_last_launch_count())
        _lib.check(rc, "dmpnn_metric_stats")
        torch.cuda.synchronize()
        return self.stats[:self.nd].cpu()

    def untouched(self):
        bad = []
        if not bool(torch.isnan(self.stats[self.nd:]).all()):
            bad.append("guard doubles behind stats written")
        if not bool((self.ws[self.ws_bytes:] == 0xA5).all()):
            bad.append("guard bytes behind the workspace written")
        if not bool((self.Pbuf[:, self.t * self.width:] == 1e30).all()) or not bool((self.Tbuf[:, self.t:] == 7.0).all()):
            bad.append("inputs written")
        return bad


def _reference(kind, t, nc, batches, start):
    """The CPU float64 ``update`` over ``batches`` [(inp, loss)] from the starting contents ``start``."""
    s = MetricStats(kind, t, nc, THR)
    s.stats.copy_(start)
    for inp, loss in batches:
        s.update(inp["P"], inp["T"], inp.get("lt"), inp.get("gt"), loss=None if loss is None else torch.as_tensor(loss, dtype=torch.float32))
    return s.stats.numpy()


def _count_slots(kind, t, nd):
    """Which doubles of the buffer are counts (exact)."""
    m = np.zeros(nd, bool)
    m[1:4] = True
    if kind == "none":
        return m
    body = m[4:].reshape(t, -1)
    if kind == "regression":
        body[:, 0] = True
        body[:, 7] = True      # (reserved: exactly 0)
    else:
        body[:, :] = True
    return m


def _judge(tag, kind, t, got, ref, scale, fails):
    got, cnt = got.numpy(), _count_slots(kind, t, got.numel())
    exact = bool(np.array_equal(got[cnt], ref[cnt]))
    err = np.abs(got - ref)
    bar = 1e-12 * scale
    worst = float(np.max(np.where(scale > 0, err / np.where(scale > 0, scale, 1), np.where(err > 0, np.inf, 0))))
    print(f"STATBAR {tag} counts_exact={exact} worst err / sum|x| = {worst:.3e} (bar 1e-12)")
    if not exact:
        fails.append(f"{tag}: counts differ at {np.nonzero(cnt & (got != ref))[0][:8].tolist()}")
    if not bool(np.all(err <= bar)):
        fails.append(f"{tag}: sums beyond the bar, worst {worst:.3e}")


@pytest.mark.parametrize("kind", list(WIDTHS))
def test_every_seam_against_the_cpu_update(kind, gpu_device):
    dev, fails = gpu_device, []
    widths = WIDTHS[kind]
    for i, n in enumerate(N_MOLS):
        for j, t in enumerate(N_TASKS):
            width = widths[(i + j) % len(widths)]
            nc = width if kind == "multiclass" else 0
            tag = f"{kind}-n{n}-t{t}-w{width}"
            inp = mh.make_inputs(kind, n, t, width, seed=31 * i + j, thr=THR)
            loss = (0.625 + 0.01 * j, float(inp["T"].isfinite().sum()))
            st = Stage(kind, n, t, width, dev)
            start = torch.arange(st.nd, dtype=torch.float64) % 5   # (small integers: counts stay exact on top of them)
            got = st.run(inp, start, loss)
            assert st.launches == 2, (tag, st.launches)
            again = st.run(inp, start, loss)
            if not torch.equal(got.view(torch.int64), again.view(torch.int64)):
                fails.append(f"{tag}: two runs from the same starting buffer differ in bits")
            ref = _reference(kind, t, nc, [(inp, loss)], start)
            _judge(tag, kind, t, got, ref, _scale(kind, nc, inp, loss) + np.abs(start.numpy()), fails)
            fails += [f"{tag}: {b}" for b in st.untouched()]
    assert not fails, fails


@pytest.mark.parametrize("kind,t,width", [("regression", 3, 2), ("binary", 65, 1), ("multiclass", 3, 16), ("none", 4, 1)])
def test_three_calls_accumulate_and_an_empty_batch_changes_nothing(kind, t, width, gpu_device):
    dev, fails = gpu_device, []
    nc = width if kind == "multiclass" else 0
    cuts = ((0, 1), (1, 130), (130, 300))
    if kind == "none":
        whole = dict(P=torch.zeros(300, t, 1), T=torch.randn(300, t, generator=torch.Generator().manual_seed(3)))
    else:
        whole = mh.make_inputs(kind, 300, t, width, seed=77, thr=THR)
    parts = [{k: v[a:b].contiguous() for k, v in whole.items()} for a, b in cuts]
    losses = [(0.5 + i, float(p["T"].isfinite().sum())) for i, p in enumerate(parts)]
    st = Stage(kind, 300, t, width, dev, n_cap=300)
    zero = torch.zeros(st.nd, dtype=torch.float64)
    for k, (p, l) in enumerate(zip(parts, losses)):
        got = st.run(p, zero if k == 0 else None, l)
        assert st.launches == (1 if kind == "none" else 2)
    before = got.clone()
    after = st.run(parts[0], None, losses[0], n=0)   # n_mols == 0: nothing launched, the buffer as it was
    assert st.launches == 0 and torch.equal(before.view(torch.int64), after.view(torch.int64))
    n_fin = sum(l[1] for l in losses)
    mean = sum(l[0] * l[1] for l in losses) / n_fin
    ref_acc = _reference(kind, t, nc, list(zip(parts, losses)), zero)
    ref_one = _reference(kind, t, nc, [(whole, None)], zero)
    scale = _scale(kind, nc, whole, (mean, n_fin)) if kind != "none" else np.array([mean * n_fin, n_fin, 3, 300.0])
    _judge(f"{kind}-three-calls", kind, t, got, ref_acc, scale, fails)
    # ... and the reference on the concatenation (one call): the body within the same bound, the header's calls apart
    g = got.numpy()
    if not bool(np.all(np.abs(g[4:] - ref_one[4:]) <= 1e-12 * scale[4:])):
        fails.append("the accumulated body differs from the one-shot reference on the concatenation")
    assert g[2] == 3 and g[3] == 300 and g[1] == n_fin and abs(g[0] - mean * n_fin) <= 1e-12 * abs(mean * n_fin)
    fails += st.untouched()
    assert not fails, fails


@pytest.mark.parametrize("kind,t,width", [("regression", 5, 4), ("binary", 3, 2), ("multiclass", 2, 3)])
def test_metric_stats_update_on_device_tensors_is_the_stage(kind, t, width, gpu_device):
    """``MetricStats.update`` on device tensors — also on views into wider tables — leaves the bits the ABI call leaves."""
    dev = gpu_device
    nc = width if kind == "multiclass" else 0
    inp = mh.make_inputs(kind, 129, t, width, seed=5, thr=THR)
    loss = (1.5, float(inp["T"].isfinite().sum()))
    st = Stage(kind, 129, t, width, dev)
    want = st.run(inp, torch.zeros(st.nd, dtype=torch.float64), loss)
    s = MetricStats(kind, t, nc, THR, device=dev)
    Pd = inp["P"].to(dev) if kind == "multiclass" or width > 1 else inp["P"].to(dev).reshape(129, t)
    masks = dict(lt_mask=inp["lt"].to(dev), gt_mask=inp["gt"].to(dev)) if "lt" in inp else {}
    s.update(Pd, inp["T"].to(dev), loss=torch.tensor(loss, device=dev), **masks)
    assert torch.equal(s.stats.cpu().view(torch.int64), want.view(torch.int64))
    s.reset()
    s.update(st.Pbuf[:, :t * width], st.Tbuf[:, :t], loss=torch.tensor(loss, device=dev), **masks)   # (views: ld_p, ld_t wider than the rows)
    assert torch.equal(s.stats.cpu().view(torch.int64), want.view(torch.int64))
    ref = _reference(kind, t, nc, [(inp, loss)], torch.zeros(st.nd, dtype=torch.float64))
    fails = []
    _judge(f"{kind}-update", kind, t, s.stats.cpu(), ref, _scale(kind, nc, inp, loss), fails)
    assert not fails, fails
    got, cpu = s.compute(), MetricStats(kind, t, nc, THR)
    cpu.stats.copy_(torch.from_numpy(ref))
    for k, v in cpu.compute().items():
        if k != "per_task":
            assert mh.close(got[k], v), (k, got[k], v)
