"""bench.py's command line: a plain run times exactly --steps steps and prints one line; --dump-outputs writes what the
last timed step computed; --full holds every side measurement."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bench
from conftest import ROOT, TOL, parity_err


def _parse(monkeypatch, *argv):
    monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
    return bench.parse()


def test_parse_defaults_are_the_plain_run(monkeypatch):
    a = _parse(monkeypatch, "--gpus", "1", "--steps", "7", "--warmup", "2")
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (7, 2, False, None)
    a = _parse(monkeypatch, "--full", "--dump-outputs", "d", "--no-cpu-baseline")
    assert a.full and a.dump_outputs == "d" and a.no_cpu_baseline


def test_parse_rejects_no_timed_steps(monkeypatch):
    with pytest.raises(SystemExit):
        _parse(monkeypatch, "--steps", "0")


def test_dump_outputs_small_arrays_whole(tmp_path):
    import torch

    g = torch.Generator().manual_seed(0)
    arrays = {"out": torch.randn(50, 8, generator=g), "grad.W": torch.randn(4, 4, generator=g, dtype=torch.float64)}
    bench.dump_outputs(str(tmp_path), arrays)
    assert sorted(os.listdir(tmp_path)) == ["grad.W.npy", "out.npy"]
    for k, v in arrays.items():
        a = np.load(tmp_path / f"{k}.npy")
        assert a.dtype == np.float32
        np.testing.assert_array_equal(a, v.float().numpy())


def test_dump_outputs_samples_rows_within_budget(tmp_path, monkeypatch):
    import torch

    monkeypatch.setattr(bench, "DUMP_BYTES_MAX", 3 << 20)
    g = torch.Generator().manual_seed(0)
    arrays = {"out": torch.randn(2000, 300, generator=g), "big": torch.randn(3000, 300, generator=g),
              "w": torch.randn(300, 300, generator=g)}
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), arrays)
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == ["big.npy", "big.rows.npy", "out.npy", "out.rows.npy", "w.npy"]
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in files) <= 3 << 20
    np.testing.assert_array_equal(np.load(tmp_path / "a" / "w.npy"), arrays["w"].numpy())  # (small: whole)
    for k in ("out", "big"):
        rows = np.load(tmp_path / "a" / f"{k}.rows.npy")
        assert rows.dtype == np.float64 and np.all(np.diff(rows) > 0) and 0 < rows.size < arrays[k].shape[0]
        np.testing.assert_array_equal(np.load(tmp_path / "a" / f"{k}.npy"), arrays[k].numpy()[rows.astype(np.int64)])
        # the same sample every run
        np.testing.assert_array_equal(rows, np.load(tmp_path / "b" / f"{k}.rows.npy"))


@pytest.mark.gpu
def test_plain_bench_run_and_its_dump(gpu_device, tmp_path):
    """The plain run's line holds the contract's keys and none of --full's; the dumped output is the forward of the seeded
    inputs bench.py builds (recomputed here on the CPU oracle)."""
    import torch

    from chemprop_amd import synth
    from chemprop_amd.nn import BondMessagePassing
    from oracle import dmpnn_torch as ot

    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "5", "--warmup", "2",
                        "--mols", "64", "--dump-outputs", str(tmp_path)], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 1, lines
    d = json.loads(lines[0])
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup", "config"):
        assert k in d, k
    assert d["steps"] == 5 and d["warmup"] == 2 and d["ms_per_step"] > 0 and d["higher_is_better"] is True
    for k in ("roofline", "cpu_baseline", "train_step", "model_step", "other_configs", "graph_ms_per_step"):
        assert k not in d, k
    got = np.load(tmp_path / "out.npy")
    assert got.dtype == np.float32
    bmg = synth.random_batch(64, "qm9", seed=1000)
    torch.manual_seed(0)
    mp = BondMessagePassing(d_v=int(bmg.V.shape[1]), d_e=int(bmg.E.shape[1]), d_h=300, depth=3).eval()
    with torch.no_grad():
        ref = ot.forward_bmg(bmg, ot.MPWeights.from_module(mp), depth=3)
    assert parity_err(got, ref.numpy()) <= TOL
