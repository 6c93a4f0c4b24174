"""Atom descriptors (``--atom-descriptors-path``; a block built with ``d_vd > 0``: ``H_v' = W_d cat(H_v, V_d) + b_d`` behind finalize,
``message_passing/base.py``) as a stage of its own between the block and the head: ``dmpnn_vd_forward`` / ``dmpnn_vd_backward``
(csrc/dmpnn_vd.hip), ``dmpnn_step_args.vd`` and ``FusedTrainer.step(..., V_d=...)``."""
import copy
import ctypes as C
import itertools

import pytest
import torch

from chemprop_amd import _lib
from conftest import parity_err
from test_head_boundaries import MARGIN
from vd_harness import VdCase, build_inputs, compare, run_layer, yardstick

EINVAL, ENOSPC = -1, -3


# ---- CPU --------------------------------------------------------------------------------------------------------------------------
def test_entry_points_are_exported():
    lib = _lib.load()
    for name in ("dmpnn_vd_forward", "dmpnn_vd_backward", "dmpnn_vd_ws_bytes"):
        assert name in _lib.EXPORTS
        assert getattr(lib, name) is not None
    assert "dmpnn_vd.hip" in _lib.SOURCES


def test_vd_structs_match_the_c_layout(tmp_path):
    """``dmpnn_vd_args`` field by field and ``dmpnn_step_args.vd`` at the offsets the C compiler gives them (include/dmpnn.h)."""
    import os
    import shutil
    import subprocess

    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if cc is None:
        cc = "/opt/rocm/llvm/bin/clang"
    fields = [n for n, _ in _lib.VdArgs._fields_]
    fmt = " ".join(["%zu"] * (len(fields) + 4))
    offs = ",".join(f"offsetof(dmpnn_vd_args, {n})" for n in fields)
    src = tmp_path / "off.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "dmpnn.h"\nint main(void){printf("' + fmt + '\\n",' + offs +
                   ',sizeof(dmpnn_vd_args), offsetof(dmpnn_step_args, vd), sizeof(dmpnn_step_args), offsetof(dmpnn_step_args, extra));return 0;}\n')
    exe = tmp_path / "off"
    inc = os.path.join(os.path.dirname(_lib.__file__), "..", "include")
    subprocess.run([cc, "-I", inc, str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    want = [getattr(_lib.VdArgs, n).offset for n in fields] + [C.sizeof(_lib.VdArgs), _lib.StepArgs.vd.offset, C.sizeof(_lib.StepArgs),
                                                               _lib.StepArgs.extra.offset]
    assert got == want
    assert _lib.StepArgs._fields_[-1][0] == "vd"   # (grown at its end: an older caller's block is a prefix)


def _vd(n=64, d_h=300, d_vd=20, **kw):
    """A consistent argument block on made-up (never dereferenced) addresses."""
    a = _lib.VdArgs()
    D = d_h + d_vd
    a.n_atoms, a.d_h, a.d_vd = n, d_h, d_vd
    a.Hv, a.ldhv, a.V_d, a.ldvd = 0x10000, d_h, 0x20000, max(d_vd, 0)
    a.W_d, a.b_d = 0x30000, 0x40000
    a.out, a.ldout, a.gout, a.ldgout, a.gHv, a.ldghv = 0x50000, D, 0x60000, D, 0x70000, d_h
    a.gW_d, a.gb_d = 0x80000, 0x90000
    a.ws = 0xA0000
    for k, v in kw.items():
        setattr(a, k, v)
    if "ws_bytes" not in kw:
        a.ws_bytes = int(_lib.load().dmpnn_vd_ws_bytes(C.byref(a)))
    return a


def test_layer_refuses_inconsistent_arguments_before_touching_the_device():
    """Null pointers, ``d_vd < 1``, a leading dimension below its width, a width beyond the layer's: ``DMPNN_EINVAL``; a workspace that
    is too small: ``DMPNN_ENOSPC`` — before anything reaches the device (no GPU here: a launch would be ``DMPNN_EHIP``)."""
    lib = _lib.load()

    def call(a, which):
        fn = lib.dmpnn_vd_forward if which == "fwd" else lib.dmpnn_vd_backward
        return int(fn(C.byref(a), None)), lib.dmpnn_last_error_string().decode()

    assert int(lib.dmpnn_vd_ws_bytes(C.byref(_vd()))) > 0
    for which in ("fwd", "bwd"):
        rc, msg = call(_vd(d_vd=0, ws_bytes=1 << 30), which)
        assert rc == EINVAL and "d_vd" in msg, (which, rc, msg)
        rc, msg = call(_vd(d_h=400, d_vd=200, ws_bytes=1 << 30), which)
        assert rc == EINVAL and "beyond" in msg, (which, rc, msg)
        for null in ("Hv", "V_d", "W_d", "ws"):
            rc, msg = call(_vd(**{null: None}), which)
            assert rc == EINVAL and "null" in msg, (which, null, rc, msg)
        for ld, val in (("ldhv", 299), ("ldvd", 19)):
            rc, msg = call(_vd(**{ld: val}), which)
            assert rc == EINVAL and "leading dimension" in msg, (which, ld, rc, msg)
        good = _vd()
        rc, msg = call(_vd(ws_bytes=good.ws_bytes - 1), which)
        assert rc == ENOSPC and "workspace too small" in msg, (which, rc, msg)
    for null in ("b_d", "out"):
        rc, msg = call(_vd(**{null: None}), "fwd")
        assert rc == EINVAL and "null" in msg, (null, rc, msg)
    rc, msg = call(_vd(ldout=319), "fwd")
    assert rc == EINVAL and "ldout" in msg, (rc, msg)
    for null in ("gout", "gHv"):
        rc, msg = call(_vd(**{null: None}), "bwd")
        assert rc == EINVAL and "null" in msg, (null, rc, msg)
    for ld, val in (("ldgout", 319), ("ldghv", 299)):
        rc, msg = call(_vd(**{ld: val}), "bwd")
        assert rc == EINVAL and "leading dimension" in msg, (ld, rc, msg)
    # no atoms: nothing to compute in the forward — OK without touching the device
    assert call(_vd(n=0), "fwd")[0] == 0
    assert int(lib.dmpnn_vd_ws_bytes(C.byref(_vd(d_vd=0, ws_bytes=0)))) == 0


def _step(vd, **kw):
    """``dmpnn_step_args`` around ``vd``, consistent with it (made-up addresses), then ``kw`` as ``"bwd.f.W_d"``-style paths."""
    s = _lib.StepArgs()
    f = s.bwd.f
    f.flags = _lib.F_KEEP
    f.n_atoms, f.n_edges, f.d_h, f.d_v, f.d_e, f.depth = vd.n_atoms, 2 * vd.n_atoms, vd.d_h, 72, 14, 3
    f.out, f.ldout = vd.Hv, vd.ldhv
    s.bwd.gout, s.bwd.ldgout = vd.gHv, vd.ldghv
    s.head.gHv, s.head.ldg = vd.gout, vd.ldgout
    s.head.d_h, s.head.n_atoms, s.head.n_mols = vd.d_h + vd.d_vd, vd.n_atoms, 8
    s.vd = C.pointer(vd)
    for path, v in kw.items():
        obj = s
        *head, last = path.split(".")
        for p in head:
            obj = getattr(obj, p)
        setattr(obj, last, v)
    return s


def test_step_refuses_an_inconsistent_atom_descriptor_stage_before_any_launch():
    """Every consistency rule between the block, the stage and the head (include/dmpnn.h, ``dmpnn_step_args.vd``): ``DMPNN_EINVAL``
    with a message that names the stage; a consistent block gets past them and stops at the stage's own argument checks."""
    lib = _lib.load()
    vd = _vd()

    def call(s):
        return int(lib.dmpnn_train_step(C.byref(s), None)), lib.dmpnn_last_error_string().decode()

    bad = {"bwd.f.W_d": 0x1000, "bwd.f.out": 0x1234000, "bwd.gout": 0x1234000, "head.gHv": 0x1234000, "head.d_h": 300, "head.n_atoms": 65,
           "bwd.f.n_atoms": 63, "head.n_components": 2, "bwd.f.ldout": 304, "head.ldg": 324}
    for path, v in bad.items():
        rc, msg = call(_step(vd, **{path: v}))
        assert rc == EINVAL and "atom-descriptor" in msg, (path, rc, msg)
    extra = (_lib.StepComponent * 1)()   # a second block: the stage takes one
    extra[0].bwd.f.flags, extra[0].bwd.f.d_h = _lib.F_KEEP, 320
    s = _step(vd, **{"head.n_components": 2})
    s.n_extra, s.extra = 1, C.cast(extra, C.POINTER(_lib.StepComponent))
    rc, msg = call(s)
    assert rc == EINVAL and "atom-descriptor" in msg, (rc, msg)
    # consistent, but the stage's own workspace is a byte short: past the step's rules, refused by the stage's check — still no launch
    short = _vd(ws_bytes=vd.ws_bytes - 1)
    rc, msg = call(_step(short))
    assert rc == ENOSPC and "workspace too small" in msg, (rc, msg)
    short = _vd(ldvd=19)
    rc, msg = call(_step(short))
    assert rc == EINVAL and "leading dimension" in msg, (rc, msg)
    # without the stage the old rule holds: head.gHv must be the backward's gout
    s = _step(vd)
    s.vd = None
    rc, msg = call(s)
    assert rc == EINVAL and "head.gHv must be the backward's gout" in msg, (rc, msg)


def test_fused_block_takes_a_block_with_atom_descriptors():
    from chemprop_amd.model import fused_block
    from chemprop_amd.nn import BondMessagePassing

    assert fused_block(BondMessagePassing(d_vd=5)) == fused_block(BondMessagePassing())
    with pytest.raises(NotImplementedError, match="dropout"):
        fused_block(BondMessagePassing(d_vd=5, dropout=0.2))
    with pytest.raises(NotImplementedError, match="beyond"):
        fused_block(BondMessagePassing(d_h=400, d_vd=200))
    for kw in (dict(undirected=True), dict(activation="prelu"), dict(activation=torch.nn.Softplus())):
        with pytest.raises(NotImplementedError):
            fused_block(BondMessagePassing(d_vd=5, **kw))


def test_training_plan_kind_with_the_layer_outside():
    """The block's own rule is unchanged — a forward that carries ``W_d`` never takes the tile plan —; ``vd_outside=True`` answers for
    the block with ``W_d`` taken out, which is what ``FusedTrainer`` runs."""
    from chemprop_amd import synth
    from chemprop_amd.nn import BondMessagePassing, _training_plan_kind, _VALIDATE_FIRST_N

    qm9 = synth.random_batch(64, "qm9", seed=1)
    m = BondMessagePassing(d_vd=4).train()
    object.__setattr__(m, "_dmpnn_batches_checked", _VALIDATE_FIRST_N)
    assert _training_plan_kind(m, qm9) is False
    assert _training_plan_kind(m, qm9, vd_outside=True) == "tiles"
    plain = BondMessagePassing().train()
    object.__setattr__(plain, "_dmpnn_batches_checked", _VALIDATE_FIRST_N)
    assert _training_plan_kind(plain, qm9) == _training_plan_kind(plain, qm9, vd_outside=True) == "tiles"
    assert _training_plan_kind(BondMessagePassing(d_vd=4, undirected=True).train(), qm9, vd_outside=True) is False


# ---- GPU: the layer against float64 -------------------------------------------------------------------------------------------------
def _grid():
    """The whole cross of the sizes; leading dimensions, NULL gradients and mixed-magnitude rows dealt over it by the case's index."""
    cases = []
    for i, (n, h, v) in enumerate(itertools.product((1, 47, 4636, 40000), (4, 64, 300, 320), (1, 3, 8, 50, 200))):
        cases.append(VdCase(n, h, v, pad=(0, 1, 5)[i % 3], want_gW=i % 4 != 1, want_gb=i % 4 != 3, mixed=i % 5 == 2, seed=i))
    cases.append(VdCase(4636, 300, 50, pad=3, want_gW=False, want_gb=False, seed=101))       # the data gradient alone (W_d frozen)
    cases.append(VdCase(4636, 300, 50, pad=0, mixed=True, seed=102))                           # the timed shape, mixed-magnitude rows
    cases.append(VdCase(513, 343, 201, pad=2, seed=103))                                       # the widest layer: 544 columns
    cases.append(VdCase(1025, 31, 7, pad=1, seed=104))                                         # odd everything, the f16 product's first row count
    return cases


@pytest.mark.gpu
@pytest.mark.parametrize("case", _grid(), ids=lambda c: c.id)
def test_layer_against_float64(case, gpu_device):
    """``out``, ``gHv``, ``gW_d``, ``gb_d`` of one forward and one backward call against the float64 restatement: the metric and the bar
    of ``tests/head_harness.py`` (``max|got - ref| / max|ref| <= min(MARGIN max(e32, 2**-23), cap)``, ``MARGIN`` = 32 as in
    ``tests/test_head_boundaries.py``, ``e32`` = the same restatement in float32)."""
    inp = build_inputs(case)
    ref, e32 = yardstick(case, inp)
    got = run_layer(case, inp, gpu_device)
    fails, worst = compare(case, got, ref, e32, MARGIN)
    print(f"VDWORST {case.id} ratio={worst:.2f}")
    assert not fails, (case.id, fails)


@pytest.mark.gpu
def test_layer_without_atoms_zeroes_the_requested_gradients(gpu_device):
    from chemprop_amd import engine
    from vd_harness import vd_args

    case = VdCase(0, 64, 8)
    a, t = vd_args(case, build_inputs(case), gpu_device)
    lib = _lib.load()
    with engine._OnDevice(gpu_device):
        _lib.check(lib.dmpnn_vd_forward(C.byref(a), engine._stream_ptr(gpu_device)), "dmpnn_vd_forward")
        _lib.check(lib.dmpnn_vd_backward(C.byref(a), engine._stream_ptr(gpu_device)), "dmpnn_vd_backward")
    torch.cuda.synchronize()
    assert bool((t["gW_d"] == 0).all()) and bool((t["gb_d"] == 0).all())


# ---- GPU: the step ------------------------------------------------------------------------------------------------------------------
class Scale(torch.nn.Module):
    """A ``V_d_transform`` that is not the identity (the reference's ``ScaleTransform`` in evaluation mode, here always)."""

    def __init__(self, d):
        super().__init__()
        gen = torch.Generator().manual_seed(5)
        self.register_buffer("mean", torch.randn(1, d, generator=gen))
        self.register_buffer("scale", 0.5 + torch.rand(1, d, generator=gen))

    def forward(self, X):
        return (X - self.mean) / self.scale


def make_model(d_vd, d_xd=0, d_h=300, transform=False, act="elu"):
    from chemprop_amd import agg as cagg
    from chemprop_amd.model import MPNN, MSE, RegressionFFN
    from chemprop_amd.nn import BondMessagePassing

    mp = BondMessagePassing(d_h=d_h, depth=3, activation=act, d_vd=d_vd, V_d_transform=Scale(d_vd) if transform else None)
    pred = RegressionFFN(n_tasks=1, input_dim=mp.output_dim + d_xd, hidden_dim=300, n_layers=1, activation=act, criterion=MSE(1.0))
    return MPNN(mp, cagg.NormAggregation(), pred, batch_norm=True)


def step_inputs(n_mols, d_vd, dev, d_xd=0, seed=11, **kw):
    from chemprop_amd import synth

    torch.manual_seed(seed)
    a = make_model(d_vd, d_xd, **kw)
    b = copy.deepcopy(a)
    a, b = a.to(dev).train(), b.to(dev).train()
    bmg = synth.random_batch(n_mols, "qm9", seed=seed + 1)
    bmg.to(dev)
    gen = torch.Generator().manual_seed(seed + 2)
    y = torch.randn(n_mols, 1, generator=gen).to(dev)
    w = (0.5 + torch.rand(n_mols, 1, generator=gen)).to(dev)
    V = torch.randn(int(bmg.V.shape[0]), d_vd, generator=gen).to(dev) if d_vd else None
    X = torch.randn(n_mols, d_xd, generator=gen).to(dev) if d_xd else None
    return a, b, bmg, y, w, V, X


STEP_CASES = {
    "rows-512-vd20": dict(n_mols=512, d_vd=20),
    "chain-512-vd50": dict(n_mols=512, d_vd=50),
    "odd-64-vd3": dict(n_mols=64, d_vd=3),
    "with-X_d": dict(n_mols=512, d_vd=20, d_xd=16),
    "transform": dict(n_mols=64, d_vd=8, transform=True),
    "frozen-W_d": dict(n_mols=64, d_vd=8, frozen=True),
}


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(STEP_CASES))
def test_fused_step_with_atom_descriptors_equals_module_path_over_three_steps(name, gpu_device, monkeypatch):
    """``FusedTrainer.step(bmg, y, w, V_d=V)`` three times against the module path run op by op on a copy of the model —
    ``predictor.train_step(fingerprint(bmg, V_d))`` + ``masked_loss`` + backward + ``torch.optim.Adam`` (eps 1e-4: an entry whose
    gradient is fp32 noise around zero must not move by a full learning rate in the direction of the noise's sign).  With
    ``DMPNN_VALIDATE=never`` the block in front of the layer runs on the tile plan and the tile kernels: the point of the stage."""
    from chemprop_amd.model import FusedTrainer, masked_loss

    monkeypatch.setenv("DMPNN_VALIDATE", "never")
    kw = dict(STEP_CASES[name])
    frozen = kw.pop("frozen", False)
    a, b, bmg, y, w, V, X = step_inputs(dev=gpu_device, **kw)
    if frozen:
        for m in (a, b):
            m.message_passing.W_d.requires_grad_(False)
    w_d0 = a.message_passing.W_d.weight.detach().clone()
    tr = FusedTrainer(a, lr=1e-3, eps=1e-4)
    opt = torch.optim.Adam([p for p in b.parameters() if p.requires_grad], lr=1e-3, eps=1e-4)
    for s in range(3):
        la = float(tr.step(bmg, y, w, V_d=V, X_d=X)[0])
        assert str(tr.last_route).startswith("mega16") and tr._last_plan_tiles, (tr.last_route, tr._last_plan_tiles)
        opt.zero_grad()
        lb = masked_loss(b.predictor.train_step(b.fingerprint(bmg, V, X)), y, w, None, None, None, "mse")
        lb.backward()
        opt.step()
        lb = float(lb.detach())
        print(f"VDSTEP {name} step {s}: fused {la:.8f} module {lb:.8f}")
        assert abs(la - lb) <= (1e-5 if s == 0 else 1e-4) * max(1.0, abs(lb)), (s, la, lb)
    torch.cuda.synchronize()
    assert tr.opt.steps == 3
    for (k, pa), (_, pb) in zip(a.named_parameters(), b.named_parameters()):
        e = parity_err(pa.detach().cpu().numpy(), pb.detach().cpu().numpy())
        print(f"VDSTEP {name} {k}: {e:.2e}")
        assert e <= 1e-4, f"{k}: {e:.2e}"
    for k in ("running_mean", "running_var"):
        assert parity_err(getattr(a.bn, k).cpu().numpy(), getattr(b.bn, k).cpu().numpy()) <= 1e-5, k
    assert int(a.bn.num_batches_tracked) == int(b.bn.num_batches_tracked) == 3
    moved = not torch.equal(a.message_passing.W_d.weight.detach(), w_d0)
    assert moved != frozen   # (the layer learns — or, frozen, stays bit for bit)


@pytest.mark.gpu
def test_staged_step_with_atom_descriptors_equals_the_one_call_step(gpu_device, monkeypatch):
    """The data-parallel form of the step (forward + head, exchange, the layer's and the block's backward, exchange, update: forced on one
    rank) against the one-call step, at the bars ``tests/test_multicomponent.py`` holds for the same comparison."""
    from chemprop_amd.model import FusedTrainer

    a, b, bmg, y, w, V, _ = step_inputs(96, 20, gpu_device)
    ta = FusedTrainer(a, lr=1e-3, eps=1e-4)
    # (four steps: the first two on launched, validated plans; from the third on K0 inside the FORWARD stage)
    la = [float(ta.step(bmg, y, w, V_d=V)[0]) for _ in range(4)]
    monkeypatch.setenv("DMPNN_FORCE_COLLECTIVE", "1")
    tb = FusedTrainer(b, lr=1e-3, eps=1e-4)
    lb = [float(tb.step(bmg, y, w, V_d=V)[0]) for _ in range(4)]
    assert tb._checked == 2
    torch.cuda.synchronize()
    for x, z in zip(la, lb):
        assert abs(x - z) <= 1e-5 * max(1.0, abs(z)), (la, lb)
    for (k, pa), (_, pb) in zip(a.named_parameters(), b.named_parameters()):
        assert parity_err(pa.detach().cpu().numpy(), pb.detach().cpu().numpy()) <= 1e-5, k


@pytest.mark.gpu
def test_fused_step_atom_descriptor_refusals(gpu_device):
    """Missing, unexpected and misshapen ``V_d``: ``ValueError`` (the three refusals of ``X_d``); a model in eval mode: ``RuntimeError``
    as before; nothing of a refused step reaches the optimizer."""
    from chemprop_amd.model import FusedTrainer

    a, _, bmg, y, w, V, _ = step_inputs(32, 6, gpu_device)
    tr = FusedTrainer(a)
    with pytest.raises(ValueError, match="atom descriptors"):
        tr.step(bmg, y, w)
    with pytest.raises(ValueError, match="V_d must be"):
        tr.step(bmg, y, w, V_d=V[:, :5])
    with pytest.raises(ValueError, match="V_d must be"):
        tr.step(bmg, y, w, V_d=V[:-1])
    with pytest.raises(ValueError, match="V_d must live on"):
        tr.step(bmg, y, w, V_d=V.cpu())
    a.eval()
    with pytest.raises(RuntimeError, match="eval mode"):
        tr.step(bmg, y, w, V_d=V)
    a.train()
    assert tr.opt.steps == 0
    plain, _, bmg2, y2, w2, _, _ = step_inputs(32, None, gpu_device)
    with pytest.raises(ValueError, match="takes no atom descriptors"):
        FusedTrainer(plain).step(bmg2, y2, w2, V_d=torch.zeros(int(bmg2.V.shape[0]), 4, device=gpu_device))
    float(tr.step(bmg, y, w, V_d=V)[0])   # (and the accepted call still runs)
    assert tr.opt.steps == 1
