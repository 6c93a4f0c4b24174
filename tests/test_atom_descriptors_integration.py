"""``integration.HipMPNN.training_step`` with atom descriptors: a batch ``(bmg, V_d, None, y, ...)`` of a model whose block was built
with ``d_vd`` takes the one-call step (``FusedTrainer.step(..., V_d=V_d)``) instead of the module path.

The reference package is not importable here: the stand-in ``chemprop`` of ``tests/test_multicomponent_integration.py`` is used, with
the one thing its ``BondMessagePassing`` leaves out — the layer ``W_d`` of ``d_vd`` — added the way the reference builds it
(``message_passing/base.py``: ``nn.Linear(d_h + d_vd, d_h + d_vd)``, ``output_dim`` = its width)."""
import copy
import types

import pytest
import torch

from conftest import parity_err
from test_multicomponent_integration import stub_chemprop  # noqa: F401  (the fixture)


def _fake_trainer(model):
    opt = model.configure_optimizers()["optimizer"]
    model._trainer = types.SimpleNamespace(optimizers=[opt], accumulate_grad_batches=1, gradient_clip_val=None,
                                           gradient_clip_algorithm=None, strategy=None)
    return opt


def _with_w_d(S, d_vd, **kw):
    """The (rebound) CLI's bond block with the reference's ``W_d`` of ``d_vd`` atom descriptors."""
    S.Bond.output_dim = property(lambda self: self.W_d.out_features if self.W_d is not None else self.W_o.out_features)
    mp = S.cli.BondMessagePassing(d_vd=d_vd, **kw)
    d_h = mp.W_o.out_features
    mp.W_d = torch.nn.Linear(d_h + d_vd, d_h + d_vd)
    return mp


def _model(S, d_vd, dev, seed=3):
    from chemprop_amd.model import RegressionFFN

    integ = S.integration
    integ.enable()
    HipM = integ.hip_mpnn_class()[1]
    torch.manual_seed(seed)
    mp = _with_w_d(S, d_vd)
    assert type(mp) is integ.hip_bond_message_passing_class() and mp.output_dim == 300 + d_vd
    a = HipM(mp, S.mods["chemprop.nn"].NormAggregation(), RegressionFFN(input_dim=mp.output_dim), batch_norm=True, init_lr=1e-3)
    return a.to(dev).train()


def _batch(n, d_vd, dev, seed=4):
    from chemprop_amd import synth

    bmg = synth.random_batch(n, "qm9", seed=seed)
    bmg.to(dev)
    gen = torch.Generator().manual_seed(seed + 2)
    y, w = torch.randn(n, 1, generator=gen).to(dev), (0.5 + torch.rand(n, 1, generator=gen)).to(dev)
    V = torch.randn(int(bmg.V.shape[0]), d_vd, generator=gen).to(dev)
    return bmg, y, w, V


@pytest.mark.gpu
@pytest.mark.parametrize("d_vd", [20, 50])
def test_hip_mpnn_training_step_with_atom_descriptors_equals_fused_trainer(stub_chemprop, d_vd, gpu_device):  # noqa: F811
    """``HipMPNN.training_step`` under the automatic-optimization closure takes a ``"fused:..."`` route for a batch with ``V_d`` and
    computes what ``FusedTrainer.step(..., V_d=V_d)`` computes on a copy of the model, over three steps (300 + 20 columns: the head's row
    form; 300 + 50: its chain)."""
    from chemprop_amd.model import FusedTrainer

    S = stub_chemprop
    a = _model(S, d_vd, gpu_device)
    b = copy.deepcopy(a)
    n = 96
    bmg, y, w, V = _batch(n, d_vd, gpu_device)
    opt = _fake_trainer(a)
    tr = FusedTrainer(b, lr=1e-3)
    for i in range(3):
        out = {}

        def closure(i=i):
            out["loss"] = a.training_step((bmg, V, None, y, w, None, None), i)
            return out["loss"]

        opt.step(closure)
        assert a.__dict__["_hip"]["route"].startswith("fused:"), a.__dict__["_hip"]
        lb = float(tr.step(bmg, y, w, V_d=V)[0])
        assert abs(float(out["loss"]) - lb) <= 1e-6 * max(1.0, abs(lb)), (i, float(out["loss"]), lb)
    torch.cuda.synchronize()
    for (k, pa), (_, pb) in zip(a.named_parameters(), b.named_parameters()):
        assert parity_err(pa.detach().cpu().numpy(), pb.detach().cpu().numpy()) <= 1e-6, k


@pytest.mark.gpu
def test_hip_mpnn_misshapen_atom_descriptors_raise(stub_chemprop, gpu_device):  # noqa: F811
    """A ``ValueError`` of the fused step (``V_d`` of the wrong width) propagates out of ``training_step``: it is a bug of the batch, not
    a batch for the module path."""
    S = stub_chemprop
    a = _model(S, 6, gpu_device)
    bmg, y, w, V = _batch(32, 6, gpu_device)
    _fake_trainer(a)
    with pytest.raises(ValueError, match="V_d must be"):
        a.training_step((bmg, V[:, :4], None, y, w, None, None), 0)


def test_hip_mpnn_takes_a_block_with_atom_descriptors_on_the_fused_step(stub_chemprop):  # noqa: F811
    """Host side only: ``FusedTrainer``'s block rule takes the HIP subclass of the reference's block with ``W_d`` — what ``HipMPNN``
    asks before it builds its trainer — and refuses it with dropout."""
    from chemprop_amd.model import fused_block

    S = stub_chemprop
    S.integration.enable()
    assert fused_block(_with_w_d(S, 7)) == fused_block(S.cli.BondMessagePassing())
    assert fused_block(_with_w_d(S, 7))[0] == "relu"
    with pytest.raises(NotImplementedError, match="dropout"):
        fused_block(_with_w_d(S, 7, dropout=0.1))
