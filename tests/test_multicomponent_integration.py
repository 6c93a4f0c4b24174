"""``integration.HipMulticomponentMPNN`` and ``enable()``'s rebinding of ``MulticomponentMPNN`` (``chemprop train --smiles-columns a b``).

The reference package is not importable here: a stand-in ``chemprop`` — the names ``enable()`` / ``accelerate()`` read, built on this
package's mirrors, with a minimal LightningModule face (``training_step``, ``configure_optimizers`` with a ``LambdaLR``, ``log``,
``backward``) — is installed in ``sys.modules`` for the duration of each test, with every class cache of ``integration`` reset."""
import copy
import sys
import types

import pytest
import torch

from conftest import parity_err


@pytest.fixture
def stub_chemprop(monkeypatch):
    from torch.optim.lr_scheduler import LambdaLR

    from chemprop_amd import agg as cagg
    from chemprop_amd import ffn as cffn
    from chemprop_amd import integration
    from chemprop_amd import model as cmodel
    from chemprop_amd import nn as cnn

    for name in ("_cls_cache", "_atom_cache", "_mab_cache", "_mlp_cache", "_mpnn_cache", "_agg_cache", "_multi_cache", "_enabled"):
        monkeypatch.setattr(integration, name, None)

    class BondMessagePassing(torch.nn.Module):   # (the reference's construction and names, base.py; the HIP subclass adds the engine's mixin)
        def __init__(self, d_v=72, d_e=14, d_h=300, bias=False, depth=3, dropout=0.0, activation="relu", undirected=False, d_vd=None):
            super().__init__()
            self.hparams = dict(d_v=d_v, d_e=d_e, d_h=d_h, bias=bias, depth=depth, dropout=dropout, activation=activation,
                                undirected=undirected, d_vd=d_vd, cls=type(self))
            self.W_i = torch.nn.Linear(d_v + d_e, d_h, bias)
            self.W_h = torch.nn.Linear(d_h, d_h, bias)
            self.W_o = torch.nn.Linear(d_v + d_h, d_h)
            self.W_d = None
            self.depth, self.undirected = depth, undirected
            self.dropout = torch.nn.Dropout(dropout)
            self.tau = cnn.get_activation_function(activation)
            self.V_d_transform = self.graph_transform = torch.nn.Identity()

        @property
        def output_dim(self):
            return self.W_o.out_features

    class AtomMessagePassing(cnn.AtomMessagePassing):
        pass

    class MLP(cffn.MLP):
        pass

    agg = types.ModuleType("chemprop.nn.agg")
    for n in ("MeanAggregation", "SumAggregation", "NormAggregation", "AttentiveAggregation"):
        base = getattr(cagg, n)

        def init(self, *a, _base=base, **k):
            _base.__init__(self, *a, **k)
            self.hparams = {"cls": type(self)}

        setattr(agg, n, type(n, (base,), {"__init__": init}))

    class MPNN(cmodel.MPNN):
        """The reference's LightningModule face, as far as HipMPNN uses it."""

        def __init__(self, message_passing, agg, predictor, batch_norm=False, metrics=None, warmup_epochs=2, init_lr=1e-4, max_lr=1e-3,
                     final_lr=1e-4, X_d_transform=None):
            super().__init__(message_passing, agg, predictor, batch_norm, X_d_transform)
            self.init_lr = init_lr
            self.automatic_optimization = True

        def training_step(self, batch, batch_idx):
            bmg, V_d, X_d, targets, weights, lt_mask, gt_mask = batch
            preds = self.predictor.train_step(self.fingerprint(bmg, V_d, X_d))
            return cmodel.masked_loss(preds, targets, weights, None, None, None, "mse")

        def configure_optimizers(self):
            opt = torch.optim.Adam(self.parameters(), self.init_lr)
            return {"optimizer": opt, "lr_scheduler": {"scheduler": LambdaLR(opt, lambda step: 1.0), "interval": "step"}}

        def log(self, *args, **kwargs):
            pass

        def backward(self, loss, *args, **kwargs):
            loss.backward()

        def configure_gradient_clipping(self, optimizer, gradient_clip_val=None, gradient_clip_algorithm=None):
            pass

        def on_train_start(self):
            pass

        @classmethod
        def load_from_file(cls, path):   # pragma: no cover
            raise NotImplementedError

    class MulticomponentMPNN(MPNN):
        fingerprint = cmodel.MulticomponentMPNN.fingerprint
        forward = cmodel.MulticomponentMPNN.forward

    mods = {n: types.ModuleType(n) for n in ("chemprop", "chemprop.nn", "chemprop.nn.ffn", "chemprop.models", "chemprop.models.model",
                                             "chemprop.models.multi")}
    mods["chemprop.nn.agg"] = agg
    nnm = mods["chemprop.nn"]
    nnm.BondMessagePassing, nnm.AtomMessagePassing, nnm.agg = BondMessagePassing, AtomMessagePassing, agg
    nnm.MulticomponentMessagePassing, nnm.NormAggregation = cnn.MulticomponentMessagePassing, agg.NormAggregation
    mods["chemprop.nn.ffn"].MLP = MLP
    mods["chemprop.models.model"].MPNN = MPNN
    mods["chemprop.models.multi"].MulticomponentMPNN = MulticomponentMPNN
    mods["chemprop.models"].MPNN, mods["chemprop.models"].MulticomponentMPNN = MPNN, MulticomponentMPNN
    cli = types.ModuleType("chemprop.cli.train")   # (what cli/train.py binds at import)
    cli.MPNN, cli.MulticomponentMPNN, cli.BondMessagePassing = MPNN, MulticomponentMPNN, BondMessagePassing
    mods["chemprop.cli.train"] = cli
    mods["chemprop"].nn, mods["chemprop"].models = nnm, mods["chemprop.models"]
    for n, m in mods.items():
        monkeypatch.setitem(sys.modules, n, m)
    return types.SimpleNamespace(mods=mods, cli=cli, MPNN=MPNN, Multi=MulticomponentMPNN, Bond=BondMessagePassing, integration=integration)


def test_enable_rebinds_multicomponent_mpnn(stub_chemprop):
    """``enable()`` rebinds ``MulticomponentMPNN`` wherever it is bound by name (the CLI, ``chemprop.models``, ``chemprop.models.multi``)
    to ``HipMulticomponentMPNN``: a subclass of the reference class AND of ``HipMPNN``, whose step, optimizer and hooks are
    ``HipMPNN``'s own functions (not copies); the model the CLI builds by those names has its blocks on the HIP class."""
    S = stub_chemprop
    integ = S.integration
    done = integ.enable()
    RefMC, HipMC = integ.hip_multicomponent_mpnn_class()
    HipM = integ.hip_mpnn_class()[1]
    assert RefMC is S.Multi and "MulticomponentMPNN" in done["chemprop.cli.train"]
    assert S.cli.MulticomponentMPNN is HipMC and S.mods["chemprop.models"].MulticomponentMPNN is HipMC
    assert S.mods["chemprop.models.multi"].MulticomponentMPNN is HipMC and S.cli.MPNN is HipM
    assert issubclass(HipMC, S.Multi) and issubclass(HipMC, HipM) and integ.HipMulticomponentMPNN is HipMC
    for name in ("training_step", "configure_optimizers", "backward", "configure_gradient_clipping", "_hip_state"):
        assert getattr(HipMC, name) is getattr(HipM, name), name
    assert HipMC.fingerprint is S.Multi.fingerprint
    from chemprop_amd.model import RegressionFFN

    torch.manual_seed(0)
    blocks = [S.cli.BondMessagePassing(d_h=16), S.cli.BondMessagePassing(106, 28, d_h=16)]
    mp = S.mods["chemprop.nn"].MulticomponentMessagePassing(blocks, 2)
    m = S.cli.MulticomponentMPNN(mp, S.mods["chemprop.nn"].NormAggregation(), RegressionFFN(input_dim=32, hidden_dim=8), batch_norm=True)
    assert all(type(b) is integ.hip_bond_message_passing_class() for b in m.message_passing.blocks)
    assert integ.enable() is not None and integ.enabled()   # idempotent


def _fake_trainer(model):
    opt = model.configure_optimizers()["optimizer"]
    model._trainer = types.SimpleNamespace(optimizers=[opt], accumulate_grad_batches=1, gradient_clip_val=None,
                                           gradient_clip_algorithm=None, strategy=None)
    return opt


@pytest.mark.gpu
@pytest.mark.parametrize("shared", [False, True])
def test_hip_multicomponent_training_step_equals_fused_trainer(stub_chemprop, shared, gpu_device):
    """``HipMulticomponentMPNN.training_step`` under the automatic-optimization closure (``optimizer.step(closure)``) takes the one-call
    step with ``V_ds = [None, None]`` and computes what ``FusedTrainer.step`` computes on a copy of the model, over three steps."""
    from chemprop_amd import synth
    from chemprop_amd.model import FusedTrainer, RegressionFFN

    S = stub_chemprop
    integ = S.integration
    integ.enable()
    HipMC = integ.hip_multicomponent_mpnn_class()[1]
    torch.manual_seed(3)
    blocks = [S.cli.BondMessagePassing()] if shared else [S.cli.BondMessagePassing(106, 28), S.cli.BondMessagePassing()]
    mp = S.mods["chemprop.nn"].MulticomponentMessagePassing(blocks, 2, shared=shared)
    a = HipMC(mp, S.mods["chemprop.nn"].NormAggregation(), RegressionFFN(input_dim=mp.output_dim), batch_norm=True, init_lr=1e-3)
    a = a.to(gpu_device).train()
    b = copy.deepcopy(a)
    n = 96
    bmgs = [synth.random_batch(n, "qm9" if shared else "cgr", seed=4), synth.random_batch(n, "qm9", seed=5)]
    for x in bmgs:
        x.to(gpu_device)
    gen = torch.Generator().manual_seed(6)
    y, w = torch.randn(n, 1, generator=gen).to(gpu_device), (0.5 + torch.rand(n, 1, generator=gen)).to(gpu_device)
    opt = _fake_trainer(a)
    tr = FusedTrainer(b, lr=1e-3)
    for i in range(3):
        out = {}

        def closure(i=i):
            out["loss"] = a.training_step((bmgs, [None, None], None, y, w, None, None), i)
            return out["loss"]

        opt.step(closure)
        assert a.__dict__["_hip"]["route"].startswith("fused"), a.__dict__["_hip"]
        lb = float(tr.step(bmgs, y, w)[0])
        assert abs(float(out["loss"]) - lb) <= 1e-6 * max(1.0, abs(lb)), (i, float(out["loss"]), lb)
    torch.cuda.synchronize()
    for (k, pa), (_, pb) in zip(a.named_parameters(), b.named_parameters()):
        assert parity_err(pa.detach().cpu().numpy(), pb.detach().cpu().numpy()) <= 1e-6, k
