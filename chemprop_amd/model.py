"""f4: the model around the block — ``chemprop.models.MPNN`` (``models/model.py:60-161``) with a regression
predictor (``nn/predictors.py:101-169``) — and its training step as ONE C call.

:class:`MPNN` mirrors the reference's attribute names (``message_passing``, ``agg``, ``bn``, ``predictor``; ``predictor.ffn``,
``predictor.criterion.task_weights``), so a state dict moves between the two for those keys, and its ``forward`` /
``fingerprint`` / ``loss`` run on the engine's kernels through autograd like any torch module (the drop-in path).

:class:`FusedTrainer` is the MI355X-native form of ``training_step`` + ``optimizer.step()`` (``model.py:148-161,208-231``):
every parameter lives in ONE flat buffer, every gradient in another (``distributed.GradSync`` / ``optim.FlatAdam``), and a
step is ``dmpnn_train_step`` — K0, the block's forward with kept tensors, aggregation, batch norm, the predictor's layers, the
loss and its gradient, the backward pass of all of it and the Adam update are enqueued by one call (``csrc/dmpnn_head.hip``);
nothing of the step runs in Python or in ATen.  With more than one rank the gradient all-reduce sits between the backward pass
and the update (the step is then two calls around ``GradSync.allreduce``).
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Iterable, Optional

import torch
from torch import Tensor, nn

from . import _lib, engine
from .agg import MODES, Aggregation, NormAggregation, note_batch
from .distributed import GradSync, force_collective
from .ffn import mlp_blocks
from .heads import (BCE, CE, CRITERIA, CRITERION, MAE, MSE, MVE, NOT_BUILT_IN, ONE_VALUE_PER_TASK, SID, UNKNOWN_CRITERION,  # noqa: F401
                    BinaryClassificationFFN, BinaryDirichletFFN, BinaryMCC, Dirichlet, Evidential, EvidentialFFN, MulticlassClassificationFFN,
                    MulticlassDirichletFFN, MveFFN, Quantile, QuantileFFN, RegressionFFN, SpectralFFN, Wasserstein, _mro_names,
                    criterion_bounded, criterion_kind, criterion_loss, masked_loss, predictor_row, spectral_activation_of)
from .nn import BondMessagePassing, MulticomponentMessagePassing, classify_activation
from .data import merge_components
from .optim import CLIP_MODES, FlatAdam, bias_corrections

__all__ = ["MSE", "MAE", "BCE", "CE", "MVE", "Evidential", "Quantile", "RegressionFFN", "BinaryClassificationFFN", "MulticlassClassificationFFN", "MveFFN", "EvidentialFFN", "QuantileFFN",
           "Dirichlet", "BinaryDirichletFFN", "MulticlassDirichletFFN", "SID", "Wasserstein", "SpectralFFN", "BinaryMCC", "MPNN", "MulticomponentMPNN", "FusedTrainer", "masked_loss"]


class MPNN(nn.Module):
    """``chemprop.models.MPNN`` (``models/model.py:60-146``) without Lightning: the four sub-modules under the reference's
    names and ``fingerprint`` / ``forward``; ``loss(batch)`` is the arithmetic of ``training_step`` (``model.py:148-161``).

    Molecule descriptors ``X_d`` (``--molecule-featurizers`` / ``--descriptors-path``) are concatenated behind the batch norm,
    through ``X_d_transform`` (the reference's ``ScaleTransform`` or ``nn.Identity``): the predictor's ``input_dim`` is then
    ``message_passing.output_dim + d_xd``."""

    def __init__(self, message_passing: nn.Module, agg: nn.Module, predictor: nn.Module, batch_norm: bool = False,
                 X_d_transform: Optional[nn.Module] = None):
        super().__init__()
        if predictor.input_dim < message_passing.output_dim:
            raise ValueError(f"predictor input dim {predictor.input_dim} < message passing output dim {message_passing.output_dim}")
        self.message_passing = message_passing
        self.agg = agg
        self.bn = nn.BatchNorm1d(message_passing.output_dim) if batch_norm else nn.Identity()
        self.predictor = predictor
        self.X_d_transform = X_d_transform if X_d_transform is not None else nn.Identity()

    @property
    def criterion(self):
        return self.predictor.criterion

    def fingerprint(self, bmg, V_d: Optional[Tensor] = None, X_d: Optional[Tensor] = None) -> Tensor:
        H = self.bn(self.agg(self.message_passing(bmg, V_d), bmg.batch))
        return H if X_d is None else torch.cat((H, self.X_d_transform(X_d)), dim=1)

    def forward(self, bmg, V_d: Optional[Tensor] = None, X_d: Optional[Tensor] = None) -> Tensor:
        return self.predictor(self.fingerprint(bmg, V_d, X_d))

    def loss(self, bmg, targets: Tensor, weights: Optional[Tensor] = None, lt_mask: Optional[Tensor] = None,
             gt_mask: Optional[Tensor] = None, V_d: Optional[Tensor] = None, X_d: Optional[Tensor] = None) -> Tensor:
        if torch.is_grad_enabled() and self.training:
            # the module path of a training step: the block through its own autograd node, everything behind it — aggregation, batch
            # norm, the descriptors' concatenation, predictor, criterion AND their backward pass — as ONE more (head_loss); None: the
            # head kernels do not take this model or these inputs
            l = head_loss(self, self.message_passing(bmg, V_d), bmg.batch, len(bmg), targets, weights, lt_mask, gt_mask,
                          X_d=None if X_d is None else self.X_d_transform(X_d))
            if l is not None:
                return l
        return self._torch_loss(self.fingerprint(bmg, V_d, X_d), targets, weights, lt_mask, gt_mask)

    def _torch_loss(self, Z: Tensor, targets: Tensor, weights, lt_mask, gt_mask) -> Tensor:
        """The tail of ``loss`` on torch ops: the criterion on ``predictor.train_step`` of the fingerprint ``Z``."""
        return criterion_loss(self.criterion, self.predictor.train_step(Z), targets, weights, lt_mask, gt_mask)

    def predict(self, bmg, V_d: Optional[Tensor] = None, X_d: Optional[Tensor] = None) -> Tensor:
        """``self(bmg, V_d, X_d)`` without autograd; in eval mode everything behind the block is ONE C call
        (:func:`chemprop_amd.predict.fused_predict`) where the inference head takes this model and these inputs."""
        from .predict import fused_predict

        with torch.no_grad():
            r = fused_predict(self, bmg, V_d, X_d)
            return self(bmg, V_d, X_d) if r is None else r.preds

    def validate(self, bmg, targets: Tensor, stats, V_d: Optional[Tensor] = None, X_d: Optional[Tensor] = None, *,
                 metric_targets: Optional[Tensor] = None, weights: Optional[Tensor] = None, lt_mask: Optional[Tensor] = None,
                 gt_mask: Optional[Tensor] = None, fingerprint: bool = False, ranks=None):
        """One validation step without autograd: the predictions, the criterion on the raw outputs (``val_loss``) and the batch's
        metric sums added into ``stats`` (a :class:`~chemprop_amd.metrics.MetricStats`: :meth:`MetricStats.for_model`).  In eval mode
        everything behind the block is ONE C call (:func:`chemprop_amd.predict.fused_validate`) where the inference head takes this
        model and these inputs; otherwise the fingerprint is formed once, ``preds = predictor(Z)``, the loss is the criterion on
        ``predictor.train_step(Z)`` and ``stats.update`` adds the sums.  ``metric_targets``: what the metrics compare the predictions
        with where that is not ``targets`` (unscaled against scaled).  The bounds reach the statistics where they reach the criterion
        (:func:`~chemprop_amd.heads.criterion_bounded`).  ``ranks`` (a :class:`~chemprop_amd.metrics.RankStats`, binary heads): the batch's
        (score, label) rows are appended to the epoch's rank buffer for ROC-AUC / PRC-AUC — one launch more inside the same C call, or
        ``ranks.update`` on the module path.  Returns a :class:`~chemprop_amd.predict.PredictResult` (on the module path ``raw`` is
        ``train_step``'s tensor as the predictor shapes it)."""
        from .predict import PredictResult, fused_validate

        with torch.no_grad():
            r = fused_validate(self, bmg, V_d, X_d, targets=targets, stats=stats, metric_targets=metric_targets, weights=weights,
                               lt_mask=lt_mask, gt_mask=gt_mask, fingerprint=fingerprint, ranks=ranks)
            if r is not None:
                return r
            Z = self.fingerprint(bmg, V_d, X_d)
            preds, raw = self.predictor(Z), self.predictor.train_step(Z)
            l = criterion_loss(self.criterion, raw, targets, weights, lt_mask, gt_mask)
            loss = torch.stack((l.float(), targets.isfinite().sum().float()))
            bounded = criterion_bounded(self.criterion)
            stats.update(preds, targets if metric_targets is None else metric_targets, lt_mask if bounded else None,
                         gt_mask if bounded else None, loss=loss)
            if ranks is not None:
                ranks.update(preds, targets if metric_targets is None else metric_targets)
            return PredictResult(preds, raw, Z if fingerprint else None, loss)


class MulticomponentMPNN(MPNN):
    """``chemprop.models.MulticomponentMPNN`` (``models/multi.py``): a :class:`~chemprop_amd.nn.MulticomponentMessagePassing` block,
    the fingerprint ``cat([agg(H_v^c, bmg^c.batch) for c], 1)`` through the batch norm (``BatchNorm1d(sum of the blocks' widths)``),
    then the descriptors.  ``fingerprint`` / ``forward`` / ``loss`` take a list of batches and a list of ``V_d`` (or ``None``); row
    ``i`` of every component belongs to target row ``i``."""

    def fingerprint(self, bmgs, V_ds=None, X_d: Optional[Tensor] = None) -> Tensor:
        H_vs = self.message_passing(bmgs, V_ds)
        H = self.bn(torch.cat([self.agg(H_v, bmg.batch) for H_v, bmg in zip(H_vs, bmgs)], 1))
        return H if X_d is None else torch.cat((H, self.X_d_transform(X_d)), dim=1)

    def forward(self, bmgs, V_ds=None, X_d: Optional[Tensor] = None) -> Tensor:
        return self.predictor(self.fingerprint(bmgs, V_ds, X_d))

    def loss(self, bmgs, targets: Tensor, weights: Optional[Tensor] = None, lt_mask: Optional[Tensor] = None,
             gt_mask: Optional[Tensor] = None, V_ds=None, X_d: Optional[Tensor] = None) -> Tensor:
        if torch.is_grad_enabled() and self.training:
            # the module path: every block through its own autograd node, everything behind them as ONE more (head_loss on the
            # blocks' outputs side by side)
            B = len(bmgs[0])
            if all(len(b) == B for b in bmgs):
                l = head_loss(self, self.message_passing(bmgs, V_ds), [b.batch for b in bmgs], B, targets, weights, lt_mask, gt_mask,
                              X_d=None if X_d is None else self.X_d_transform(X_d))
                if l is not None:
                    return l
        return self._torch_loss(self.fingerprint(bmgs, V_ds, X_d), targets, weights, lt_mask, gt_mask)

    def predict(self, bmgs, V_ds=None, X_d: Optional[Tensor] = None) -> Tensor:
        """:meth:`MPNN.predict` on the components' batches: ``self(bmgs, V_ds, X_d)`` without autograd."""
        return super().predict(bmgs, V_ds, X_d)


def is_atom_block(mp) -> bool:
    """An ``AtomMessagePassing`` block by its parameter shapes (base.py:278-289): ``W_i [d_h, d_v]``, ``W_h [d_h, d_h + d_e]``."""
    if not all(isinstance(getattr(mp, n, None), nn.Linear) for n in ("W_i", "W_h", "W_o")):
        return False
    d_h = mp.W_h.out_features
    return mp.W_h.in_features > d_h and mp.W_o.in_features > d_h and mp.W_i.in_features == mp.W_o.in_features - d_h


def fused_block(mp, rows_dropout: bool = False, vd_dropout: bool = False, atom_messages: bool = False, undirected: bool = False) -> tuple:
    """``(activation, slope)`` of a block the one-call step takes: a bond block (this package's mirror, or the subclass of the
    reference's own class, ``integration.HipBondMessagePassing``) with a built-in activation (not PReLU), directed, dropout 0
    or ``nn.Dropout`` with a ReLU-class activation — with ``rows_dropout=True`` (the mask in the row kernels of the per-step general
    route, ``engine.rows_dropout_refusal``) with any built-in activation; ``NotImplementedError`` for anything else (it trains
    through the module path).
    A block built with ``d_vd > 0`` is taken — its layer ``W_d`` runs as a stage of its own behind the block (``dmpnn_vd_forward`` /
    ``dmpnn_vd_backward``) — unless ``d_h + d_vd`` is beyond ``_lib.VD_MAX_WIDTH`` or it also has dropout: the reference applies the
    block's dropout a second time behind ``W_d``, and only ``vd_dropout=True`` asks for that fourth mask (site ``_lib.DROP_SITE_VD``
    inside the stage's kernels, ``dmpnn_vd_args.dropout_p``).  The block is then taken under exactly the conditions it would meet
    without ``W_d`` (``nn.Dropout``; a ReLU-class activation, or ``rows_dropout=True`` and a built-in smooth one).
    ``atom_messages=True`` also takes an atom block (``W_i [d_h, d_v]``, ``W_h [d_h, d_h + d_e]``: :func:`is_atom_block`) that is
    directed, has a built-in activation other than PReLU, no ``W_d``, ``1 <= d_e <= 16`` and dropout 0 — or ``nn.Dropout`` with
    ``rows_dropout=True`` (its only home is the row kernels: the atom tile kernels carry no mask).  The default refuses it.
    ``undirected=True`` also takes a bond block with ``mp.undirected`` (base.py:202-203), under exactly the conditions a directed one
    meets — except that with ``p > 0`` its only dropout home is the row kernels (``DMPNN_F_UNDIRECTED_MASK``): ``nn.Dropout`` and
    ``rows_dropout=True`` (and ``vd_dropout=True`` beside ``W_d``, as for a directed block).  An undirected ATOM block stays refused.
    The default refuses an undirected block."""
    # (W_h is [d_h, d_h] in a bond block: the atom variant's takes d_e + d_h columns, the mol-atom-bond ones have a second read-out)
    bond = (all(isinstance(getattr(mp, n, None), nn.Linear) for n in ("W_i", "W_h", "W_o"))
            and mp.W_h.in_features == mp.W_h.out_features and mp.W_o.in_features > mp.W_h.out_features)
    atom = not bond and bool(atom_messages) and is_atom_block(mp)
    if not bond and not atom:
        raise NotImplementedError("FusedTrainer: a BondMessagePassing block (W_i / W_h [d_h, d_h] / W_o)"
                                  + (" — atom_messages=True also takes an AtomMessagePassing block" if is_atom_block(mp) else ""))
    act, slope, slope_t = classify_activation(mp.tau)
    if act in ("custom", "prelu") or (mp.undirected and not (undirected and bond)):
        raise NotImplementedError("FusedTrainer: built-in activation (not PReLU), directed — other blocks train "
                                  "through the module path (MPNN.loss + autograd)"
                                  + (" (undirected=True also takes an undirected bond block)" if mp.undirected and bond and not undirected else ""))
    if atom:
        d_e = mp.W_h.in_features - mp.W_h.out_features
        if mp.W_d is not None:
            raise NotImplementedError("FusedTrainer: an atom block with atom descriptors (W_d) trains through the module path")
        if not 1 <= d_e <= 16:
            raise NotImplementedError(f"FusedTrainer: an atom block with d_e = {d_e} (the kernels keep the bond-feature half of the "
                                      "messages as rows of 16 columns: 1 <= d_e <= 16)")
        if mp.dropout.p > 0 and not (type(mp.dropout) is nn.Dropout and rows_dropout):
            raise NotImplementedError("FusedTrainer: dropout inside an atom block needs nn.Dropout and rows_dropout=True (the mask lives "
                                      "in the row kernels; the atom tile kernels carry none)")
        return act, slope
    if mp.W_d is not None:
        if mp.dropout.p > 0 and not vd_dropout:
            raise NotImplementedError("FusedTrainer: atom descriptors (W_d) together with dropout inside the block — the dropout behind "
                                      "W_d has no mask site; this model trains through the module path (vd_dropout=True masks inside "
                                      "the atom-descriptor stage)")
        if not (isinstance(mp.W_d, nn.Linear) and mp.W_d.in_features == mp.W_d.out_features and mp.W_d.bias is not None
                and mp.W_d.in_features > mp.W_o.out_features):
            raise NotImplementedError("FusedTrainer: W_d must be a square nn.Linear with a bias over cat(H_v, V_d)")
        if mp.W_d.in_features > _lib.VD_MAX_WIDTH:
            raise NotImplementedError(f"FusedTrainer: d_h + d_vd = {mp.W_d.in_features} is beyond the {_lib.VD_MAX_WIDTH} columns the "
                                      "atom-descriptor stage takes")
    if mp.undirected and mp.dropout.p > 0 and not (type(mp.dropout) is nn.Dropout and rows_dropout):
        raise NotImplementedError("FusedTrainer: dropout inside an undirected block needs nn.Dropout and rows_dropout=True (the mask lives "
                                  "in the row kernels; the tile kernels and the lean step kernels are directed)")
    if mp.dropout.p > 0 and not (type(mp.dropout) is nn.Dropout and (rows_dropout or act in ("relu", "leakyrelu"))):
        # (active dropout lives inside the tile kernels and the lean step kernels, for ReLU-class activations, and — rows_dropout — in the
        #  row kernels of the per-step general route for every built-in one: dmpnn_fwd_args.dropout_p; a dropout module that is not
        #  exactly nn.Dropout has its own semantics and stays on the module path)
        raise NotImplementedError("FusedTrainer: dropout inside the block needs nn.Dropout and a ReLU / LeakyReLU activation"
                                  + ("" if rows_dropout else " (rows_dropout=True also takes tanh / elu / selu, on the row kernels)"))
    return act, slope


def aggregation_mode(agg) -> Optional[str]:
    """``"sum" | "mean" | "norm"`` for this package's aggregations (``.mode``) and for the reference's own classes / their HIP
    subclasses (``chemprop/nn/agg.py:66-113``, told by class name); ``None`` for anything else (attentive, custom)."""
    mode = getattr(agg, "mode", None)
    if mode in MODES:
        return mode
    names = _mro_names(agg)
    for cls, m in (("NormAggregation", "norm"), ("MeanAggregation", "mean"), ("SumAggregation", "sum")):  # (Norm derives from Sum)
        if cls in names:
            return m
    return None


def _batch_vector_ok(batch: Optional[Tensor], n_atoms: int, dev) -> bool:
    """The head kernels read ``batch`` through a raw pointer: a wrong dtype / size would be an out-of-bounds device read, not an error."""
    return batch is not None and batch.dtype == torch.int64 and batch.is_contiguous() and batch.device == dev and batch.numel() == n_atoms


def _component_batch(batches: list, n_mols: int) -> Tensor:
    """ONE batch vector over every component's rows: molecule ``i`` of component ``c`` is ``c n_mols + i`` (torch ops)."""
    return torch.cat([b + c * n_mols for c, b in enumerate(batches)]) if len(batches) > 1 else batches[0]


class HeadSpec:
    """What ``dmpnn_head`` needs to know of the model around the block — aggregation, batch norm, the predictor's layers and
    activation, the criterion — taken once from the modules; raises ``NotImplementedError`` for what the head kernels do not
    implement.  Shared by :class:`FusedTrainer` (the whole step as one C call) and :func:`head_loss` (the module path's ONE
    autograd node for everything behind the block).

    ``d_xd`` is the width of the molecule descriptors the model expects: the first layer's ``in_features`` less the block's output
    width (0: none).  ``fill(..., X_d=...)`` hands them over as ``dmpnn_head_args.X_d`` / ``ld_xd`` with ``dims[0] = d_h + d_xd``.

    ``ffn_dropout=True``: the predictor's dropout may be active — ONE ``nn.Dropout`` shared by its blocks (``MLP.build``), kept as
    ``drop``; ``fill(..., ffn_dropout=(p, seed))`` hands it to the kernels as their hash mask (``dmpnn_head_args.ffn_dropout_p``).
    Without it a predictor with dropout is refused (the module path keeps torch's ``nn.Dropout``).

    ``attentive=True`` also takes ``AttentiveAggregation`` (this package's mirror, the reference's class or a subclass of it,
    ``nn/agg.py:116-133``) when its ``W`` is an ``nn.Linear(d_h, 1)`` with a bias over the head's input width and the model has one
    component: ``dmpnn_head_args.agg_mode = DMPNN_MOLAGG_ATTENTIVE`` with ``att_W`` / ``att_b``; ``att`` is that layer (``None``
    otherwise).  The default refuses it like any aggregation that is not sum / mean / norm.

    Which predictor meets which criterion is the tables' word (``heads.CRITERIA`` / ``PREDICTORS``, the reference's classes by MRO name).
    A Dirichlet head: ``n_classes`` the predictor's (2 for the binary one), ``v_kl`` handed over as ``evid_v_kl``.  A spectral head:
    ``spectral_act`` (``"softplus" | "exp"``, off ``ffn.spectral_activation``, which is not one of ``layers``) and ``spectral_threshold``
    (the criterion's ``threshold``, 0.0 for ``None``) travel in ``dmpnn_head_args``."""

    def __init__(self, model, ffn_dropout: bool = False, attentive: bool = False):
        agg, pred = model.agg, model.predictor
        mode = aggregation_mode(agg)
        self.att = None
        if mode is None and attentive and (getattr(agg, "mode", None) == "attentive" or "AttentiveAggregation" in _mro_names(agg)):
            mp_ = model.message_passing
            if isinstance(getattr(mp_, "blocks", None), nn.ModuleList) and hasattr(mp_, "n_components"):
                raise NotImplementedError("attentive aggregation in a multicomponent model (dmpnn_head takes it with one component)")
            W, width = getattr(agg, "W", None), int(getattr(mp_, "output_dim", 0))
            if not isinstance(W, nn.Linear) or W.out_features != 1 or W.in_features != width:
                raise NotImplementedError(f"attentive aggregation: W must be an nn.Linear({width}, 1) over the block's output "
                                          f"(got {W!r})")
            if W.bias is None:
                raise NotImplementedError("attentive aggregation: W must be an nn.Linear with a bias (the kernels read att_b)")
            self.att = W
        elif mode is None:
            raise NotImplementedError(f"sum / mean / norm aggregation (got {type(agg).__name__})")
        blocks = mlp_blocks(pred.ffn)   # (a SpectralFFN's spectral_activation child is not a layer)
        if len(blocks) > _lib.MAX_FFN_LAYERS:
            raise NotImplementedError(f"at most {_lib.MAX_FFN_LAYERS} predictor layers")
        f_act, f_slope = "none", 0.0
        for b in blocks[1:]:
            code, sl, _ = classify_activation(b[0])
            if code in ("custom", "prelu") or (b[1].p > 0 and not ffn_dropout):
                raise NotImplementedError("predictor with a built-in activation (not PReLU) and dropout 0")
            f_act, f_slope = code, sl
        # the predictor's dropout on the kernels: the hash mask has one p for every layer — chemprop's MLP shares one module
        self.drop = None
        drops = list({id(b[1]): b[1] for b in blocks[1:]}.values())
        if ffn_dropout and drops:
            if len(drops) == 1 and type(drops[0]) is nn.Dropout and 0 <= drops[0].p < 1:
                self.drop = drops[0]
            elif any(d.p > 0 for d in drops):
                raise NotImplementedError("predictor dropout: one nn.Dropout with 0 < p < 1 shared by the predictor's blocks")
        # (the reference's UnscaleTransform IS the identity in training mode, transforms.py:45-50: what a scaled regression run carries)
        if not (isinstance(pred.output_transform, nn.Identity) or "UnscaleTransform" in _mro_names(pred.output_transform)):
            raise NotImplementedError("the output transform is the identity while training (predictors.py:166-169)")
        kind, self.bounded = criterion_kind(pred.criterion)   # (the criterion's row and the predictor's, held against each other)
        if kind is None:
            raise NotImplementedError(next((why for n, why in NOT_BUILT_IN.items() if n in _mro_names(pred.criterion)), UNKNOWN_CRITERION))
        crit, row = CRITERION[kind], predictor_row(pred)
        name, fmt = getattr(row, "name", None), dict(kind=kind, cls=type(pred).__name__)
        for c in CRITERIA:   # predictors that take one criterion alone: a Dirichlet head, then (table order) a SpectralFFN
            if c.alone and (crit.predictors == c.predictors) != (name in c.predictors):
                raise NotImplementedError((c.alone if name in c.predictors else crit.refusal).format(**fmt))
        self.spectral_act, self.spectral_threshold = None, 0.0
        if row is not None and row.transform == "spectral":
            self.spectral_act = spectral_activation_of(pred)
            if self.spectral_act is None:
                raise NotImplementedError(f"a SpectralFFN whose spectral_activation is softplus or exp (got {getattr(pred.ffn, 'spectral_activation', None)!r})")
            thr = getattr(pred.criterion, "threshold", None)
            self.spectral_threshold = 0.0 if thr is None else float(thr)
            if not (math.isfinite(self.spectral_threshold) and self.spectral_threshold >= 0):
                raise NotImplementedError(f"a spectral criterion's threshold is None or a finite number >= 0 (got {thr!r})")
        # a criterion with predictors of its own (binary MCC, MVE / evidential / quantile); the binary Dirichlet head's two values are classes
        if crit.predictors is not None and name not in crit.predictors:
            raise NotImplementedError(crit.refusal.format(**fmt))
        two_classes = row is not None and row.classes == 2
        self.n_targets = 1 if two_classes else int(getattr(pred, "n_targets", 1))
        if self.n_targets != crit.values:
            raise NotImplementedError(ONE_VALUE_PER_TASK)
        if crit.values > 1 and int(blocks[-1][-1].out_features) % crit.values:
            raise NotImplementedError("the output width must be n_tasks * n_targets")
        self.v_kl, self.eps, self.q_alpha = (float(getattr(pred.criterion, n, d)) for n, d in (("v_kl", 0.2), ("eps", 1e-8), ("alpha", 0.1)))
        self.n_classes = 2 if two_classes else int(getattr(pred, "n_classes", 0) or 0)
        if crit.classes != (self.n_classes >= 2):
            raise NotImplementedError("a multiclass predictor (n_classes >= 2) with CrossEntropyLoss or DirichletLoss, or neither")
        if crit.classes and int(blocks[-1][-1].out_features) % self.n_classes:
            raise NotImplementedError("the output width must be n_tasks * n_classes")
        self.agg_mode, self.agg_norm = (_lib.MOLAGG_ATTENTIVE if self.att is not None else MODES[mode]), float(getattr(agg, "norm", 1.0))
        self.f_act, self.f_slope, self.kind = f_act, f_slope, kind
        self.layers = [b[-1] for b in blocks]
        # a multicomponent model (models/multi.py): the fingerprint is the components' aggregates side by side, ONE width per block
        self.n_components, self.blocks = 1, None
        mp = model.message_passing
        if isinstance(getattr(mp, "blocks", None), nn.ModuleList) and hasattr(mp, "n_components"):
            comp = list(mp.blocks)
            for b in comp:
                fused_block(b)
            if len({int(b.output_dim) for b in comp}) != 1:
                raise NotImplementedError("multicomponent blocks of one output width d_h")
            if len(comp) > _lib.MAX_COMPONENTS:
                raise NotImplementedError(f"at most {_lib.MAX_COMPONENTS} components")
            self.n_components, self.blocks = len(comp), comp
        k0 = int(self.layers[0].in_features)
        self.d_xd = k0 - int(getattr(model.message_passing, "output_dim", k0))
        if self.d_xd < 0:
            raise NotImplementedError("a predictor at least as wide as the block's output")
        self.bn = model.bn if isinstance(model.bn, nn.BatchNorm1d) else None
        if self.bn is not None and (self.bn.momentum is None or not self.bn.affine or not self.bn.track_running_stats):
            raise NotImplementedError("nn.BatchNorm1d with a fixed momentum, affine, running statistics")
        self.criterion = pred.criterion

    @property
    def n_out(self) -> int:
        """Width of the output layer (= columns of the predictions the kernels write)."""
        return int(self.layers[-1].out_features)

    @property
    def n_tasks(self) -> int:
        """Columns of ``targets``: the output width, or — multiclass — that over ``n_classes``."""
        return self.n_out // self.n_classes if self.n_classes >= 2 else self.n_out // self.n_targets

    def params(self) -> list:
        """The head's parameters in the order ``fill`` asks ``gptr`` about them."""
        ps = [] if self.att is None else [self.att.weight, self.att.bias]   # (model.parameters() order: agg, bn, predictor)
        if self.bn is not None:
            ps += [self.bn.weight, self.bn.bias]
        for lin in self.layers:
            ps.append(lin.weight)
            if lin.bias is not None:
                ps.append(lin.bias)
        return ps

    def descriptors(self, X_d: Optional[Tensor], n_mols: int, dev) -> Optional[Tensor]:
        """``X_d`` (already through ``X_d_transform``) as fp32 rows on ``dev`` with unit column stride — what ``fill`` hands to the
        kernels; ``ValueError`` when the model expects descriptors and gets none, gets descriptors it has no columns for, or the
        shape is not ``[n_mols, d_xd]``."""
        if X_d is None:
            if self.d_xd:
                raise ValueError(f"this model's predictor expects {self.d_xd} molecule descriptors per molecule (X_d), got none")
            return None
        if not self.d_xd:
            raise ValueError("X_d given, but this model's predictor takes no molecule descriptors")
        if X_d.dim() != 2 or tuple(X_d.shape) != (n_mols, self.d_xd):
            raise ValueError(f"X_d must be [{n_mols}, {self.d_xd}], got {tuple(X_d.shape)}")
        if X_d.device != dev:
            raise ValueError(f"X_d must live on {dev}, got {X_d.device}")
        X = X_d.detach()
        if X.dtype != torch.float32 or X.stride(1) != 1 or X.stride(0) < self.d_xd:
            X = X.float().contiguous()
        return X

    def fill(self, h, nV: int, n_mols: int, d_out: int, batch: Tensor, T: Tensor, weights, lt_mask, gt_mask, gptr, bn_training: bool = True,
             X_d: Optional[Tensor] = None, ffn_dropout: Optional[tuple] = None) -> list:
        """Fill ``h`` (a ``_lib.HeadArgs``) but for ``preds / loss_out / gHv / ws``; ``gptr(param)`` gives the address the gradient of
        ``param`` goes to (``None``: not wanted).  ``X_d``: the molecule descriptors as :meth:`descriptors` returns them.
        ``ffn_dropout``: ``(p, seed)`` of the predictor's dropout mask, or ``None`` (no dropout).  Returns the tensors that must stay
        alive until the call has been enqueued."""
        dev = T.device
        h.n_atoms, h.n_mols, h.d_h = nV, n_mols, d_out
        if ffn_dropout is not None:
            h.ffn_dropout_p, h.ffn_dropout_seed = float(ffn_dropout[0]), int(ffn_dropout[1])
        if self.n_components > 1:   # (d_out: one block's width; `batch` numbers molecule i of component c as c n_mols + i)
            h.n_components = self.n_components
        h.batch = batch.data_ptr()
        h.agg_mode, h.agg_norm = self.agg_mode, self.agg_norm
        if self.att is not None:
            h.att_W, h.att_b = self.att.weight.data_ptr(), self.att.bias.data_ptr()
            h.g_att_W, h.g_att_b = gptr(self.att.weight), gptr(self.att.bias)
        bn = self.bn
        if bn is not None:
            h.bn_weight, h.bn_bias = bn.weight.data_ptr(), bn.bias.data_ptr()
            h.bn_running_mean, h.bn_running_var = bn.running_mean.data_ptr(), bn.running_var.data_ptr()
            h.bn_eps, h.bn_momentum, h.bn_training = float(bn.eps), float(bn.momentum), 1 if bn_training else 0
            h.g_bn_weight, h.g_bn_bias = gptr(bn.weight), gptr(bn.bias)
            nbt = bn.num_batches_tracked
            if bn_training and nbt is not None and nbt.dtype == torch.int64 and nbt.device == dev:
                h.bn_num_batches_tracked = nbt.data_ptr()  # (counted by the batch-norm kernel: no launch of its own)
        h.n_layers, h.act, h.act_slope = len(self.layers), _lib.ACT[self.f_act], float(self.f_slope)
        h.dims[0] = self.n_components * d_out
        if X_d is not None:
            h.X_d, h.ld_xd = X_d.data_ptr(), X_d.stride(0)
            h.dims[0] = self.n_components * d_out + self.d_xd
        for l, lin in enumerate(self.layers):
            h.W[l], h.b[l] = lin.weight.data_ptr(), (None if lin.bias is None else lin.bias.data_ptr())
            h.dims[l + 1] = lin.out_features
            h.gW[l], h.gb[l] = gptr(lin.weight), gptr(lin.bias)
        h.loss = _lib.LOSS[self.kind]
        h.n_classes = self.n_classes
        h.evid_v_kl, h.evid_eps, h.quantile_alpha = self.v_kl, self.eps, self.q_alpha
        if self.spectral_act is not None:
            h.spectral_act, h.spectral_threshold = _lib.SPECTRAL_ACT[self.spectral_act], self.spectral_threshold
        h.targets = T.data_ptr()
        keep = [] if X_d is None else [X_d]
        if weights is not None:
            wt = engine._f32c(weights.reshape(-1, 1), "weights").reshape(-1).contiguous()
            h.weights = wt.data_ptr()
            keep.append(wt)
        tw = getattr(self.criterion, "task_weights", None)
        if tw is not None:
            tw = tw.reshape(-1).float()
            if tw.numel() == 1 and self.n_tasks > 1:  # (task_weights = 1.0 broadcasts over the tasks, metrics.py:69-70)
                tw = tw.expand(self.n_tasks)
            tw = tw.contiguous()
            h.task_weights = tw.data_ptr()
            keep.append(tw)
        for name, m in (("lt_mask", lt_mask), ("gt_mask", gt_mask)):
            if m is not None and self.bounded:   # (the reference's plain MSE / MAE ignore the masks: nn/metrics.py:139-150)
                m8 = m.to(torch.uint8).contiguous()
                setattr(h, name, m8.data_ptr())
                keep.append(m8)
        return keep

    def call_args(self, nV: int, n_mols: int, batch: Tensor, T: Tensor, weights, lt_mask, gt_mask, gptr, gHv: Tensor, **fill_kw) -> tuple:
        """A ``_lib.HeadArgs`` ready to launch: :meth:`fill` (``fill_kw``: its ``bn_training / X_d / ffn_dropout``), fresh ``preds
        [n_mols, n_out]`` and ``loss [2]``, the gradient of ``H_v`` into ``gHv`` (``[nV, d_out]``, any row stride) and the workspace
        the library asks for.  Returns ``(h, preds, loss, keep)``; ``keep`` must stay alive until the call is enqueued."""
        dev = T.device
        h = _lib.HeadArgs()
        keep = self.fill(h, nV, n_mols, int(gHv.shape[1]), batch, T, weights, lt_mask, gt_mask, gptr, **fill_kw)
        preds = torch.empty(n_mols, self.n_out, dtype=torch.float32, device=dev)
        loss = torch.empty(2, dtype=torch.float32, device=dev)
        h.preds, h.loss_out = preds.data_ptr(), loss.data_ptr()
        h.gHv, h.ldg = gHv.data_ptr(), gHv.stride(0)
        nb = int(_lib.load().dmpnn_head_ws_bytes(C.byref(h)))
        ws = torch.empty(max(nb, 16), dtype=torch.uint8, device=dev)
        h.ws, h.ws_bytes = ws.data_ptr(), nb
        keep.append(ws)
        return h, preds, loss, keep


class _HeadLoss(torch.autograd.Function):
    """Everything behind the block — aggregation, batch norm, the predictor's layers, the criterion — AND its backward pass as ONE
    ``dmpnn_head`` call in the forward of one autograd node: the loss comes back with the gradient of ``H_v`` and of every head
    parameter already computed (for a unit upstream gradient); ``backward`` scales them by the upstream gradient (one launch over
    one flat buffer) and hands them to autograd.  Replaces ~40 torch launches and autograd nodes of the module path."""

    @staticmethod
    def forward(ctx, spec, Hv, batch, n_mols, T, weights, lt_mask, gt_mask, X_d, *params):
        dev = Hv.device
        Hv = engine._f32c(Hv, "H_v")
        nV, d_out = int(Hv.shape[0]), int(Hv.shape[1])   # (a multicomponent H_v: every component's rows, one block's width)
        # one flat buffer for the head's parameter gradients (16-byte aligned pieces) + gH_v
        offs, n = [], 0
        for p in params:
            offs.append(n)
            n += (p.numel() + 3) // 4 * 4
        flat = torch.empty(n + nV * d_out, dtype=torch.float32, device=dev)
        ptr = {id(p): flat.data_ptr() + 4 * o for p, o in zip(params, offs)}
        want = {id(p) for p, need in zip(params, ctx.needs_input_grad[9:]) if need}
        gH = flat[n:].view(nV, d_out)
        h, preds, loss, keep = spec.call_args(nV, n_mols, batch, T, weights, lt_mask, gt_mask,
                                              lambda p: None if (p is None or id(p) not in want) else ptr[id(p)], gH,
                                              bn_training=spec.bn is None or spec.bn.training, X_d=X_d)
        with engine._OnDevice(dev):
            _lib.check(_lib.load().dmpnn_head(C.byref(h), Hv.data_ptr(), Hv.stride(0), engine._stream_ptr(dev)), "dmpnn_head")
        del keep
        ctx.flat, ctx.n, ctx.offs, ctx.shapes, ctx.want = flat, n, offs, [tuple(p.shape) for p in params], [id(p) in want for p in params]
        ctx.hv_shape = (nV, d_out)
        ctx.preds = preds
        return loss[0]

    @staticmethod
    def backward(ctx, gl):
        flat = ctx.flat * gl   # (ONE launch scales every gradient of the head by the upstream gradient)
        n = ctx.n
        gH = flat[n:].view(ctx.hv_shape) if ctx.needs_input_grad[1] else None
        gp = [flat[o:o + math.prod(sh)].view(sh) if w else None for o, sh, w in zip(ctx.offs, ctx.shapes, ctx.want)]
        return (None, gH, None, None, None, None, None, None, None, *gp)


def _head_spec_key(model) -> tuple:
    """What a spec cached on the model (``head_loss``, ``predict.predict_spec``) is keyed on: the identities of what it was read
    from — swapping model.predictor / criterion / bn / agg, or changing a predictor dropout p, after the first call must not leave
    the old modules in use (round-4 ADVICE)."""
    pred = model.predictor
    return (id(model.agg), id(model.bn), id(pred), id(getattr(pred, "criterion", None)), id(getattr(pred, "ffn", None)),
            id(getattr(pred, "output_transform", None)),
            tuple(float(getattr(m, "p", 0.0)) for m in pred.modules() if isinstance(m, nn.Dropout)) if isinstance(pred, nn.Module) else ())


def head_loss(model, Hv: Tensor, batch: Tensor, n_mols: int, targets: Tensor, weights: Optional[Tensor] = None,
              lt_mask: Optional[Tensor] = None, gt_mask: Optional[Tensor] = None, X_d: Optional[Tensor] = None) -> Optional[Tensor]:
    """``criterion(predictor.train_step(cat(bn(agg(H_v, batch)), X_d)), targets, ...)`` (``models/model.py:152-157``) as ONE autograd
    node on the head kernels (:class:`_HeadLoss`); ``X_d``: the molecule descriptors already through ``X_d_transform`` (no gradient
    flows to them).  ``None`` when the head kernels do not implement this model or these inputs — ``X_d`` that needs a gradient
    included (the caller then runs the torch modules)."""
    key = _head_spec_key(model)
    cached = model.__dict__.get("_dmpnn_head_spec")
    if cached is not None and cached[0] == key:
        spec = cached[1]
    else:
        try:
            spec = HeadSpec(model)
        except NotImplementedError as e:
            spec = str(e)
        model.__dict__["_dmpnn_head_spec"] = (key, spec)
    if isinstance(spec, str):
        return None
    if isinstance(Hv, (list, tuple)):
        # a multicomponent model: the blocks' outputs as ONE H_v of every component's rows (the fused step writes them in place)
        if spec.n_components != len(Hv) or len(batch) != len(Hv) or any(b is None for b in batch):
            return None
        batch = _component_batch(list(batch), n_mols)
        Hv = torch.cat(list(Hv)) if len(Hv) > 1 else Hv[0]
    elif spec.n_components != 1:
        return None
    if Hv.device.type != "cuda" or Hv.dtype != torch.float32:
        return None
    if not _batch_vector_ok(batch, Hv.shape[0], Hv.device):
        return None
    T = targets if (targets.dtype == torch.float32 and targets.is_contiguous()) else targets.float().contiguous()
    if T.dim() != 2 or T.shape[0] != n_mols or T.shape[1] != spec.n_tasks or (spec.bn is not None and spec.bn.training and n_mols < 2):
        return None
    if weights is not None and weights.numel() != n_mols:
        return None
    if X_d is not None and X_d.requires_grad:
        return None
    try:
        Xd = spec.descriptors(X_d, n_mols, Hv.device)
    except ValueError:
        return None
    return _HeadLoss.apply(spec, Hv, batch, int(n_mols), T, weights, lt_mask, gt_mask, Xd, *spec.params())


class _BlockPart:
    """One block's share of a step (``FusedTrainer._block_args``): plan, kept forward state, the backward's argument block, what they
    point into, the block's rows of ``H_v`` / ``gH_v``, the route, the step's dropout ``(p, seed)`` or ``None`` — and what K0 reads, named as ``dmpnn_step_args`` names it."""

    __slots__ = ("plan", "st", "bwd", "keep_b", "out", "gout", "route", "bmg", "edge_index", "rev_edge_index", "batch", "plan_bytes", "drop")

    def set_on(self, c, plan_ready: int) -> None:
        """Fill the fields ``_lib.StepArgs`` and ``_lib.StepComponent`` share."""
        c.edge_index, c.rev_edge_index, c.batch = self.edge_index, self.rev_edge_index, self.batch
        c.plan_bytes, c.plan_ready, c.bwd = self.plan_bytes, plan_ready, self.bwd


class FusedTrainer:
    """``training_step`` + ``Adam.step`` of an :class:`MPNN` as one ``dmpnn_train_step`` call per batch.

    Takes what the kernels implement and refuses the rest loudly (those models train through the module path): a
    :class:`~chemprop_amd.nn.BondMessagePassing` block with a built-in activation, directed, with or without atom descriptors
    (``d_vd > 0``: ``step(..., V_d=...)``, the layer ``W_d`` as a stage of its own behind the block), dropout 0 or — with a
    ReLU-class activation — ``nn.Dropout`` inside the tile kernels or, for molecules beyond the tile, inside the lean step kernels
    (d_h <= 320, depth 2 .. 8, even d_v / d_e; the same hash mask, one seed per step from torch's CPU generator); sum /
    mean / norm aggregation; optional ``nn.BatchNorm1d``; an MLP predictor with a built-in activation and dropout 0; MSE / MAE.
    A predictor wider than the block's output takes molecule descriptors: ``step(..., X_d=...)`` concatenates
    ``model.X_d_transform(X_d)`` behind the batch norm inside the same call (no gradient flows to ``X_d``).

    ``ffn_dropout=True`` also takes a predictor with dropout (one ``nn.Dropout`` shared by its blocks, as ``MLP.build`` makes it):
    ``step`` reads its ``p`` at every step and, while the model and that module are in training mode and ``p > 0``, draws one more
    seed from torch's CPU generator — after the block's — for the head's hash mask (``dmpnn_head_args.ffn_dropout_p``; kept as
    ``last_head_dropout_seed``); otherwise the head gets ``p = 0``.  The default refuses such a predictor.

    ``rows_dropout=True`` gives block dropout a third home behind the tile kernels and the lean step kernels: the row kernels of the
    per-step general route on the f16 pipe (``route == "general16"``; ``d_h <= 1024``, depth >= 1, relu / leakyrelu / tanh / elu / selu — what
    ``engine.rows_dropout_refusal`` takes), the same hash mask and the same one seed per step.  The default refuses what the first two
    homes do not take.

    ``vd_dropout=True`` also takes a block with atom descriptors AND dropout: the reference applies the block's ``nn.Dropout`` once
    more behind ``W_d``, and that fourth mask lives in the atom-descriptor stage's own kernels (site ``_lib.DROP_SITE_VD``;
    ``dmpnn_vd_args.dropout_p`` / ``dropout_seed`` are the block's ``(p, seed)`` of the step: still one draw, ``last_dropout_seed``).
    The backward stage overwrites ``gH_v'`` with the masked gradient.  The default refuses such a block.

    ``atom_messages=True`` also takes an ``AtomMessagePassing`` block (:func:`fused_block`).  Its two homes: with ``p = 0`` a batch
    bound for the tile kernels (no molecule beyond the tile, at most 30 directed edges per molecule, even ``d_v / d_e / d_h``) runs
    on them with ``DMPNN_F_ATOM``; everything else — molecules beyond the tile, wide or odd shapes, ``p > 0`` at any size — on the
    per-step general route on the f16 pipe (``route == "general16"``).  The default refuses such a block.

    ``undirected=True`` also takes a bond block with ``undirected`` messages (:func:`fused_block`): with ``p = 0`` on the route the
    engine's rule gives an undirected forward (``general`` / ``general16``, a full plan), with ``p > 0`` — ``rows_dropout=True`` as
    well — on the row kernels of the per-step general route on the f16 pipe with ``DMPNN_F_UNDIRECTED_MASK``; what those refuse is
    refused before a seed is drawn.  Not in a multicomponent model.  The default refuses such a block.

    ``attentive=True`` also takes a model with ``AttentiveAggregation`` (:class:`HeadSpec`): the attention is a stage of two kernels
    around the head inside the same call, its ``W`` trains with the head's slice of the flat buffer.  Not in a multicomponent model.
    The gradient of ``W.bias`` is analytically zero (the softmax is shift invariant): what the kernels — and the reference — return is
    rounding noise, which Adam turns into steps of about ``lr``.  The default refuses such a model.
    """

    def __init__(self, model: MPNN, lr: float = 1e-4, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 0.0, group=None,
                 tile_plan: bool = True, ffn_dropout: bool = False, rows_dropout: bool = False, vd_dropout: bool = False,
                 atom_messages: bool = False, undirected: bool = False, attentive: bool = False):
        mp, agg, pred = model.message_passing, model.agg, model.predictor
        # a multicomponent model: ONE block shared by every component (the components' graphs merged into one batch per step), or
        # one block per component (each block's forward into its rows of one H_v, the head once, each block's backward)
        multi = isinstance(getattr(mp, "blocks", None), nn.ModuleList) and hasattr(mp, "n_components")
        self.blocks = list(mp.blocks) if multi else [mp]
        self.shared = multi and all(b is self.blocks[0] for b in self.blocks)
        self.n_components = len(self.blocks) if multi else 1
        self.rows_dropout = bool(rows_dropout)
        self.vd_dropout = bool(vd_dropout)
        self.atom_messages = bool(atom_messages)
        self.undirected = bool(undirected)
        if multi and any(getattr(b, "undirected", False) for b in self.blocks):
            raise NotImplementedError("FusedTrainer: undirected blocks in a multicomponent model")
        if multi and any(is_atom_block(b) for b in self.blocks):
            raise NotImplementedError("FusedTrainer: atom blocks in a multicomponent model")
        acts = [fused_block(b, rows_dropout=self.rows_dropout, vd_dropout=self.vd_dropout, atom_messages=self.atom_messages,
                            undirected=self.undirected) for b in self.blocks]
        if multi and any(b.dropout.p > 0 for b in self.blocks):
            raise NotImplementedError("FusedTrainer: dropout inside the blocks of a multicomponent model")
        if multi and any(b.W_d is not None for b in self.blocks):
            raise NotImplementedError("FusedTrainer: atom descriptors (V_ds) in a multicomponent model")
        try:
            self.head = HeadSpec(model, ffn_dropout=ffn_dropout, attentive=attentive)
        except NotImplementedError as e:
            raise NotImplementedError(f"FusedTrainer: {e}") from None
        self.model, self.mp, self.multi, self.acts = model, self.blocks[0], multi, acts
        self.layers, self.bn, self.bounded = self.head.layers, self.head.bn, self.head.bounded
        params = [p for p in model.parameters() if p.requires_grad]
        engine._require_device(params[0], "model parameters")
        self.sync = GradSync(params, modules=[model], group=group)
        self.opt = FlatAdam(self.sync, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay)
        self.dev = params[0].device
        self._views = {id(p): v for p, v in zip(self.sync.params, self.sync.views)}
        # the two slices of the flat gradient buffer a data-parallel step exchanges one after the other (see step())
        blk = [p for p in mp.parameters() if p.requires_grad]   # (every component's block: one contiguous run)
        blk_ids = {id(p) for p in blk}
        rest = [p for p in params if id(p) not in blk_ids]
        self._block_range = self.sync.range_of(blk) if blk else (0, 0)
        self._head_range = self.sync.range_of(rest) if rest else (0, 0)
        self._checked = 0
        self.tile_plan = bool(tile_plan)   # False: always the full (CSR) plan — what every round before used; tests keep both alive
        self.last_route = None

    # ---- helpers ----
    def _gv(self, p: Optional[Tensor]) -> Optional[int]:
        if p is None or not p.requires_grad:
            return None
        return self._views[id(p)].data_ptr()

    def _world(self) -> int:
        d = torch.distributed
        return d.get_world_size(self.sync.group) if (d.is_available() and d.is_initialized()) else 1

    def step(self, bmg, targets: Tensor, weights: Optional[Tensor] = None, lt_mask: Optional[Tensor] = None,
             gt_mask: Optional[Tensor] = None, lr: Optional[float] = None, clip: Optional[tuple] = None,
             X_d: Optional[Tensor] = None, V_ds=None, V_d: Optional[Tensor] = None) -> Tensor:
        """One optimisation step on ``(bmg, targets, ...)`` (a ``TrainingBatch``); returns the device
        tensor ``[loss, number of finite targets]`` of THIS step (no host sync).  ``model.train()`` semantics (batch norm uses
        and updates batch statistics).  ``clip = (value, "norm" | "value")``: Lightning's ``gradient_clip_val`` / ``_algorithm``
        (``cli/train.py:1937``), applied between the backward pass and the update inside the same call.  ``X_d``: the batch's
        molecule descriptors ``[n_mols, d_xd]`` for a model whose predictor takes them (``ValueError`` when they are missing,
        unexpected or of the wrong shape); ``model.X_d_transform`` is applied to them here.  ``V_d``: the batch's atom descriptors
        ``[n_atoms, d_vd]`` for a block built with ``d_vd > 0`` (``ValueError`` when missing, unexpected or misshapen); the block's
        ``V_d_transform`` is applied to them here, no gradient flows to them.  The step is then K0, the block, ``dmpnn_vd_forward``,
        the head on ``H_v' = W_d cat(H_v, V_d) + b_d``, ``dmpnn_vd_backward``, the block's backward, clip, Adam — still one call.

        A :class:`MulticomponentMPNN`: ``bmg`` is the list of the components' batches, each of the same ``B`` molecules, and ``V_ds``
        ``None`` or a list of ``None`` (``ValueError`` otherwise)."""
        from .nn import _VALIDATE_FIRST_N

        comps, blocks, n_mols = self._components(bmg, V_ds)
        T, Vd, Xd = self._check_inputs(comps, n_mols, targets, weights, lt_mask, gt_mask, X_d, V_d)
        validate = _lib.opt("DMPNN_VALIDATE", "first") != "never" and self._checked < _VALIDATE_FIRST_N
        world = self._world()
        self.sync.wait()
        if validate:
            self._checked += 1
        # (everything the argument blocks point into lives in these locals until the call has been enqueued)
        parts, out, gout, vd, vd_keep = self._blocks(comps, blocks, validate, Vd)
        h, preds, loss, keep = self._head_args(comps, n_mols, T, weights, lt_mask, gt_mask, Xd, gout)
        s, extra = self._step_args(parts, h, vd, validate)
        if clip is not None:   # (normalised: None, or a positive value and its mode)
            clip = (float(clip[0]), clip[1] or "norm") if (clip[0] is not None and float(clip[0]) > 0) else None
        # (None: the staged data-parallel step — the update is opt.step's; DMPNN_FORCE_COLLECTIVE takes it on one rank too)
        k = self._optimizer_args(s, lr, clip) if (world == 1 and not force_collective()) else None
        self._launch(s, staged=k is None)
        self._commit(h, preds, k, lr, clip)
        return loss

    def _components(self, bmg, V_ds) -> tuple:
        """``(comps, blocks, n_mols)``: the batches the blocks run on and the block of each; a shared block takes the components merged
        into ONE batch of ``n B`` molecules, numbered ``c B + i`` (the head folds it back into ``[B, n d_h]``)."""
        if not self.multi:
            if V_ds is not None:
                raise ValueError("FusedTrainer.step: V_ds is for multicomponent models")
            engine._require_device(bmg.V, "bmg.V")
            return [bmg], [self.mp], len(bmg)
        bmgs = list(bmg)
        if len(bmgs) != self.n_components:
            raise ValueError(f"FusedTrainer.step: {self.n_components} component batches expected, got {len(bmgs)}")
        if V_ds is not None and any(v is not None for v in V_ds):
            raise ValueError("FusedTrainer.step: atom descriptors (V_ds) per component are not taken by the fused step")
        if len({len(b) for b in bmgs}) != 1:
            raise ValueError(f"FusedTrainer.step: every component must hold the same number of molecules, got {[len(b) for b in bmgs]}")
        for b in bmgs:
            engine._require_device(b.V, "bmg.V")
        return ([merge_components(bmgs)], [self.mp], len(bmgs[0])) if self.shared else (bmgs, self.blocks, len(bmgs[0]))

    def _check_inputs(self, comps, n_mols: int, targets, weights, lt_mask, gt_mask, X_d, V_d) -> tuple:
        """Everything that refuses a step for its inputs — before anything is counted, drawn or enqueued.  Returns the targets, the
        atom descriptors and the molecule descriptors as the kernels read them (the two through their transforms; ``None``: none)."""
        if not self.model.training:
            # (batch norm would update its running statistics while the block's dropout follows model.training: the two switches
            #  must not disagree — and a training step of a model in eval mode is a bug of the caller, not a mode)
            raise RuntimeError("FusedTrainer.step: the model is in eval mode — call model.train() first")
        Vd = self._atom_descriptors(V_d, comps[0])
        n_tasks = self.head.n_tasks
        T = engine._f32c(targets, "targets")
        if T.dim() != 2 or T.shape[0] != n_mols or T.shape[1] != n_tasks or not T.is_contiguous():
            raise ValueError(f"targets must be a contiguous [{n_mols}, {n_tasks}] matrix, got {tuple(targets.shape)}")
        for cb in comps:
            if not _batch_vector_ok(cb.batch, int(cb.V.shape[0]), cb.V.device):
                raise ValueError(f"bmg.batch must be a contiguous int64 vector of {int(cb.V.shape[0])} molecule ids on {cb.V.device}")
        if weights is not None and weights.numel() != n_mols:
            raise ValueError(f"weights must hold one value per molecule ({n_mols}), got {tuple(weights.shape)}")
        for name, m in (("lt_mask", lt_mask), ("gt_mask", gt_mask)):
            if m is not None and tuple(m.shape) != (n_mols, n_tasks):
                raise ValueError(f"{name} must have the targets' shape [{n_mols}, {n_tasks}], got {tuple(m.shape)}")
        if self.bn is not None and n_mols == 1:
            raise ValueError("Expected more than 1 value per channel when training (batch norm on a batch of one molecule)")
        if X_d is not None and self.head.d_xd and tuple(X_d.shape) == (n_mols, self.head.d_xd):
            xt = getattr(self.model, "X_d_transform", None)
            with torch.no_grad():
                X_d = X_d if xt is None else xt(X_d)
        return T, Vd, self.head.descriptors(X_d, n_mols, self.dev)

    def _blocks(self, comps, blocks, validate: bool, Vd: Optional[Tensor]) -> tuple:
        """Every block's argument blocks (:meth:`_block_args`) and the atom-descriptor stage's (:meth:`_vd_args`).  ``out`` / ``gout``
        are what the head reads / writes: with a block per component ONE ``H_v`` / ``gH_v`` that every block takes its rows of, with
        atom descriptors ``H_v'`` / ``gH_v'`` ``[n_atoms, d_h + d_vd]``."""
        H_all = g_all = None
        if len(comps) > 1:
            nV_all, d_blk = sum(int(cb.V.shape[0]) for cb in comps), int(blocks[0].output_dim)
            H_all = torch.empty(nV_all, d_blk, dtype=torch.float32, device=self.dev)
            g_all = torch.empty(nV_all, d_blk, dtype=torch.float32, device=self.dev)
        parts, row = [], 0
        for mp, cb in zip(blocks, comps):
            nV_c = int(cb.V.shape[0])
            parts.append(self._block_args(mp, cb, len(cb), self.acts[self.blocks.index(mp)], validate,
                                          None if H_all is None else H_all[row:row + nV_c], None if g_all is None else g_all[row:row + nV_c]))
            row += nV_c
        self.last_route = parts[0].route if len(parts) == 1 else tuple(p.route for p in parts)
        self._last_plan_tiles = all(p.plan.tiles_only for p in parts)
        out, gout = (parts[0].out, parts[0].gout) if H_all is None else (H_all, g_all)
        return (parts, out, gout, None, None) if Vd is None else (parts, *self._vd_args(self.mp, Vd, out, gout, parts[0].drop))

    def _head_args(self, comps, n_mols: int, T: Tensor, weights, lt_mask, gt_mask, Xd, gout: Tensor) -> tuple:
        """The head's argument block (:meth:`HeadSpec.call_args`) over every component's rows, its gradients into the flat buffer's
        views and ``gout``; with an active predictor dropout one seed from torch's CPU generator first — drawn after the block's."""
        batch = _component_batch([cb.batch for cb in comps], n_mols)
        if self.multi:
            note_batch(batch, self.n_components * n_mols)
        hdrop = None
        drop = self.head.drop
        if drop is not None and drop.training and float(drop.p) > 0:
            if not float(drop.p) < 1:
                raise ValueError(f"FusedTrainer.step: the predictor's dropout needs p < 1, got {drop!r}")
            hdrop = (float(drop.p), int(torch.randint(0, 2 ** 62, (1,), dtype=torch.int64).item()))
            self.last_head_dropout_seed = hdrop[1]
        h, preds, loss, keep = self.head.call_args(int(gout.shape[0]), n_mols, batch, T, weights, lt_mask, gt_mask, self._gv, gout,
                                                   X_d=Xd, ffn_dropout=hdrop)
        keep.append(batch)
        return h, preds, loss, keep

    @staticmethod
    def _step_args(parts: list, h, vd, validate: bool) -> tuple:
        """``dmpnn_step_args`` from the parts: component 0 inline, the further ones as an array (returned: it must stay alive)."""
        s = _lib.StepArgs()
        ready = 1 if validate else 0   # (while the first batches are validated, K0 was launched with the plan: _block_args)
        parts[0].set_on(s, ready)
        s.head = h
        if vd is not None:
            s.vd = C.pointer(vd)
        extra = None
        if len(parts) > 1:
            extra = (_lib.StepComponent * (len(parts) - 1))()
            for e, pc in zip(extra, parts[1:]):
                pc.set_on(e, ready)
            s.n_extra, s.extra = len(parts) - 1, C.cast(extra, C.POINTER(_lib.StepComponent))
        return s, extra

    def _optimizer_args(self, s, lr: Optional[float], clip: Optional[tuple]) -> int:
        """Adam's scalars and the clip for an update inside the call; returns the step count to commit once the call has returned OK
        (a refused step must not advance Adam's bias correction)."""
        opt = self.opt
        k = opt.steps + 1
        b1, b2 = opt.betas
        s.p, s.g, s.m, s.v, s.n_params = opt.flat.data_ptr(), self.sync.flat.data_ptr(), opt.m.data_ptr(), opt.v.data_ptr(), opt.flat.numel()
        s.lr, s.beta1, s.beta2, s.eps, s.weight_decay = float(opt.lr if lr is None else lr), b1, b2, opt.eps, opt.weight_decay
        (s.bias_corr1, s.sqrt_bias_corr2), s.grad_scale = bias_corrections(opt.betas, k), 1.0   # (from the betas as float32: optim.py)
        if clip is not None:
            s.clip_val, s.clip_mode, s.clip_ws = clip[0], CLIP_MODES[clip[1]], opt.clip_ws.data_ptr()
        return k

    def _launch(self, s, staged: bool) -> None:
        """The step as one call — or, data parallel, as two: the head's gradients (predictor, batch norm) are final before the block's
        backward pass starts, so their slice of the flat buffer goes out on the communication stream while that pass runs; the
        block's slice follows it; the update waits (stream dependency) for both."""
        lib = _lib.load()
        with engine._OnDevice(self.dev):
            stream = engine._stream_ptr(self.dev)
            if not staged:
                _lib.check(lib.dmpnn_train_step(C.byref(s), stream), "dmpnn_train_step")
                return
            s.stages = _lib.STEP_FORWARD
            _lib.check(lib.dmpnn_train_step(C.byref(s), stream), "dmpnn_train_step(forward)")
            self.sync.allreduce(*self._head_range)
            s.stages = _lib.STEP_BACKWARD
            _lib.check(lib.dmpnn_train_step(C.byref(s), stream), "dmpnn_train_step(backward)")
            self.sync.allreduce(*self._block_range)

    def _commit(self, h, preds: Tensor, k: Optional[int], lr, clip) -> None:
        """The bookkeeping of a step that was taken: the batch norm's count where the kernel did not keep it, ``preds``, and either
        Adam's step count and the parameters' versions (``k``: the update ran inside the call) or the update itself (``opt.step``)."""
        bn = self.bn
        if bn is not None and not h.bn_num_batches_tracked and bn.num_batches_tracked is not None:
            bn.num_batches_tracked += 1
        self.preds = preds
        if k is None:
            self.opt.step(lr, clip=clip)
            return
        self.opt.steps = k
        for p in self.sync.params:  # (the engine's weight caches key on the autograd version)
            torch.autograd.graph.increment_version(p)
        self.sync.new_step()

    def _atom_descriptors(self, V_d: Optional[Tensor], bmg) -> Optional[Tensor]:
        """``V_d`` through the block's ``V_d_transform`` as fp32 rows ``[n_atoms, d_vd]`` on the device (``None``: a block without
        ``W_d``); ``ValueError`` when they are missing, unexpected or misshapen — the three refusals of ``X_d``."""
        W_d = None if self.multi else self.mp.W_d
        if W_d is None:
            if V_d is not None:
                raise ValueError("V_d given, but this model's block takes no atom descriptors (it was built without d_vd)")
            return None
        d_vd = int(W_d.in_features - self.mp.W_o.out_features)
        if V_d is None:
            raise ValueError(f"this model's block expects {d_vd} atom descriptors per atom (V_d), got none")
        nV = int(bmg.V.shape[0])
        if V_d.dim() != 2 or tuple(V_d.shape) != (nV, d_vd):
            raise ValueError(f"V_d must be [{nV}, {d_vd}], got {tuple(V_d.shape)}")
        if V_d.device != self.dev:
            raise ValueError(f"V_d must live on {self.dev}, got {V_d.device}")
        xt = getattr(self.mp, "V_d_transform", None)
        with torch.no_grad():
            V = V_d if xt is None else xt(V_d)
        V = V.detach()
        if V.dtype != torch.float32 or V.stride(1) != 1 or tuple(V.shape) != (nV, d_vd):
            V = V.to(torch.float32).contiguous()
        return V

    def _vd_args(self, mp, Vd: Tensor, Hv: Tensor, gHv: Tensor, drop: Optional[tuple] = None) -> tuple:
        """``dmpnn_vd_args`` of the layer ``W_d`` behind the block's output ``Hv`` (its gradient goes to ``gHv``): allocates ``H_v'``,
        ``gH_v'`` and the workspace, takes the gradient views of ``W_d`` from the flat buffer (``None`` for a frozen parameter).
        ``drop``: the block's ``(p, seed)`` of this step (``None``: no dropout) — the same module masks ``H_v'``."""
        lib = _lib.load()
        nV, d_h = int(Hv.shape[0]), int(Hv.shape[1])
        D = int(mp.W_d.out_features)
        Wd, bd = mp.W_d.weight, mp.W_d.bias
        if Wd.dtype != torch.float32 or not Wd.is_contiguous() or bd.dtype != torch.float32 or not bd.is_contiguous():
            raise NotImplementedError("FusedTrainer: W_d must be contiguous float32")
        out2 = torch.empty(nV, D, dtype=torch.float32, device=self.dev)
        gout2 = torch.empty(nV, D, dtype=torch.float32, device=self.dev)
        a = _lib.VdArgs()
        a.n_atoms, a.d_h, a.d_vd = nV, d_h, D - d_h
        a.Hv, a.ldhv = Hv.data_ptr(), Hv.stride(0)
        a.V_d, a.ldvd = Vd.data_ptr(), Vd.stride(0)
        a.W_d, a.b_d = Wd.data_ptr(), bd.data_ptr()
        a.out, a.ldout = out2.data_ptr(), out2.stride(0)
        a.gout, a.ldgout = gout2.data_ptr(), gout2.stride(0)
        a.gHv, a.ldghv = gHv.data_ptr(), gHv.stride(0)
        a.gW_d, a.gb_d = self._gv(Wd), self._gv(bd)
        if drop is not None:
            if not self.vd_dropout:   # (fused_block refused it at construction: p was raised on the module since)
                raise NotImplementedError("FusedTrainer: atom descriptors (W_d) together with dropout inside the block needs vd_dropout=True")
            a.dropout_p, a.dropout_seed = drop
        nb = int(lib.dmpnn_vd_ws_bytes(C.byref(a)))
        ws = torch.empty(max(nb, 16), dtype=torch.uint8, device=self.dev)
        a.ws, a.ws_bytes = ws.data_ptr(), nb
        return out2, gout2, a, [Vd, Hv, gHv, ws, Wd, bd]

    def _rows_gate(self, mp, bmg, act: str, what: str, **kind) -> None:
        """A block whose only dropout home is the row kernels (``what``; ``kind``: its ``rows_dropout_refusal`` switches): what they
        refuse is refused here, before a seed is drawn."""
        d_v, d_e, d_h = int(bmg.V.shape[1]), int(bmg.E.shape[1]), int(mp.W_h.weight.shape[0])
        why = None if self.rows_dropout else "rows_dropout=False"
        why = why or engine.rows_dropout_refusal(d_v, d_e, d_h, int(mp.depth), act, **kind)
        if why is None and (type(mp.dropout) is not nn.Dropout or float(mp.dropout.p) >= 1.0):
            why = "nn.Dropout with p < 1"
        if why is None and (bmg.V.dtype != torch.float32 or bmg.V.stride(0) % 2 or bmg.V.data_ptr() % 8):
            why = "V rows must be fp32, 8-byte aligned with an even stride"
        if why is not None:
            raise NotImplementedError(f"FusedTrainer: dropout inside {what} lives in the row kernels, which refuse it ({why}); "
                                      "this model trains through the module path (MPNN.loss + autograd)")

    def _block_plan(self, mp, bmg, n_mols: int, validate: bool, atom: bool, p: float) -> tuple:
        """``(plan, level)``: K0's plan of one block — launched while the first batches are validated (host read of the verdict), else
        built inside the C call — and the cap on its route (2: the tile kernels).  Once the first batches are validated, a batch bound
        for the tile kernels gets the TILE plan: K0 is then the 11 us tile table instead of the 28 us CSR plan, the kept tensors stay
        in the caller's edge order and the backward tile kernel reads the batch's own index arrays (``DMPNN_F_TILE_PLAN``; every tile
        checks itself, a molecule beyond the tile takes the kernels' generic path)."""
        from .nn import _route, _training_plan_kind, batch_oversize

        nV, nE, d_v, d_e = int(bmg.V.shape[0]), int(bmg.E.shape[0]), int(bmg.V.shape[1]), int(bmg.E.shape[1])
        no_mega = getattr(mp, "_dmpnn_no_mega", False) or (n_mols > 0 and nE > 30 * n_mols)
        oversize = getattr(bmg, "oversize", None)
        if atom:
            # the atom tile kernels carry no mask, take even shapes only, and answer NaN for a molecule beyond the tile: the host must KNOW
            tile_shapes = p == 0 and d_e >= 2 and d_v % 2 == 0 and d_e % 2 == 0 and int(mp.W_h.weight.shape[0]) % 2 == 0 and nE > 0
            count = tile_shapes
        else:
            # (with dropout the tile kernels' generic path for a molecule beyond the tile answers NaN as well — which this step would
            #  feed to Adam; such a batch goes to the lean step kernels instead)
            tile_shapes, count = True, mp.dropout.p > 0 and not mp.undirected
        if oversize is None and count and not no_mega:
            oversize = batch_oversize(bmg, n_mols)   # (a foreign batch is counted on the device)
        level = 2 if (tile_shapes and not no_mega and (oversize is False if atom else oversize is not True)) else 1
        # (ONE rule for "this training forward runs on the tile plan", the module path's: shapes of the tile kernel — d_h <= 320, even
        #  d_v / d_e —, the environment switches, a plan the library can build; anything else keeps the full plan and the per-step routes)
        kind = _training_plan_kind(mp, bmg, atom=atom, vd_outside=True) if (self.tile_plan and not validate and level == 2) else False
        if atom and not kind and level == 2 and not validate:
            # (no tile plan for these shapes / this batch size: the full plan serves the atom tile kernels only within the single-workgroup plan)
            level = 2 if engine.small_plan_fits(nV, nE) else 1
        plan = engine.GraphPlan.from_bmg(bmg, light=kind, launch=validate)
        plan.oversize = oversize
        if validate:
            level = min(level, _route(mp, plan, n_mols, bmg.batch))
        if plan.tiles_only and level < 2:  # (cannot happen: the tile plan was only asked for at level 2)
            raise RuntimeError("FusedTrainer: a tile plan without the tile kernels")
        if not self.multi:
            note_batch(bmg.batch, n_mols)
        return plan, level

    def _draw_seed(self, p: float) -> Optional[tuple]:
        """The step's ``(p, seed)``: one seed from torch's CPU generator (``torch.manual_seed`` fixes the run), like the module path's
        fused dropout — after every refusal of the step's own, before anything is prepared.  ``None``: no dropout."""
        if not p > 0:
            return None
        drop = (p, int(torch.randint(0, 2 ** 62, (1,), dtype=torch.int64).item()))
        self.last_dropout_seed = drop[1]
        return drop

    @staticmethod
    def _prepare(mp, plan, bmg, act_slope: tuple, drop: Optional[tuple], out: Optional[Tensor]):
        """``fwd(**demands on the route)``: ``engine.forward`` of a block's kept forward, prepared and not enqueued."""
        from .nn import _param as W

        return lambda **kw: engine.forward(
            plan, bmg.V, bmg.E, W(mp, "W_i", "weight"), W(mp, "W_h", "weight"), W(mp, "W_o", "weight"), W(mp, "W_o", "bias"),
            W(mp, "W_i", "bias"), W(mp, "W_h", "bias"), depth=mp.depth, act=act_slope[0], slope=act_slope[1], keep=True,
            launch=False, dropout=drop, out=out, **kw)

    def _block_args(self, mp, bmg, n_mols: int, act_slope: tuple, validate: bool, out: Optional[Tensor], gout: Optional[Tensor]) -> "_BlockPart":
        """K0's plan and the argument blocks of one block's forward / backward on ``bmg`` (workspace allocated, nothing enqueued but —
        while the first batches are validated — the plan).  ``out`` / ``gout``: the block's rows of a multicomponent step's H_v / gHv
        (``None``: allocated here).  The homes of a block's forward:

        * a directed bond block: the tile kernels; with ``p > 0`` and molecules beyond the tile — at any edge count — the lean step
          kernels, which the route rule never picks for ``p > 0`` (the step asks: ``route="fused16"`` on the full plan); with
          ``rows_dropout`` the row kernels of the per-step general route on the f16 pipe take what those two refuse;
        * an undirected bond block with ``p > 0``: the row kernels only;
        * an atom block (``DMPNN_F_ATOM``): the tile kernels (``p = 0``, no molecule beyond the tile, at most 30 directed edges per
          molecule, even ``d_v / d_e / d_h``), else the per-step general route on the f16 pipe, with ``p > 0`` at any molecule size.
        Every refusal of the step's own comes before the seed is drawn, the seed before anything is prepared."""
        act = act_slope[0]
        atom = self.atom_messages and is_atom_block(mp)
        und = bool(mp.undirected)   # (taken at construction with undirected=True only: the general route, a full plan)
        p = float(mp.dropout.p) if self.model.training else 0.0
        d_v, d_e, d_h = int(bmg.V.shape[1]), int(bmg.E.shape[1]), int(mp.W_h.weight.shape[0])
        if atom and (int(mp.W_i.weight.shape[1]) != d_v or int(mp.W_h.weight.shape[1]) != d_h + d_e or not 1 <= d_e <= 16):
            raise NotImplementedError(f"FusedTrainer: the batch's features (d_v {d_v}, d_e {d_e}) are not the atom block's "
                                      f"(W_i {tuple(mp.W_i.weight.shape)}, W_h {tuple(mp.W_h.weight.shape)}; 1 <= d_e <= 16)")
        if atom and p > 0:   # (before the plan: its prologue may count the batch's molecules on the device)
            self._rows_gate(mp, bmg, act, "an atom block", atom=True)
        plan, level = self._block_plan(mp, bmg, n_mols, validate, atom, p)
        if und and p > 0:
            self._rows_gate(mp, bmg, act, "an undirected block", undirected=True, undirected_dropout=True)
        drop = self._draw_seed(p)
        fwd = self._prepare(mp, plan, bmg, act_slope, drop, out)
        st = None
        if atom:
            if level == 2:
                try:
                    out, st = fwd(atom=True, max_level=2)
                except engine.RouteUnavailable:
                    if plan.tiles_only:
                        raise RuntimeError("FusedTrainer: a tile plan without the atom tile kernels") from None
            if st is None:   # (the general route on demand: for every p)
                try:
                    out, st = fwd(atom=True, route="general", mfma="split16")
                except engine.RouteUnavailable as e:
                    raise NotImplementedError(f"FusedTrainer: neither the tile kernels nor the per-step general route take this atom block ({e}); "
                                              "it trains through the module path (MPNN.loss + autograd)") from None
        elif und and drop is not None:
            try:
                out, st = fwd(undirected=True, route="general", mfma="split16", undirected_dropout=True)
            except engine.RouteUnavailable as e:
                raise NotImplementedError(f"FusedTrainer: the row kernels refuse this undirected block with dropout ({e}); it trains through "
                                          "the module path (MPNN.loss + autograd)") from None
        else:   # a bond block: tile, then lean, then rows
            tile_why = "molecules beyond the tile"
            if drop is None or level == 2 or plan.tiles_only:
                try:
                    out, st = fwd(undirected=und, max_level=level)
                except engine.RouteUnavailable as e:
                    tile_why = str(e)
                    if drop is None or plan.tiles_only or getattr(plan, "light", False):
                        raise NotImplementedError(f"FusedTrainer: this batch does not take the tile kernels ({e}); dropout on the other routes "
                                                  "runs through the module path (MPNN.loss + autograd)") from None
            if st is None:
                why = engine.lean_dropout_refusal(d_v, d_e, d_h, int(mp.depth), act)
                if why is None:
                    try:
                        out, st = fwd(undirected=und, route="fused16")
                    except engine.RouteUnavailable as e:
                        why = str(e)
                    except RuntimeError as e:   # (only the refusal of the demanded route is this step's to translate)
                        if "route 'fused16' requested but not available" not in str(e):
                            raise
                        why = str(e)
                rows_why = None
                if st is None and self.rows_dropout:
                    rows_why = engine.rows_dropout_refusal(d_v, d_e, d_h, int(mp.depth), act)
                    if rows_why is None:
                        try:
                            out, st = fwd(undirected=und, route="general", mfma="split16")
                        except engine.RouteUnavailable as e:
                            rows_why = str(e)
                if st is None:
                    raise NotImplementedError(f"FusedTrainer: this batch does not take the tile kernels ({tile_why}) and the lean step kernels "
                                              f"refuse it ({why})" + (f", and so do the row kernels ({rows_why})" if self.rows_dropout else "")
                                              + "; dropout on the other routes runs through the module path (MPNN.loss + autograd)") from None
        return self._finish_block_args(mp, bmg, plan, st, out, gout, drop)

    def _finish_block_args(self, mp, bmg, plan, st, out: Tensor, gout: Optional[Tensor], drop) -> "_BlockPart":
        """The backward's argument block for a prepared forward ``st`` (gradients into the flat buffer's views) and the block's part."""
        from .nn import _param

        batch = bmg.batch
        nV = int(bmg.V.shape[0])
        d_out = int(out.shape[1])
        if gout is None:
            gout = torch.empty(nV, d_out, dtype=torch.float32, device=self.dev)
        need, views = {}, {}
        for k, (lin, n) in dict(W_i=("W_i", "weight"), b_i=("W_i", "bias"), W_h=("W_h", "weight"), b_h=("W_h", "bias"),
                                W_o=("W_o", "weight"), b_o=("W_o", "bias")).items():
            p = _param(mp, lin, n)
            need[k] = p is not None and p.requires_grad
            if need[k]:
                views[k] = self._views[id(p)]
        grads, b, keep_b = engine.backward(st, gout, need, out=views, launch=False)
        for k, g in grads.items():  # (a view the engine did not take would silently drop the gradient)
            if g is not None and g is not views.get(k):
                raise RuntimeError(f"FusedTrainer: the gradient view of {k} was not accepted (dtype / layout)")
        part = _BlockPart()
        part.plan, part.st, part.bwd, part.keep_b, part.out, part.gout, part.route, part.bmg = plan, st, b, keep_b, out, gout, st.route, bmg
        part.drop = drop
        part.edge_index, part.rev_edge_index = plan.edge_index.data_ptr(), plan.rev_edge_index.data_ptr()
        part.batch = batch.data_ptr()   # (int64, contiguous: _check_inputs)
        part.plan_bytes = plan.buf.numel() * 4
        return part
