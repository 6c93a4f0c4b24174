"""Dispatch of one BondMessagePassing forward onto the HIP kernels (+ autograd wiring).

Two routes, both entirely on HIP kernels for the arithmetic of the path:

* **fused** — ``tau`` is one of chemprop's built-in activations (nn/utils.py:43-53) and dropout is
  inactive (p == 0 or eval): one ``dmpnn_forward`` C call enqueues the whole chain.
* **rows**  — arbitrary ``nn.Module`` activation, learnable PReLU under grad, or active dropout:
  the row kernels (linear / message / aggregate) are chained from Python and the activation /
  dropout *modules themselves* run in between (so their RNG and parameters behave as in the
  reference, base.py:135-141,180-194).
"""
from __future__ import annotations

from typing import Optional

import torch
from torch import Tensor

from . import engine


_FUSED_ARGS = ("W_i", "b_i", "W_h", "b_h", "W_o", "b_o", "W_d", "b_d")   # the tensors behind FusedMP.apply's options, in its order


def _params(mp):
    g = lambda lin, n: None if lin is None else getattr(lin, n)
    return dict(W_i=mp.W_i.weight, b_i=mp.W_i.bias, W_h=mp.W_h.weight, b_h=mp.W_h.bias,
                W_o=mp.W_o.weight, b_o=mp.W_o.bias, W_d=g(mp.W_d, "weight"), b_d=g(mp.W_d, "bias"))


def _wants_grad(mp, *tensors) -> bool:
    if not torch.is_grad_enabled():
        return False
    if any(p.requires_grad for p in mp.parameters()):
        return True
    return any(t is not None and t.requires_grad for t in tensors)


def input_grad_wanted(*tensors) -> bool:
    """An input of the block (``bmg.V``, ``bmg.E``, ``V_d``) requires grad under an enabled autograd: the forward then needs a FULL
    plan and the route cap 0 (the per-step general route or the rows route: the two that return input gradients)."""
    return torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in tensors)


def input_grad_plan(in_grad: bool, light, level: int) -> tuple:
    """The routing decision of ``message_passing_forward`` for input gradients, as a pure function: ``(plan kind, route cap)`` —
    a full plan (no light plan, no tile plan) and level 0 whenever an input requires grad, else what the caller had."""
    return (False, 0) if in_grad else (light, level)


def mp_forward(mp, plan: engine.GraphPlan, V: Tensor, E: Tensor, V_d: Optional[Tensor],
               max_level: int = 2) -> Tensor:
    from .nn import classify_activation

    act, slope, slope_t = classify_activation(mp.tau)
    drop_active = mp.training and mp.dropout.p > 0
    grad = _wants_grad(mp, V, E, V_d)
    p = _params(mp)
    has_vd = mp.W_d is not None and V_d is not None
    # V, E or V_d requires grad (attributions on a frozen model, a learned featurizer / descriptor network in front of the block): the
    # per-step general route, whose backward pass also returns the input gradients (dmpnn_backward_inputs) — a built-in activation
    # other than PReLU with inactive dropout; everything else takes the rows route below, where every row Function has a data gradient
    in_grad = input_grad_wanted(V, E, V_d if has_vd else None)
    if in_grad and act not in ("custom", "prelu") and not drop_active:
        from .backward import FusedMP, FusedOptions

        return FusedMP.apply(mp, plan, V, E, V_d if has_vd else None, act, slope, FusedOptions(slope_t=slope_t, max_level=0, route="general"),
                             *[p[k] for k in _FUSED_ARGS])
    # (the dropout scale of the backward pass lives in the backward TILE kernel, which only runs when a gradient of W_i or W_h is
    #  wanted: a block with both frozen — W_o alone trainable — keeps the rows route)
    edge_grad = any(t is not None and t.requires_grad for t in (p["W_i"], p["b_i"], p["W_h"], p["b_h"]))
    if (drop_active and grad and edge_grad and act in ("relu", "leakyrelu") and not has_vd and max_level >= 2
            and type(mp.dropout) is torch.nn.Dropout and not in_grad):
        # ACTIVE dropout inside the tile kernels (round 3): the mask is a counter-based hash of (seed, site, row, column), the seed
        # one draw from torch's CPU generator (so torch.manual_seed fixes the run); a batch that takes another route falls
        # through to the rows route below, where the block's own nn.Dropout runs between the kernels (as does any module that is not
        # exactly nn.Dropout: a subclass has its own semantics)
        seed = int(torch.randint(0, 2 ** 62, (1,), dtype=torch.int64).item())
        try:
            from .backward import FusedMP, FusedOptions

            return FusedMP.apply(mp, plan, V, E, None, act, slope,
                                 FusedOptions(slope_t=slope_t, max_level=max_level, dropout=(float(mp.dropout.p), seed)), *[p[k] for k in _FUSED_ARGS])
        except engine.RouteUnavailable:
            pass
    use_rows = act == "custom" or drop_active or (act == "prelu" and grad) or in_grad

    if not use_rows:
        if grad:
            from .backward import FusedMP, FusedOptions

            return FusedMP.apply(mp, plan, V, E, V_d if has_vd else None, act, slope, FusedOptions(slope_t=slope_t, max_level=max_level),
                                 *[p[k] for k in _FUSED_ARGS])
        out, st = engine.forward(plan, V, E, p["W_i"], p["W_h"], p["W_o"], p["b_o"], p["b_i"], p["b_h"],
                                 p["W_d"] if has_vd else None, p["b_d"] if has_vd else None,
                                 V_d if has_vd else None, depth=mp.depth, act=act, slope=slope,
                                 slope_t=slope_t, undirected=mp.undirected, keep=False, max_level=max_level,
                                 wcache=mp.__dict__.setdefault("_dmpnn_wcache", {}))
        mp.__dict__["_dmpnn_last"] = st  # (nn.py builds the replay state of the steady inference path from it)
        return out

    from .nn import _Block

    return rows_forward(_Block(mp), plan, V, E, V_d, grad=grad, in_grad=in_grad)[0]


def _direct_linear(A1, W, b, A2=None, gather=None, n_rows=None, Cadd=None, plan=None):
    return engine.linear(A1, W, b, A2=A2, gather1=gather, n_rows=n_rows, Cadd=Cadd)


def edge_readout(blk, linear_fn, E: Tensor, H: Tensor, E_d: Optional[Tensor]) -> Tensor:
    """``edge_finalize`` of the mol-atom-bond blocks (mol_atom_bond.py:221-264) on the last edge states ``H``."""
    H_e = blk.dropout(blk.tau(linear_fn(E, blk.W_eo.weight, blk.W_eo.bias, A2=H)))
    if E_d is not None:
        H_e = blk.dropout(linear_fn(H_e, blk.W_ed.weight, blk.W_ed.bias, A2=E_d))
    return H_e


def rows_forward(blk, plan: engine.GraphPlan, V: Tensor, E: Tensor, V_d: Optional[Tensor] = None, E_d: Optional[Tensor] = None, *,
                 grad: bool, in_grad: bool) -> tuple:
    """The rows route of every block (``blk``: ``nn._Block``) -> ``(H_v | None, H_e | None)``: a row kernel for every contraction /
    segment operation, the block's own ``tau`` / dropout MODULES between them (base.py:135-141,180-194; mixins.py:8-30;
    mol_atom_bond.py:174-264).  Bond messages ``M = message(H)``, atom messages ``M = [(segsum_dst H)[src] || (segsum_dst E)[src]]``
    — the second half constant over the loop, formed once, through its Functions when ``E`` requires grad.

    ``grad``: chain the autograd Functions of ``backward.py``; ``False`` calls the engine directly (the bond forward without a
    gradient to record; the atom and mol-atom-bond forwards always pass ``True``).  ``in_grad``: an input requires grad — the first
    contraction then carries the plan, for the gradient of the gathered ``V``."""
    if grad:
        from .backward import aggregate_fn, gather_src_fn, linear_fn, message_fn
    else:
        assert not blk.atom, "rows_forward(grad=False) serves bond messages only (no direct form of the source gather)"
        linear_fn, message_fn, aggregate_fn = _direct_linear, engine.message, engine.aggregate
    tau, drop, W_i, W_h = blk.tau, blk.dropout, blk.W_i, blk.W_h
    nE = plan.n_edges
    H0 = linear_fn(V, W_i.weight, W_i.bias, A2=None if blk.atom else E, gather=plan.src32, n_rows=nE, plan=plan if in_grad else None)
    H = tau(H0)
    # (behind tau(H0) for every caller; the mol-atom-bond forward used to enqueue these two kernels in front of it: they depend on
    #  E alone, and the outputs are bit-identical)
    if blk.atom and blk.depth > 1 and nE:
        if torch.is_grad_enabled() and E.requires_grad:
            ME = gather_src_fn(plan, aggregate_fn(plan, E))                     # (the same two kernels, with their transposes)
        else:
            with torch.no_grad():
                ME = engine.gather_rows(engine.aggregate(plan, E), plan.src32)      # [E, d_e], constant over the loop
    # a batch without edges: the atom and the mol-atom-bond chains skip the W_h contraction, the bond block's runs it on no rows — each
    # as before.  (A backward pass through either form is refused on such a batch, by dmpnn_linear_wgrad: the recorded table holds that.)
    skip_empty = (blk.atom or blk.mab) and not nE
    rev = None
    for _ in range(1, blk.depth):
        if blk.undirected:
            if rev is None:
                rev = plan.rev64
            H = (H + H[rev]) / 2
        if skip_empty:
            H = drop(tau(H0))
        elif blk.atom:
            MH = gather_src_fn(plan, aggregate_fn(plan, H))
            H = drop(tau(linear_fn(MH, W_h.weight, W_h.bias, A2=ME, Cadd=H0)))
        else:
            H = drop(tau(linear_fn(message_fn(plan, H), W_h.weight, W_h.bias, Cadd=H0)))
    H_v = H_e = None
    if blk.want_v:
        Mv = aggregate_fn(plan, H)
        H_v = drop(tau(linear_fn(V, blk.W_o.weight, blk.W_o.bias, A2=Mv)))
        if V_d is not None and blk.W_d is not None:
            H_v = drop(linear_fn(H_v, blk.W_d.weight, blk.W_d.bias, A2=V_d))
    if blk.want_e:
        H_e = edge_readout(blk, linear_fn, E, H, E_d)
    return H_v, H_e
