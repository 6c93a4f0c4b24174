"""Shared helpers of the atom-message tests (``tests/test_atom_edge_kernels.py``, ``tests/test_atom_general_route.py``,
``tests/test_atom_step.py``, ``tests/test_atom_tile_boundaries.py``): no fixtures, no pytest settings — a plain module.

* ``atom_message_ref`` / ``atom_message_seq32`` / ``atom_message_bwd_ref``: the atom message ``M[e] = sum_{e': dst e' = src e} X[e']``
  (mixins.py:21-30) in float64 / float32, as the float32 sum in increasing edge id the kernel forms (bit for bit), and its transpose
  by autograd.
* ``run_atom_message_fwd`` / ``run_atom_message_bwd``: ``dmpnn_message_fwd(flags = DMPNN_F_ATOM)`` and ``dmpnn_atom_message_bwd``
  through ctypes on ``rows_harness.Mat`` buffers (NaN padding, guard regions).
* ``mixed_batch``: a single-atom molecule, QM9-shaped ones and one 40-atom molecule in one batch, at any ``d_v`` / ``d_e``.
* ``block_weights`` / ``block_ref``: an atom block's parameters and its restatement (base.py:196-212 with the atom mixin) in any
  dtype — with the biases, any activation of ``lean_harness.ENGINE_ACT``, fixed ReLU-class decisions and dropout keep masks — equal to ``oracle.dmpnn_torch.atom_forward``
  where that applies (checked by the CPU tests).
* ``compare``: ``rows_harness.compare`` (``err <= min(MARGIN max(e32, 2**-23), cap)``) returning the worst ratio as well.
"""
import numpy as np
import torch

import rows_harness as rh
from chemprop_amd import _lib
from conftest import parity_err_unfloored
from oracle import dmpnn_torch as ot

EPS32 = rh.EPS32
PARAMS = ("W_i", "b_i", "W_h", "b_h", "W_o", "b_o")


# ---- the edge kernels ----------------------------------------------------------------------------------------------------------------
def atom_message_ref(bmg, X, dtype=torch.float64):
    src, dst = bmg.edge_index
    return ot.segment_sum_dst(X.to(dtype), dst, int(bmg.V.shape[0]))[src]


def atom_message_seq32(bmg, X):
    """The float32 sum of the incoming rows of ``src(e)`` in increasing edge id, ``((r1 + r2) + r3) ...``: what the kernel forms."""
    src, dst = bmg.edge_index
    nV, nE = int(bmg.V.shape[0]), int(dst.numel())
    X = X.float()
    S = torch.zeros(nV, X.shape[1])
    seen = torch.zeros(nV, dtype=torch.bool)
    order = torch.sort(dst, stable=True).indices                    # by destination, increasing edge id within one
    d_sorted = dst[order]
    rank = torch.arange(nE) - torch.searchsorted(d_sorted, d_sorted)   # position among the incoming edges of its atom
    for k in range(int(rank.max()) + 1 if nE else 0):
        e = order[rank == k]
        v = dst[e]
        S[v] = torch.where(seen[v].view(-1, 1), S[v] + X[e], X[e])
        seen[v] = True
    return S[src]


def atom_message_bwd_ref(bmg, gM, dtype=torch.float64):
    """``gX[e'] = sum_{e: src e = dst e'} gM[e]``: the transpose of ``atom_message_ref`` by autograd in ``dtype``."""
    X = torch.zeros(gM.shape, dtype=dtype, requires_grad=True)
    atom_message_ref(bmg, X, dtype).backward(gM.to(dtype))
    return X.grad


def atom_message_literal(src, dst, X, n_atoms, dtype=torch.float64):
    """The literal edge form on ANY index arrays: ``M[e] = S[src e]``, ``S[v] = sum_{dst e' = v} X[e']``."""
    S = torch.zeros(n_atoms, X.shape[1], dtype=dtype).index_add_(0, dst, X.to(dtype))
    return S[src]


def run_atom_message_fwd(dev, plan, X, flags=None, ld_in=None, ld_out=None):
    lib = _lib.load()
    h = int(X.shape[1])
    mi = rh.Mat(dev, int(X.shape[0]), h, ld_in, 0, X)
    mo = rh.Mat(dev, plan.n_edges, h, ld_out, 0)
    rc, msg, _ = rh._call(dev, lib.dmpnn_message_fwd, plan.buf.data_ptr(), plan.n_atoms, plan.n_edges, h, mi.ptr, mi.ld, mo.ptr, mo.ld,
                          _lib.ACT["none"], 0.0, None, _lib.F_ATOM if flags is None else flags)
    return rc, msg, mo


def run_atom_message_bwd(dev, plan, gM, ld_in=None, ld_out=None):
    lib = _lib.load()
    h = int(gM.shape[1])
    mi = rh.Mat(dev, int(gM.shape[0]), h, ld_in, 0, gM)
    mo = rh.Mat(dev, plan.n_edges, h, ld_out, 0)
    rc, msg, _ = rh._call(dev, lib.dmpnn_atom_message_bwd, plan.buf.data_ptr(), plan.n_atoms, plan.n_edges, h, mi.ptr, mi.ld, mo.ptr, mo.ld)
    return rc, msg, mo


# ---- batches -------------------------------------------------------------------------------------------------------------------------
def mixed_batch(d_v=72, d_e=14, seed=0, n_qm9=6, big=40):
    """One single-atom molecule, ``n_qm9`` QM9-shaped ones and (``big``) one molecule of that many atoms, beyond the tile."""
    from chemprop_amd import synth
    from chemprop_amd.data import BatchMolGraph

    rng = np.random.default_rng(1000 + seed)
    mols = [synth.random_molgraph(rng, d_v=d_v, d_e=d_e, n_atoms=1)]
    mols += [synth.random_molgraph(rng, 9.0, d_v, d_e) for _ in range(n_qm9)]
    if big:
        mols.insert(3, synth.random_molgraph(rng, d_v=d_v, d_e=d_e, n_atoms=big))
    return BatchMolGraph(mols)


def on_device(bmg, dev):
    b = bmg.__copy__()
    b.to(dev)
    return b


# ---- the block -----------------------------------------------------------------------------------------------------------------------
def block_weights(d_v, d_e, d_h, bias, seed=0):
    """float32 CPU parameters of an atom block in ``nn.Linear``'s initialisation range (``None`` for a missing bias)."""
    gen = torch.Generator().manual_seed(77 + seed)
    u = lambda n, k: (2 * torch.rand(n, k, generator=gen) - 1) / k ** 0.5
    w = dict(W_i=u(d_h, d_v), W_h=u(d_h, d_h + d_e), W_o=u(d_h, d_v + d_h))
    w["b_o"] = ((2 * torch.rand(d_h, generator=gen) - 1) / (d_v + d_h) ** 0.5)
    w["b_i"] = ((2 * torch.rand(d_h, generator=gen) - 1) / d_v ** 0.5) if bias else None
    w["b_h"] = ((2 * torch.rand(d_h, generator=gen) - 1) / (d_h + d_e) ** 0.5) if bias else None
    return w


def scale32(p):
    """The kernels' ``1.f / (1.f - p)`` as a Python float."""
    return float(np.float32(1.0) / (np.float32(1.0) - np.float32(p)))


RELU_SLOPE = dict(relu=0.0, leakyrelu=0.1)   # the ReLU class: the factor of a negative entry (leakyrelu: ``lean_harness.LEAKY_SLOPE``)


def block_ref(bmg, w, depth, act, dtype=torch.float64, decisions=None, keeps=None, p=0.0, leaves=False):
    """base.py:196-212 with the atom mixin (mixins.py:21-30) in ``dtype`` on the CPU.  ``act``: the names of ``lean_harness.ENGINE_ACT``
    — relu | leakyrelu (slope 0.1) | identity (LeakyReLU with slope 1) | tanh | elu.  ``decisions`` (the ReLU class): one bool
    tensor per activation site (H0, the updates, the finalize) that replaces the activation by a fixed factor, 1 or the slope.  ``keeps``: the dropout
    keep masks of the update sites and the finalize (``oracle.dropout_hash.keep_mask``), applied with the kernels' float scale.
    Returns ``(out, leaves, pre, made)``: the parameters as leaves with autograd, every pre-activation, every decision made.
    ``leaves``: ``w`` already holds the leaves in ``dtype`` (a training loop's own parameters)."""
    f = lambda t: None if t is None else t.detach().to(dtype).requires_grad_(True)
    L = {k: w.get(k) for k in PARAMS} if leaves else {k: f(w[k]) for k in PARAMS}
    V, E = bmg.V.to(dtype), bmg.E.to(dtype)
    src, dst = bmg.edge_index
    nV = int(V.shape[0])
    pre, made = [], []

    def tau(z):
        pre.append(z.detach())
        if act == "tanh":
            return torch.tanh(z)
        if act == "elu":
            return torch.nn.functional.elu(z)
        if act == "identity":          # (the engine's LeakyReLU with slope 1: either decision gives the factor 1)
            return z
        assert act in RELU_SLOPE, act
        m = (z.detach() > 0) if decisions is None else decisions[len(made)]
        made.append(m)
        if act == "relu":
            return z * m.to(dtype)
        f = m.to(dtype)
        return z * (f + (1 - f) * RELU_SLOPE[act])

    site = [0]

    def drop(x):
        if keeps is None:
            return x
        k = keeps[site[0]]
        site[0] += 1
        return x * (k.to(dtype) * scale32(p))

    lin = torch.nn.functional.linear
    H0 = lin(V[src], L["W_i"], L["b_i"])
    H = tau(H0)
    ME = ot.segment_sum_dst(E, dst, nV)[src]                        # (constant over the depth loop)
    for _ in range(1, depth):
        M = torch.cat((ot.segment_sum_dst(H, dst, nV)[src], ME), 1)
        H = drop(tau(H0 + lin(M, L["W_h"], L["b_h"])))
    Mv = ot.segment_sum_dst(H, dst, nV)
    out = drop(tau(lin(torch.cat((V, Mv), 1), L["W_o"], L["b_o"])))
    return out, L, pre, made


def block_grads(out, L, G):
    """Parameter gradients of ``sum(out * G)`` by autograd (``None``: no such parameter; zeros: it took no part)."""
    (out * G.to(out.dtype)).sum().backward()
    return {k: (None if L[k] is None else (torch.zeros_like(L[k]) if L[k].grad is None else L[k].grad)) for k in PARAMS}


def named(out, grads, d_h):
    """The tensors a case compares: the output, every present gradient, and the two column blocks of ``gW_h`` on their own."""
    t = dict(out=out.detach())
    for k, g in grads.items():
        if g is not None:
            t["g" + k] = g.detach()
    t["gW_h[:, :d_h]"], t["gW_h[:, d_h:]"] = t["gW_h"][:, :d_h], t["gW_h"][:, d_h:]
    return t


def train_ref(model, bmg, y, steps, dtype, lr, eps, keeps_of=None, p=0.0):
    """``steps`` training steps of ``model`` (an atom block, sum / norm aggregation, ``BatchNorm1d``, an MLP predictor, MSE) restated
    on the CPU in ``dtype`` from the model's current parameters, with ``torch.optim.Adam``: ``block_ref``, the aggregation, the batch
    norm on batch statistics, the predictor's layers, ``masked_loss``.  ``keeps_of(i)``: the dropout keep masks of step ``i``.
    Returns ``(losses, {parameter name: value after the last step})`` — in float32 the yardstick of the float64 run."""
    from chemprop_amd.model import masked_loss

    P = {k: v.detach().cpu().to(dtype).clone().requires_grad_(True) for k, v in model.named_parameters()}
    opt = torch.optim.Adam(list(P.values()), lr=lr, eps=eps)
    mp = model.message_passing
    act = {"ReLU": "relu", "Tanh": "tanh"}[type(mp.tau).__name__]
    n = int(y.shape[0])
    losses = []
    for i in range(steps):
        w = {k: P.get(f"message_passing.{lin}.{nm}") for k, lin, nm in (("W_i", "W_i", "weight"), ("b_i", "W_i", "bias"), ("W_h", "W_h", "weight"),
                                                                       ("b_h", "W_h", "bias"), ("W_o", "W_o", "weight"), ("b_o", "W_o", "bias"))}
        Hv = block_ref(bmg, w, mp.depth, act, dtype, keeps=None if keeps_of is None else keeps_of(i), p=p, leaves=True)[0]
        Z = torch.zeros(n, Hv.shape[1], dtype=dtype).index_add(0, bmg.batch, Hv) / float(model.agg.norm)
        Z = torch.nn.functional.batch_norm(Z, None, None, P["bn.weight"], P["bn.bias"], training=True, eps=model.bn.eps)
        for bi, blk in enumerate(model.predictor.ffn):
            for li, layer in enumerate(blk):
                if isinstance(layer, torch.nn.Linear):
                    Z = torch.nn.functional.linear(Z, P[f"predictor.ffn.{bi}.{li}.weight"], P.get(f"predictor.ffn.{bi}.{li}.bias"))
                elif not isinstance(layer, torch.nn.Dropout):
                    Z = layer(Z)
        loss = masked_loss(Z, y.to(dtype), None, None, None, None, "mse")
        opt.zero_grad()
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    return losses, {k: v.detach() for k, v in P.items()}


def yardstick(ref64: dict, ref32: dict) -> dict:
    return {k: parity_err_unfloored(ref32[k].double().numpy(), ref64[k].double().numpy()) for k in ref64}


def kinds(tensors) -> dict:
    return {k: ("fwd" if k == "out" else "grad") for k in tensors}


def compare(case_id, got, ref, e32, margin, report=print):
    """``rows_harness.compare`` per tensor, plus the worst ``err / max(e32, 2**-23)`` of the case (reported, for the module's MARGIN)."""
    worst = [0.0]

    def rep(line):
        report(line.replace("ROWSBAR", "ATOMBAR"))
        if "ratio=" in line:
            worst[0] = max(worst[0], float(line.split("ratio=")[1].split()[0]))

    fails = rh.compare(case_id, got, ref, e32, kinds(got), margin=margin, report=rep)
    return fails, worst[0]
