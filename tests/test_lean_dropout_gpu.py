"""Block dropout inside the lean step kernels (``k_step16`` forward, ``k_bstep16`` backward, the finalize's mask launch): molecules
beyond the tile with ``engine.forward(..., keep=True, route="fused16", dropout=(p, seed))`` and the one-call step on top of it.

The reference is the restated forward (``tests/test_dropout_gpu.py``) in FLOAT64 with the hash masks of ``oracle/dropout_hash.py``
replayed: a stochastic op is compared given its mask.  The shapes are the smallest at which this code can go wrong — several 48-row
tiles with a partial last one, a plan whose row order is not the caller's edge order, padded and tail column blocks."""
import copy
import types

import numpy as np
import pytest
import torch
from torch import nn

from conftest import TOL, parity_err, parity_err_unfloored
from test_dropout_gpu import ReplayDropout, _restated_forward

pytestmark = pytest.mark.gpu

NAMES = (("W_i", "W_i", "weight"), ("b_i", "W_i", "bias"), ("W_h", "W_h", "weight"), ("b_h", "W_h", "bias"),
         ("W_o", "W_o", "weight"), ("b_o", "W_o", "bias"))


class RecordingTau(nn.Module):
    """tau of the reference, recording every pre-activation it sees (call order: H_0, the updates, finalize)."""

    def __init__(self, inner):
        super().__init__()
        self.inner, self.pre = inner, []

    def forward(self, z):
        self.pre.append(z.detach().clone())
        return self.inner(z)


class ReplayTau(nn.Module):
    """A ReLU-class activation with its 0 / 1 decisions fixed: z * (m + (1 - m) * slope)."""

    def __init__(self, pos, slope):
        super().__init__()
        self.f, self.i = [m.double() + (1.0 - m.double()) * slope for m in pos], 0

    def forward(self, z):
        f = self.f[self.i]
        self.i += 1
        assert f.shape == z.shape
        return z * f


def _slope(mp):
    return float(getattr(mp.tau, "negative_slope", 0.0))


def _engine_forward(mp, plan, bmg, drop, **kw):
    from chemprop_amd import engine

    W = lambda lin, n: getattr(getattr(mp, lin), n)
    act = {"ReLU": "relu", "LeakyReLU": "leakyrelu"}[type(mp.tau).__name__]
    return engine.forward(plan, bmg.V, bmg.E, W("W_i", "weight"), W("W_h", "weight"), W("W_o", "weight"), W("W_o", "bias"),
                          W("W_i", "bias"), W("W_h", "bias"), depth=mp.depth, act=act, slope=_slope(mp), keep=True, dropout=drop, **kw)


def _masks(seed, p, depth, nE, nV, d_h):
    """The hash masks (bool: kept) of the update sites — rows are the caller's edge ids — and of the finalize site (atom ids)."""
    from oracle import dropout_hash as dh

    return [torch.from_numpy(dh.keep_mask(seed, t, nE, d_h, p)) for t in range(depth - 1)] + [torch.from_numpy(dh.keep_mask(seed, depth - 1, nV, d_h, p))]


def _reference(cpu_bmg, mp_kw, state, p, keeps, tau_of):
    """The restated forward in float64 with the masks replayed; ``tau_of`` wraps the activation."""
    from chemprop_amd.nn import BondMessagePassing

    ref = BondMessagePassing(dropout=p, **mp_kw)
    ref.load_state_dict(state)
    ref = ref.double().train()
    ref.tau = tau_of(ref.tau)
    g = types.SimpleNamespace(V=cpu_bmg.V.double(), E=cpu_bmg.E.double(), edge_index=cpu_bmg.edge_index, rev_edge_index=cpu_bmg.rev_edge_index)
    masks = [k.double() / (1.0 - float(np.float32(p))) for k in keeps]
    return ref, _restated_forward(g, ref, ReplayDropout(p, masks))


CASES = [
    (8, "synth40", dict(d_h=64, depth=3), 0.25),
    (24, "zinc", dict(d_h=128, depth=4, activation="leakyrelu", bias=True), 0.4),
    (16, "cgr", dict(d_v=106, d_e=28, d_h=100, depth=2), 0.1),                     # columns padded to 128; one update site + the finalize site
    (12, "zinc", dict(d_h=300, depth=3), 0.5),                                     # five column blocks, a 12-column tail
]


@pytest.mark.parametrize("n_mols,kind,kw,p", CASES, ids=[f"{c[1]}-{c[0]}-h{c[2]['d_h']}" for c in CASES])
def test_lean_route_dropout_given_its_masks(n_mols, kind, kw, p, gpu_device):
    from chemprop_amd import engine, synth
    from chemprop_amd.nn import BondMessagePassing

    dev = gpu_device
    seed, seed2 = 0x1234_5678_9ABC_DEF, 77
    cpu_bmg = synth.random_batch(n_mols, kind, seed=11)
    torch.manual_seed(5)
    mp = BondMessagePassing(dropout=p, **kw)
    state = {k: v.clone() for k, v in mp.state_dict().items()}
    nV, nE, d_h, depth = int(cpu_bmg.V.shape[0]), int(cpu_bmg.E.shape[0]), kw["d_h"], mp.depth
    G = torch.randn(nV, d_h, generator=torch.Generator().manual_seed(6))
    mp = mp.to(dev).train()
    bmg = synth.random_batch(n_mols, kind, seed=11)
    bmg.to(dev)
    plan = engine.GraphPlan.from_bmg(bmg)
    inv = plan.inv32.long()
    assert nE > 2 * 48 and nE % 48 != 0                                            # several row tiles, a partial one
    assert not torch.equal(inv.cpu(), torch.arange(nE))                            # the plan's rows are NOT the caller's edges

    out, st = _engine_forward(mp, plan, bmg, (p, seed), route="fused16")
    assert st.route == "fused16/lean", st.route
    assert abs(float(st.args.dropout_p) - p) < 1e-7 and int(st.args.dropout_seed) == seed
    need = {k: True for k, _, _ in NAMES}
    g1 = engine.backward(st, G.to(dev), need)
    g1 = {k: (None if v is None else v.clone()) for k, v in g1.items()}
    g2 = engine.backward(st, G.to(dev), need)
    torch.cuda.synchronize()
    # 5. two backward passes on the same forward: bit-identical
    for k in g1:
        assert (g1[k] is None) == (g2[k] is None) and (g1[k] is None or torch.equal(g1[k], g2[k])), k
    # 6. the same seed again: bit-identical; another seed: another zero pattern
    again, _ = _engine_forward(mp, plan, bmg, (p, seed), route="fused16")
    other, _ = _engine_forward(mp, plan, bmg, (p, seed2), route="fused16")
    assert torch.equal(again, out)
    assert not torch.equal(other == 0, out == 0)

    keeps = _masks(seed, p, depth, nE, nV, d_h)
    out_c = out.detach().cpu()
    # 2. what the finalize zeroed is what the hash says; the kept fraction is the hash's own property
    fin = keeps[-1]
    assert bool((out_c[~fin] == 0).all())
    frac = float(fin.double().mean())
    assert abs(frac - (1 - p)) <= 5 * np.sqrt(p * (1 - p) / fin.numel()), (frac, 1 - p)

    # 1. the output against float64 given the masks
    ref, ref_out = _reference(cpu_bmg, kw, state, p, keeps, RecordingTau)
    err_out = parity_err(out_c.numpy(), ref_out.detach().numpy())
    pre = ref.tau.pre
    assert len(pre) == depth + 1
    # 3. the kept bits: the sign of tau(z) BEFORE dropout at every site (a dropped, positive element keeps bit 1)
    bits = engine.lean_sign_bits(st)[:, inv].cpu()                                 # [depth, n_edges, d_h], caller's edge order
    flips, dropped_pos = 0, 0
    for t in range(depth):
        z = pre[t]
        diff = (z > 0) != bits[t]
        flips += int(diff.sum())
        if diff.any():
            assert float(z[diff].abs().max()) <= 1e-5 * float(z.abs().max()), f"site {t}: a sign bit differs away from the kink"
        if t >= 1:
            sel = ~keeps[t - 1] & (z > 1e-5 * float(z.abs().max()))
            dropped_pos += int(sel.sum())
            assert bool(bits[t][sel].all()), f"site {t}: a dropped positive element lost its bit"
    assert flips <= 8, f"{flips} sign-bit disagreements"
    assert dropped_pos > 0
    print(f"lean-dropout {kind}-{n_mols}: output error {err_out:.3e}, sign-bit disagreements {flips}, dropped positive elements {dropped_pos}")
    assert err_out <= TOL, err_out

    # 4. every gradient against float64 autograd, the engine's activation decisions replayed: its bits at the edge sites; at the
    # finalize the sign of its output where the mask kept the entry, the reference's own decision where it did not (times 0 there)
    cond = [bits[t] for t in range(depth)] + [torch.where(fin, out_c > 0, pre[depth] > 0)]
    ref, ref_out = _reference(cpu_bmg, kw, state, p, keeps, lambda inner: ReplayTau(cond, _slope(mp)))
    (ref_out * G.double()).sum().backward()
    assert parity_err(out_c.numpy(), ref_out.detach().numpy()) <= TOL
    errs = {}
    for k, lin, n in NAMES:
        prm = getattr(getattr(ref, lin), n)
        if prm is None:
            assert g1[k] is None
            continue
        errs[k] = parity_err_unfloored(g1[k].cpu().numpy(), prm.grad.numpy())
    print(f"lean-dropout {kind}-{n_mols}: gradient errors given the masks {errs}")
    assert max(errs.values()) <= 2e-5, errs


def test_the_same_mask_on_the_tile_kernels_and_on_the_lean_route(gpu_device):
    from chemprop_amd import engine, synth
    from chemprop_amd.nn import BondMessagePassing

    dev, p, seed = gpu_device, 0.3, 424242
    torch.manual_seed(8)
    mp = BondMessagePassing(d_h=64, dropout=p).to(dev).train()
    bmg = synth.random_batch(64, "qm9", seed=12)
    bmg.to(dev)
    plan = engine.GraphPlan.from_bmg(bmg)
    tile, st_t = _engine_forward(mp, plan, bmg, (p, seed))
    lean, st_l = _engine_forward(mp, plan, bmg, (p, seed), route="fused16")
    assert st_t.route == "mega16" and st_l.route == "fused16/lean", (st_t.route, st_l.route)
    assert float(st_t.args.dropout_p) == float(st_l.args.dropout_p) > 0
    err = parity_err(lean.cpu().numpy(), tile.cpu().numpy())
    differ = float(((lean == 0) != (tile == 0)).float().mean())
    print(f"tile kernels against the lean route, one seed: output difference {err:.3e}, zero patterns differ in {differ:.3e} of the entries")
    assert err <= TOL
    assert differ < 1e-4


def _model(dev, **mp_kw):
    from chemprop_amd import agg as cagg
    from chemprop_amd.model import MPNN, RegressionFFN
    from chemprop_amd.nn import BondMessagePassing

    d_h = mp_kw.get("d_h", 64)
    return MPNN(BondMessagePassing(dropout=0.2, **mp_kw), cagg.MeanAggregation(), RegressionFFN(input_dim=d_h)).to(dev).train()


def _zinc_batch(dev):
    from chemprop_amd import synth

    bmg = synth.random_batch(24, "zinc", seed=13)
    # targets the graph determines: a fixed readout of every molecule's mean atom features, standardised
    coef = torch.randn(bmg.V.shape[1], 1, generator=torch.Generator().manual_seed(14))
    n = len(bmg)
    m = torch.zeros(n, bmg.V.shape[1]).index_add(0, bmg.batch, bmg.V) / torch.bincount(bmg.batch, minlength=n).view(-1, 1)
    y = m @ coef
    y = (y - y.mean()) / y.std()
    bmg.to(dev)
    return bmg, y.to(dev)


def test_fused_trainer_takes_the_lean_route_for_block_dropout_beyond_the_tile(gpu_device):
    from chemprop_amd import engine
    from chemprop_amd.model import FusedTrainer
    from head_harness import run_head

    dev = gpu_device
    torch.manual_seed(21)
    model = _model(dev, d_h=64)
    bmg, y = _zinc_batch(dev)
    before = copy.deepcopy(model)
    tr = FusedTrainer(model, lr=1e-3)
    torch.manual_seed(99)
    first = int(torch.randint(0, 2 ** 62, (1,), dtype=torch.int64).item())
    torch.manual_seed(99)
    loss = tr.step(bmg, y)
    torch.cuda.synchronize()
    assert str(tr.last_route).startswith("fused16/lean"), tr.last_route
    assert tr.last_dropout_seed == first
    step_grads = {id(p): tr._views[id(p)].detach().clone() for p in model.message_passing.parameters()}

    # the same step by hand on the parameters before it: engine.forward for that seed, the head on its output, engine.backward on gH_v
    mp = before.message_passing
    plan = engine.GraphPlan.from_bmg(bmg)
    out, st = _engine_forward(mp, plan, bmg, (0.2, first), route="fused16")
    assert st.route == "fused16/lean"
    head_loss, _, _, gH = run_head(before, out, bmg.batch, len(bmg), y, None, None, None)
    assert abs(float(loss[0]) - head_loss) <= 1e-6 * abs(head_loss), (float(loss[0]), head_loss)
    grads = engine.backward(st, gH.to(dev), {k: True for k, _, _ in NAMES})
    torch.cuda.synchronize()
    named = dict(model.message_passing.named_parameters())
    assert len(named) == len(step_grads)
    for k, lin, n in NAMES:
        p_new = named.get(f"{lin}.{n}")
        if p_new is None:
            assert grads[k] is None
            continue
        assert torch.equal(grads[k], step_grads[id(p_new)]), f"{k}: the step's gradient is not engine.backward's, bit for bit"


def test_fused_trainer_learns_with_block_dropout_beyond_the_tile(gpu_device):
    from chemprop_amd.model import FusedTrainer

    dev = gpu_device
    torch.manual_seed(22)
    model = _model(dev, d_h=64)
    bmg, y = _zinc_batch(dev)
    tr = FusedTrainer(model, lr=3e-3)
    losses = [float(tr.step(bmg, y)[0]) for _ in range(60)]
    assert str(tr.last_route).startswith("fused16/lean"), tr.last_route
    print(f"lean-dropout trainer: first five losses {losses[:5]}, last five {losses[-5:]}")
    assert np.mean(losses[-5:]) < 0.7 * np.mean(losses[:5]), (losses[:5], losses[-5:])


def test_fused_trainer_eval_draws_no_seed_and_other_blocks_are_still_refused(gpu_device):
    from chemprop_amd.model import FusedTrainer

    dev = gpu_device
    torch.manual_seed(23)
    model = _model(dev, d_h=64)
    bmg, y = _zinc_batch(dev)
    tr = FusedTrainer(model, lr=1e-3)
    # .eval(): the block's argument blocks carry no dropout and no seed is drawn (the step itself refuses an eval model)
    model.eval()
    rng = torch.get_rng_state()
    part = tr._block_args(tr.mp, bmg, len(bmg), tr.acts[0], False, None, None)
    assert float(part.st.args.dropout_p) == 0.0 and torch.equal(torch.get_rng_state(), rng)
    assert not hasattr(tr, "last_dropout_seed") or tr.last_dropout_seed is None
    with pytest.raises(RuntimeError, match="eval mode"):
        tr.step(bmg, y)
    model.train()
    # a smooth activation, a block wider than the step kernels' 320 columns: refused as before, the reason named
    for kw, match in ((dict(d_h=64, activation="tanh"), None), (dict(d_h=400), "320")):
        torch.manual_seed(24)
        with pytest.raises(NotImplementedError, match=match):                      # (at construction — fused_block — or by the step)
            FusedTrainer(_model(dev, **kw), lr=1e-3).step(bmg, y)


def test_the_default_route_still_refuses_dropout_beyond_the_tile(gpu_device):
    """The lean form with dropout is a DEMAND (``route="fused16"``).  From 20 000 directed edges on the route rule itself picks the lean
    form for a keeping forward — it is asked with p = 0 — and a default-route forward with ``dropout=`` must then refuse as it always
    did, so that the module path under autograd keeps its own ``nn.Dropout`` between the row kernels at every edge count."""
    from chemprop_amd import engine, synth
    from chemprop_amd.nn import _VALIDATE_FIRST_N, BondMessagePassing

    dev = gpu_device
    torch.manual_seed(31)
    mp = BondMessagePassing(d_h=64, dropout=0.2).to(dev).train()
    bmg = synth.random_batch(512, "zinc", seed=15)
    bmg.to(dev)
    assert int(bmg.E.shape[0]) >= 20000
    plan = engine.GraphPlan.from_bmg(bmg)
    _, st = _engine_forward(mp, plan, bmg, None, max_level=1)
    assert st.route == "fused16/lean" and float(st.args.dropout_p) == 0.0          # (the rule's choice without dropout)
    with pytest.raises(engine.RouteUnavailable):
        _engine_forward(mp, plan, bmg, (0.2, 5), max_level=1)
    # the module path: through the validation window and beyond it, no forward carries dropout inside the kernels
    for _ in range(_VALIDATE_FIRST_N + 2):
        mp.zero_grad()
        out = mp(bmg)
        assert not hasattr(out.grad_fn, "st") or float(out.grad_fn.st.args.dropout_p) == 0.0
        out.sum().backward()
        assert all(torch.isfinite(q.grad).all() for q in mp.parameters())
    assert bool((out.detach() == 0).float().mean() > 0.15)                         # (nn.Dropout was applied: p = 0.2 of the finalize output)
