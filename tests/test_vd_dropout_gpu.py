"""Block dropout behind the atom-descriptor layer on the GPU: the mask site inside ``k_vd_gemm`` (``dmpnn_vd_args.dropout_p``, site
``DMPNN_DROP_SITE_VD``) through the C ABI, then through ``FusedTrainer(..., vd_dropout=True)`` on each of the block's three dropout
homes, the staged step and ``HipMPNN``.

A stochastic op is compared GIVEN its mask: the masks are ``oracle/dropout_hash.py``'s restatement of the kernels' hash for the seed the
step drew, replayed in the reference (``ReplayDropout``)."""
import copy
import ctypes as C
import functools
import types

import numpy as np
import pytest
import torch

from chemprop_amd import _lib
from conftest import parity_err
from oracle.dropout_hash import keep_mask
from test_dropout_gpu import ReplayDropout
from test_head_boundaries import MARGIN
from test_lean_dropout_gpu import RecordingTau, ReplayTau
from test_multicomponent_integration import stub_chemprop  # noqa: F401  (the fixture)
from vd_harness import OUTPUTS, VdCase, build_inputs, compare, reference, vd_args
from conftest import parity_err_unfloored

pytestmark = pytest.mark.gpu

SITE = 0x8000   # (DMPNN_DROP_SITE_VD; pinned against the library in tests/test_vd_dropout.py)
SEED, SEED2 = 0x0123_4567_89AB_CDEF, 77


def _scale32(p) -> np.float32:
    """The kernels' scale: the float ``1.f / (1.f - p)``."""
    return np.float32(1) / (np.float32(1) - np.float32(p))


# ---- 1. the stage against float64, given the mask -------------------------------------------------------------------------------------
# (n, d_h, d_vd): one atom; a full and a one-row partial 32-row tile; the widest layer (544 columns); odd everything at the f16
# weight-gradient product's first row count; the timed shape.  pad and p dealt over them; one case without gW_d / gb_d.
STAGE = [
    (VdCase(1, 4, 1, pad=0, seed=1), 0.1),
    (VdCase(33, 64, 3, pad=1, seed=2), 0.5),
    (VdCase(47, 300, 20, pad=5, seed=3), 0.1),
    (VdCase(64, 343, 201, pad=0, seed=4), 0.5),
    (VdCase(1025, 31, 7, pad=1, seed=5), 0.1),
    (VdCase(4636, 300, 50, pad=5, seed=6), 0.5),
    (VdCase(47, 300, 20, pad=1, want_gW=False, want_gb=False, seed=7), 0.5),
]


@functools.lru_cache(maxsize=None)
def _stage_reference(case: VdCase, p: float):
    """Inputs, mask and the float64 restatement with the mask on ``out`` and on its gradient (+ the float32 yardstick): computed once
    per case, shared, never written."""
    inp = build_inputs(case)
    n, D = case.n_atoms, case.d_h + case.d_vd
    keep = torch.from_numpy(keep_mask(SEED, SITE, n, D, p))
    s32 = _scale32(p)

    def restate(dtype):
        g = torch.where(keep, inp["gout"].to(dtype) * float(s32), torch.zeros((), dtype=dtype))
        r = reference(case, dict(inp, gout=g), dtype)
        r["out"] = torch.where(keep, r["out"] * float(s32), torch.zeros((), dtype=dtype))
        return r

    r64, r32 = restate(torch.float64), restate(torch.float32)
    e32 = {k: parity_err_unfloored(r32[k].double().numpy(), r64[k].numpy()) for k in OUTPUTS}
    return inp, keep, r64, e32


def _run_stage(case, inp, dev, p, seed, backward=True):
    """One ``dmpnn_vd_forward`` (+ one ``dmpnn_vd_backward``) with ``dropout_p`` / ``dropout_seed`` set, outputs NaN-prefilled
    (``vd_harness.vd_args``); returns the tensors by name, on the CPU."""
    from chemprop_amd import engine

    lib = _lib.load()
    a, t = vd_args(case, inp, dev)
    a.dropout_p, a.dropout_seed = p, seed
    with engine._OnDevice(dev):
        _lib.check(lib.dmpnn_vd_forward(C.byref(a), engine._stream_ptr(dev)), "dmpnn_vd_forward")
        if backward:
            t["ws"].fill_(0xFF)   # (nothing of the forward's workspace may be relied on)
            _lib.check(lib.dmpnn_vd_backward(C.byref(a), engine._stream_ptr(dev)), "dmpnn_vd_backward")
    torch.cuda.synchronize()
    return {k: t[k].cpu() for k in OUTPUTS + ("gout",)}


def _bits(x):
    return x.contiguous().view(torch.int32)


@pytest.mark.parametrize("case,p", STAGE, ids=[f"{c.id}-p{p}" for c, p in STAGE])
def test_stage_with_dropout_against_float64_given_the_mask(case, p, gpu_device):
    inp, keep, r64, e32 = _stage_reference(case, p)
    s32 = torch.tensor(_scale32(p))
    plain = _run_stage(case, inp, gpu_device, 0.0, 0, backward=False)
    got = _run_stage(case, inp, gpu_device, p, SEED)
    again = _run_stage(case, inp, gpu_device, p, SEED)
    # forward: a dropped entry is +0.0; a kept entry is the p = 0 value times the float scale — bit for bit
    assert bool((_bits(got["out"])[~keep] == 0).all()), "a dropped entry of out is not +0.0"
    assert torch.equal(_bits(got["out"])[keep], _bits(plain["out"] * s32)[keep]), "a kept entry of out is not the p = 0 value times the scale"
    # the same seed twice: bit-identical; another seed: another zero pattern
    for k in OUTPUTS + ("gout",):
        assert torch.equal(_bits(got[k]), _bits(again[k])), k
    if keep.numel() >= 64:
        other = _run_stage(case, inp, gpu_device, p, SEED2, backward=False)
        assert not torch.equal(other["out"] == 0, got["out"] == 0)
    # backward: gout leaves as the masked gradient, bit for bit (also when no weight gradient is asked for)
    want_g = torch.where(keep, inp["gout"] * s32, torch.zeros(()))
    assert torch.equal(_bits(got["gout"]), _bits(want_g)), "gout is not where(keep, gout * scale, +0.0) after the backward call"
    # out and the gradients against float64 with the mask applied to out and to its gradient
    fails, worst = compare(case, got, r64, e32, MARGIN)
    print(f"VDWORST {case.id} p={p} ratio={worst:.2f}")
    assert not fails, (case.id, p, fails)


def test_stage_with_p_zero_is_the_old_call_whatever_the_seed(gpu_device):
    """The grown struct with ``dropout_p = 0`` and a non-zero seed: ``out`` and every gradient bit-identical to seed 0, ``gout`` untouched."""
    case = VdCase(1025, 31, 7, pad=1, seed=5)
    inp = build_inputs(case)
    zero = _run_stage(case, inp, gpu_device, 0.0, 0)
    seeded = _run_stage(case, inp, gpu_device, 0.0, SEED)
    for k in OUTPUTS:
        assert torch.equal(_bits(zero[k]), _bits(seeded[k])), k
        assert bool(torch.isfinite(seeded[k]).all()), k
    for r in (zero, seeded):
        assert torch.equal(_bits(r["gout"]), _bits(inp["gout"]))
    assert not bool((seeded["out"] == 0).any())


# ---- 2. the one-call step against the module path, given the masks --------------------------------------------------------------------
P = 0.2


def make_model(d_vd, d_h, act, dropout=P):
    """``tests/test_atom_descriptors.py::make_model`` with dropout inside the block."""
    from chemprop_amd import agg as cagg
    from chemprop_amd.model import MPNN, MSE, RegressionFFN
    from chemprop_amd.nn import BondMessagePassing

    mp = BondMessagePassing(d_h=d_h, depth=3, activation=act, d_vd=d_vd, dropout=dropout)
    pred = RegressionFFN(n_tasks=1, input_dim=mp.output_dim, hidden_dim=300, n_layers=1, activation=act, criterion=MSE(1.0))
    return MPNN(mp, cagg.NormAggregation(), pred, batch_norm=True)


def step_inputs(n_mols, kind, d_vd, d_h, act, dev, seed=11):
    from chemprop_amd import synth

    torch.manual_seed(seed)
    a = make_model(d_vd, d_h, act)
    b = copy.deepcopy(a)
    a, b = a.to(dev).train(), b.to(dev).train()
    bmg = synth.random_batch(n_mols, kind, seed=seed + 1)
    bmg.to(dev)
    gen = torch.Generator().manual_seed(seed + 2)
    y = torch.randn(n_mols, 1, generator=gen).to(dev)
    w = (0.5 + torch.rand(n_mols, 1, generator=gen)).to(dev)
    V = torch.randn(int(bmg.V.shape[0]), d_vd, generator=gen).to(dev)
    return a, b, bmg, y, w, V


def _spy(tr):
    """Keep what the step builds: the block's part (plan, kept forward state, ``H_v``) and the stage's argument block."""
    seen = {}
    block_args, vd_args_ = tr._block_args, tr._vd_args

    def block(*a, **kw):
        seen["part"] = block_args(*a, **kw)
        return seen["part"]

    def vd(*a, **kw):
        r = vd_args_(*a, **kw)
        seen["vd"] = r[2]
        return r

    tr._block_args, tr._vd_args = block, vd
    return seen


def _masks(seed, p, depth, nE, nV, d_h, d_vd, dev):
    """The four kinds of site in the reference's call order, as float multipliers ``keep * scale``: the update steps (rows: the
    caller's edge ids, which is the order of the module path's edge rows), finalize (atoms), and last the site behind ``W_d``."""
    s = _scale32(p)
    sites = [(t, nE, d_h) for t in range(depth - 1)] + [(depth - 1, nV, d_h), (SITE, nV, d_h + d_vd)]
    keeps = [torch.from_numpy(keep_mask(seed, site, n, d, p)).to(dev) for site, n, d in sites]
    return keeps, [k.float() * float(s) for k in keeps]


def _engine_decisions(part, keeps, pre, d_h, depth):
    """The 0 / 1 decisions of a ReLU-class activation the fused step took, per site (H_0, the updates, finalize), in the caller's edge
    order: the lean step kernels keep them as sign bits BEFORE dropout; the tile kernels keep the post-dropout tensors, whose sign
    says it where the mask kept the entry — elsewhere (the entry is multiplied by 0) the reference's own decision stands."""
    from chemprop_amd import engine

    st, out = part.st, part.out[:, :d_h]
    if st.route.startswith("fused16/lean"):
        bits = engine.lean_sign_bits(st)[:, part.plan.inv32.long()]
        cond = [bits[t] for t in range(depth)]
    else:
        assert st.route == "mega16" and part.plan.tiles_only, st.route   # (kept tensors in the caller's edge order)
        cond = [st.H0[:, :d_h] > 0] + [torch.where(keeps[t], st.Hs[t][:, :d_h] > 0, pre[t + 1] > 0) for t in range(depth - 1)]
    cond.append(torch.where(keeps[depth - 1], out > 0, pre[depth] > 0))
    flips = 0
    for t in range(depth + 1):
        diff = cond[t] != (pre[t] > 0)
        flips += int(diff.sum())
        if diff.any():
            assert float(pre[t][diff].abs().max()) <= 1e-5 * max(1.0, float(pre[t].abs().max())), f"site {t}: a decision differs away from the kink"
    return cond, flips


HOMES = {
    "tile": dict(n_mols=64, kind="qm9", d_h=64, act="relu", d_vd=3),
    "lean": dict(n_mols=32, kind="zinc", d_h=64, act="relu", d_vd=20),
    "rows": dict(n_mols=32, kind="zinc", d_h=64, act="elu", d_vd=8, rows_dropout=True),
    "tile-frozen-W_d": dict(n_mols=64, kind="qm9", d_h=64, act="relu", d_vd=3, frozen=True),
}


def _assert_home(name, tr):
    if name.startswith("tile"):
        assert str(tr.last_route).startswith("mega16") and tr._last_plan_tiles, (tr.last_route, tr._last_plan_tiles)
    elif name == "lean":
        assert str(tr.last_route).startswith("fused16/lean"), tr.last_route
    else:
        assert tr.last_route == "general16", tr.last_route


@pytest.mark.parametrize("name", list(HOMES))
def test_fused_step_with_vd_dropout_equals_module_path_given_the_masks(name, gpu_device, monkeypatch):
    """``FusedTrainer(vd_dropout=True).step(bmg, y, w, V_d=V)`` three times against the module path run op by op on a copy whose
    block's dropout replays the hash masks of the seed each step drew — the update sites, finalize, and LAST the site behind ``W_d``
    — and, for a ReLU-class block, whose activation replays the decisions the kernels took.  No entry is left out."""
    from chemprop_amd.model import FusedTrainer, masked_loss

    monkeypatch.setenv("DMPNN_VALIDATE", "never")
    kw = dict(HOMES[name])
    frozen, rows = kw.pop("frozen", False), kw.pop("rows_dropout", False)
    dev = gpu_device
    a, b, bmg, y, w, V = step_inputs(dev=dev, **kw)
    if frozen:
        for m in (a, b):
            m.message_passing.W_d.requires_grad_(False)
    with pytest.raises(NotImplementedError, match="W_d"):   # (the default still refuses the block)
        FusedTrainer(copy.deepcopy(a), lr=1e-3, eps=1e-4, rows_dropout=rows)
    mp_b = b.message_passing
    depth, d_h, d_vd = int(mp_b.depth), kw["d_h"], kw["d_vd"]
    nV, nE = int(bmg.V.shape[0]), int(bmg.E.shape[0])
    relu = kw["act"] == "relu"
    tau_b = mp_b.tau
    w_d0 = a.message_passing.W_d.weight.detach().clone()
    tr = FusedTrainer(a, lr=1e-3, eps=1e-4, rows_dropout=rows, vd_dropout=True)
    seen = _spy(tr)
    opt = torch.optim.Adam([p for p in b.parameters() if p.requires_grad], lr=1e-3, eps=1e-4)
    seeds = []
    for s in range(3):
        la = float(tr.step(bmg, y, w, V_d=V)[0])
        _assert_home(name, tr)
        seed = int(tr.last_dropout_seed)
        seeds.append(seed)
        vd = seen["vd"]
        assert abs(float(vd.dropout_p) - P) < 1e-7 and int(vd.dropout_seed) == seed
        assert float(seen["part"].st.args.dropout_p) == float(vd.dropout_p) and int(seen["part"].st.args.dropout_seed) == seed
        keeps, masks = _masks(seed, P, depth, nE, nV, d_h, d_vd, dev)
        if relu:
            mp_b.tau, mp_b.dropout = RecordingTau(tau_b), ReplayDropout(P, masks)
            with torch.no_grad():
                mp_b(bmg, V)
            pre = mp_b.tau.pre
            assert len(pre) == depth + 1
            cond, flips = _engine_decisions(seen["part"], keeps, pre, d_h, depth)
            print(f"VDDROP {name} step {s}: {flips} activation decisions differ from the module path's own")
            mp_b.tau = ReplayTau(cond, 0.0)
            mp_b.tau.f = [f.float() for f in mp_b.tau.f]
        mp_b.dropout = ReplayDropout(P, masks)
        opt.zero_grad()
        lb = masked_loss(b.predictor.train_step(b.fingerprint(bmg, V, None)), y, w, None, None, None, "mse")
        lb.backward()
        opt.step()
        assert mp_b.dropout.i == depth + 1   # (every site was visited, the one behind W_d last)
        lb = float(lb.detach())
        print(f"VDDROP {name} step {s}: fused {la:.8f} module {lb:.8f}")
        assert abs(la - lb) <= (1e-5 if s == 0 else 1e-4) * max(1.0, abs(lb)), (s, la, lb)
    torch.cuda.synchronize()
    assert len(set(seeds)) == 3 and tr.opt.steps == 3
    mp_b.tau = tau_b
    for (k, pa), (kb, pb) in zip(a.named_parameters(), b.named_parameters()):
        assert k == kb
        e = parity_err(pa.detach().cpu().numpy(), pb.detach().cpu().numpy())
        print(f"VDDROP {name} {k}: {e:.2e}")
        assert e <= 1e-4, f"{k}: {e:.2e}"
    for k in ("running_mean", "running_var"):
        assert parity_err(getattr(a.bn, k).cpu().numpy(), getattr(b.bn, k).cpu().numpy()) <= 1e-5, k
    assert int(a.bn.num_batches_tracked) == int(b.bn.num_batches_tracked) == 3
    moved = not torch.equal(a.message_passing.W_d.weight.detach(), w_d0)
    assert moved != frozen   # (the layer learns — or, frozen, stays bit for bit)


def test_eval_still_raises_and_p_zero_sends_no_mask(gpu_device, monkeypatch):
    from chemprop_amd.model import FusedTrainer

    monkeypatch.setenv("DMPNN_VALIDATE", "never")
    a, _, bmg, y, w, V = step_inputs(64, "qm9", 3, 64, "relu", gpu_device)
    tr = FusedTrainer(a, lr=1e-3, eps=1e-4, vd_dropout=True)
    seen = _spy(tr)
    float(tr.step(bmg, y, w, V_d=V)[0])
    assert float(seen["vd"].dropout_p) > 0
    a.eval()
    with pytest.raises(RuntimeError, match="eval mode"):
        tr.step(bmg, y, w, V_d=V)
    a.train()
    assert tr.opt.steps == 1
    a.message_passing.dropout.p = 0.0
    rng = torch.get_rng_state()
    loss = float(tr.step(bmg, y, w, V_d=V)[0])
    assert float(seen["vd"].dropout_p) == 0.0 and int(seen["vd"].dropout_seed) == 0
    assert float(seen["part"].st.args.dropout_p) == 0.0 and torch.equal(torch.get_rng_state(), rng)   # (and no seed was drawn)
    assert np.isfinite(loss) and tr.opt.steps == 2


# ---- 3. the staged step ---------------------------------------------------------------------------------------------------------------
def test_staged_step_with_vd_dropout_equals_the_one_call_step(gpu_device, monkeypatch):
    """The data-parallel form (forward + head, exchange, the layer's and the block's backward, exchange, update: forced on one rank)
    against the one-call step under the same seeds — the backward stage runs the layer ONCE: a second run would mask ``gout`` twice."""
    from chemprop_amd.model import FusedTrainer

    a, b, bmg, y, w, V = step_inputs(96, "qm9", 20, 300, "relu", gpu_device)
    torch.manual_seed(501)
    ta = FusedTrainer(a, lr=1e-3, eps=1e-4, vd_dropout=True)
    # (four steps: the first two on launched, validated plans; from the third on K0 inside the FORWARD stage)
    la, sa = [], []
    for _ in range(4):
        la.append(float(ta.step(bmg, y, w, V_d=V)[0]))
        sa.append(ta.last_dropout_seed)
    monkeypatch.setenv("DMPNN_FORCE_COLLECTIVE", "1")
    torch.manual_seed(501)
    tb = FusedTrainer(b, lr=1e-3, eps=1e-4, vd_dropout=True)
    lb, sb = [], []
    for _ in range(4):
        lb.append(float(tb.step(bmg, y, w, V_d=V)[0]))
        sb.append(tb.last_dropout_seed)
    assert tb._checked == 2 and sa == sb and len(set(sa)) == 4
    torch.cuda.synchronize()
    for x, z in zip(la, lb):
        assert abs(x - z) <= 1e-5 * max(1.0, abs(z)), (la, lb)
    for (k, pa), (_, pb) in zip(a.named_parameters(), b.named_parameters()):
        assert parity_err(pa.detach().cpu().numpy(), pb.detach().cpu().numpy()) <= 1e-5, k


# ---- 4. HipMPNN -----------------------------------------------------------------------------------------------------------------------
def test_hip_mpnn_with_atom_descriptors_and_dropout_takes_the_fused_step(stub_chemprop, gpu_device):  # noqa: F811
    """``HipMPNN.training_step`` takes a ``"fused:..."`` route for a model with ``W_d`` and ``dropout=0.1`` and computes, under the same
    torch seed, what ``FusedTrainer(copy, ffn_dropout=True, rows_dropout=True, vd_dropout=True)`` computes, over three steps."""
    from chemprop_amd.model import FusedTrainer, RegressionFFN
    from test_atom_descriptors_integration import _batch, _fake_trainer, _with_w_d

    S, d_vd = stub_chemprop, 20
    integ = S.integration
    integ.enable()
    HipM = integ.hip_mpnn_class()[1]
    torch.manual_seed(3)
    mp = _with_w_d(S, d_vd, dropout=0.1)
    a = HipM(mp, S.mods["chemprop.nn"].NormAggregation(), RegressionFFN(input_dim=mp.output_dim), batch_norm=True, init_lr=1e-3)
    a = a.to(gpu_device).train()
    b = copy.deepcopy(a)
    bmg, y, w, V = _batch(96, d_vd, gpu_device)
    opt = _fake_trainer(a)
    tr = FusedTrainer(b, lr=1e-3, ffn_dropout=True, rows_dropout=True, vd_dropout=True)
    for i in range(3):
        out = {}

        def closure(i=i):
            out["loss"] = a.training_step((bmg, V, None, y, w, None, None), i)
            return out["loss"]

        torch.manual_seed(700 + i)
        opt.step(closure)
        assert a.__dict__["_hip"]["route"].startswith("fused:"), a.__dict__["_hip"]
        torch.manual_seed(700 + i)
        lb = float(tr.step(bmg, y, w, V_d=V)[0])
        assert a.__dict__["_hip"]["fused"].last_dropout_seed == tr.last_dropout_seed
        assert abs(float(out["loss"]) - lb) <= 1e-6 * max(1.0, abs(lb)), (i, float(out["loss"]), lb)
    torch.cuda.synchronize()
    for (k, pa), (_, pb) in zip(a.named_parameters(), b.named_parameters()):
        assert parity_err(pa.detach().cpu().numpy(), pb.detach().cpu().numpy()) <= 1e-6, k
