"""Block dropout in the row kernels of the per-step general route on the f16 pipe (``general16``): the DROP builds of ``k_rows16``
alone through ``dmpnn_linear16_dropout_fwd``, the training forward / backward through ``engine.forward(route="general",
mfma="split16", keep=True, dropout=(p, seed))`` and ``engine.backward``, the same mask on the lean route, and the one-call step
(``FusedTrainer(model, rows_dropout=True)``).

Every reference is float64 with the hash masks of ``oracle/dropout_hash.py`` replayed — a stochastic op is compared given its mask —
and the ``float`` scale ``1.f / (1.f - p)`` the kernels use.  Shapes: the smallest at which this code can go wrong (a partial and a full
48-row tile, one to four column blocks, a 12-column tail, ``N % 4 != 0``: the scalar epilogue, column 1023: the last hash column) plus
the streaming shapes that leave the ``GC = 12`` builds (more than 512 workgroups), one per ``WN``.

Figures of this file's cases on one MI355X (they are printed before every assertion):
  row kernel   err / max(e32, 2**-23) at most 1.55 (C) and 1.92 (Zpre) over the 50 shapes; the bar is rows_harness.MARGIN = 16
  engine       output error 2.7e-07 .. 7.9e-07 (bar TOL = 1e-5), every gradient given the masks at most 5.7e-07 (bar 2e-5), no
               ReLU-class decision differs from float64's in the three ReLU-class cases (at most 8 may, each at the kink)
  two routes   the lean route and the row kernels under one seed: output difference 1.9e-07 (bar TOL), no entry's zero pattern differs
               (bar: 1e-4 of the entries, ReLU zeros at the kink)
"""
import copy
import ctypes as C
import types

import numpy as np
import pytest
import torch

import rows_harness as rh
from chemprop_amd import _lib
from conftest import TOL, parity_err, parity_err_unfloored
from test_dropout_gpu import ReplayDropout, _restated_forward
from test_lean_dropout_gpu import NAMES, RecordingTau, ReplayTau

pytestmark = pytest.mark.gpu

SEED, SEED2 = 0x1234_5678_9ABC_DEF, 77


def _scale32(p):
    """The kernels' ``1.f / (1.f - p)`` as a Python float."""
    return float(np.float32(1.0) / (np.float32(1.0) - np.float32(p)))


# ---- 1. the row kernel alone -----------------------------------------------------------------------------------------------------------
ROW_M, ROW_N = (1, 47, 48, 49, 97), (4, 64, 68, 300, 302, 320, 324, 644, 1024)
# beyond 512 workgroups the launch leaves the GC = 12 builds: 12 340 x 324 is <3, 4>; one more streaming shape per remaining WN
STREAM = ((12340, 324), (24600, 64), (24600, 68), (12340, 644), (24600, 302))
ROW_CASES = [(m, n) for n in ROW_N for m in ROW_M] + list(STREAM)
ROW_ACTS, ROW_PS = ("none", "relu", "tanh"), (0.1, 0.5)


def test_the_row_cases_reach_every_drop_build():
    builds = {rh.linear16_build(m, n) for m, n in ROW_CASES}
    assert builds == {(wn, gc) for wn in (1, 2, 3, 4, 5) for gc in (4, 12)}, sorted(builds)
    assert {rh.linear16_build(m, n)[1] for m, n in STREAM} == {4}
    assert any(n % 4 for _, n in ROW_CASES) and any(n == 1024 for _, n in ROW_CASES)


def _run16(dev, inp, act, drop=None):
    """One ``dmpnn_linear16_fwd`` (``drop is None``) or ``dmpnn_linear16_dropout_fwd`` (``drop = (p, seed, site)``) call on dense
    operands; ``C`` has a padded leading dimension.  -> (C, Zpre) read back with padding and guard regions checked."""
    lib = _lib.load()
    M, N, K1, K2 = inp["M"], inp["N"], inp["K1"], inp["K2"]
    m1 = rh.Mat(dev, M, K1, None, 0, inp["A1"])
    m2 = rh.Mat(dev, M, K2, None, 0, inp["A2"]) if K2 else None
    mw = rh.Mat(dev, N, K1 + K2, None, 0, inp["W"])
    mc = rh.Mat(dev, M, N, None, 0, inp["Cadd"])
    oC, oZ = rh.Mat(dev, M, N, N + 4), rh.Mat(dev, M, N)
    b = inp["bias"].to(dev)
    g = _lib.GemmArgs()
    g.M, g.N, g.K1, g.K2 = M, N, K1, K2
    g.A1, g.lda1 = m1.ptr, m1.ld
    if m2 is not None:
        g.A2, g.lda2 = m2.ptr, m2.ld
    g.W, g.ldw, g.bias = mw.ptr, mw.ld, b.data_ptr()
    g.Cadd, g.ldcadd = mc.ptr, mc.ld
    g.C, g.ldc, g.Zpre, g.ldz = oC.ptr, oC.ld, oZ.ptr, oZ.ld
    g.act, g.act_slope = _lib.ACT[act], rh.act_slope(act) or 0.0
    nb = int(lib.dmpnn_linear16_wsplit_bytes(N, K1 + K2))
    ws = torch.full((nb + 4096,), 0xA5, dtype=torch.uint8, device=dev)
    if drop is None:
        rc, msg, _ = rh._call(dev, lib.dmpnn_linear16_fwd, C.byref(g), ws.data_ptr(), nb, 0)
    else:
        rc, msg, _ = rh._call(dev, lib.dmpnn_linear16_dropout_fwd, C.byref(g), ws.data_ptr(), nb, 0, float(drop[0]), int(drop[1]), int(drop[2]))
    assert rc == 0, (rc, msg)
    assert bool((ws[nb:] == 0xA5).all()), "the weight split wrote behind its workspace"
    return oC.read("C"), oZ.read("Zpre")


@pytest.mark.parametrize("M,N", ROW_CASES, ids=[f"M{m}-N{n}" for m, n in ROW_CASES])
def test_row_kernel_dropout_given_the_hash_mask(M, N, gpu_device):
    from oracle import dropout_hash as dh

    dev = gpu_device
    i = ROW_CASES.index((M, N))
    act, p, site = ROW_ACTS[i % 3], ROW_PS[(i // 3) % 2], 1 + i % 5
    # two operands, 66 columns (three k-chunks, the last one partial); the streaming shapes: several 128-column operand groups
    K1, K2 = (40, 26) if M < 1000 else (200, 124)
    inp = rh.linear_inputs(M, N, K1, K2, seed=i)
    wn, gc = rh.linear16_build(M, N)
    case = f"rows-dropout M{M} N{N} {act} p{p} site{site} <{wn},{gc}>"

    Cd, Zd = _run16(dev, inp, act, (p, SEED, site))
    Cd2, Zd2 = _run16(dev, inp, act, (p, SEED, site))
    Co, _ = _run16(dev, inp, act, (p, SEED2, site))
    Cs, _ = _run16(dev, inp, act, (p, SEED, site + 1))
    Cp, Zp = _run16(dev, inp, act)

    keep = torch.from_numpy(dh.keep_mask(SEED, site, M, N, p))
    bits = lambda t: t.contiguous().view(torch.int32)
    # every masked entry is exactly +0.0; Zpre is the unmasked run's, bit for bit; the same seed twice: bit-identical
    assert bool((bits(Cd)[~keep] == 0).all()), case
    assert torch.equal(bits(Zd), bits(Zp)), case
    assert torch.equal(bits(Cd), bits(Cd2)) and torch.equal(bits(Zd), bits(Zd2)), case
    # a kept entry is the unmasked one times the float scale, bit for bit
    assert Cp.dtype == torch.float32 and torch.equal(bits(Cd)[keep], bits(Cp * _scale32(p))[keep]), case
    # another seed / another site: another zero pattern (from 64 entries on: 4 entries at p = 0.1 can agree by chance)
    if M * N >= 64:
        keep_o, keep_s = torch.from_numpy(dh.keep_mask(SEED2, site, M, N, p)), torch.from_numpy(dh.keep_mask(SEED, site + 1, M, N, p))
        assert not torch.equal(keep_o, keep) and not torch.equal(keep_s, keep)
        assert bool((bits(Co)[~keep_o] == 0).all()) and bool((bits(Cs)[~keep_s] == 0).all()), case
        if act != "relu":   # (a ReLU zero looks like a dropped entry; none / tanh are zero only where dropped)
            assert torch.equal(Co == 0, ~keep_o) and torch.equal(Cs == 0, ~keep_s) and torch.equal(Cd == 0, ~keep), case

    # the kept entries against float64 given the mask, at the row kernels' own bar
    s = _scale32(p)
    r64, r32 = rh.linear_ref(inp, act), rh.linear_ref(inp, act, torch.float32)
    ref = dict(C=torch.where(keep, r64["C"] * s, torch.zeros((), dtype=torch.float64)), Zpre=r64["Zpre"])
    ref32 = dict(C=torch.where(keep, r32["C"] * s, torch.zeros(())), Zpre=r32["Zpre"])
    fails = rh.compare(case, dict(C=Cd, Zpre=Zd), ref, rh.yardstick(ref, ref32), "fwd")
    assert not fails, (case, fails)


# ---- 2. forward and every parameter gradient through the engine -----------------------------------------------------------------------
ACT_OF = {"ReLU": "relu", "LeakyReLU": "leakyrelu", "Tanh": "tanh", "ELU": "elu"}


def _slope(mp):
    return float(getattr(mp.tau, "negative_slope", 0.0))


def _engine_forward(mp, plan, bmg, drop, **kw):
    from chemprop_amd import engine

    W = lambda lin, n: getattr(getattr(mp, lin), n)
    return engine.forward(plan, bmg.V, bmg.E, W("W_i", "weight"), W("W_h", "weight"), W("W_o", "weight"), W("W_o", "bias"),
                          W("W_i", "bias"), W("W_h", "bias"), depth=mp.depth, act=ACT_OF[type(mp.tau).__name__], slope=_slope(mp), keep=True,
                          dropout=drop, **kw)


ROWS = dict(route="general", mfma="split16")


def _masks(seed, p, depth, nE, nV, d_h):
    """The hash masks (bool: kept): the update sites — rows are the caller's edge ids — then the finalize site (atom ids)."""
    from oracle import dropout_hash as dh

    return [torch.from_numpy(dh.keep_mask(seed, t, nE, d_h, p)) for t in range(depth - 1)] + [torch.from_numpy(dh.keep_mask(seed, depth - 1, nV, d_h, p))]


def _reference(cpu_bmg, mp_kw, state, p, keeps, tau_of):
    """The restated forward in float64 with the masks replayed at the kernels' float scale; ``tau_of`` wraps the activation."""
    from chemprop_amd.nn import BondMessagePassing

    ref = BondMessagePassing(dropout=p, **mp_kw)
    ref.load_state_dict(state)
    ref = ref.double().train()
    ref.tau = tau_of(ref.tau)
    g = types.SimpleNamespace(V=cpu_bmg.V.double(), E=cpu_bmg.E.double(), edge_index=cpu_bmg.edge_index, rev_edge_index=cpu_bmg.rev_edge_index)
    masks = [k.double() * _scale32(p) for k in keeps]
    return ref, _restated_forward(g, ref, ReplayDropout(p, masks))


CASES = [
    (12, "zinc", dict(d_h=400, depth=3), 0.25),
    (8, "synth40", dict(d_h=324, depth=2, activation="leakyrelu", bias=True), 0.4),
    (6, "zinc", dict(d_h=644, depth=3, activation="tanh"), 0.1),
    (4, "synth40", dict(d_h=1024, depth=2, activation="elu", bias=True), 0.5),
    (16, "qm9", dict(d_h=302, depth=4, activation="tanh"), 0.2),                   # N % 4 != 0: the scalar epilogue, ldh = 304
    (10, "zinc", dict(d_h=64, depth=1), 0.3),                                      # the finalize site only
]


@pytest.mark.parametrize("n_mols,kind,kw,p", CASES, ids=[f"{c[1]}-{c[0]}-h{c[2]['d_h']}" for c in CASES])
def test_general16_dropout_given_its_masks(n_mols, kind, kw, p, gpu_device):
    from chemprop_amd import engine, synth
    from chemprop_amd.nn import BondMessagePassing

    dev = gpu_device
    cpu_bmg = synth.random_batch(n_mols, kind, seed=11)
    torch.manual_seed(5)
    mp = BondMessagePassing(dropout=p, **kw)
    state = {k: v.clone() for k, v in mp.state_dict().items()}
    nV, nE, d_h, depth = int(cpu_bmg.V.shape[0]), int(cpu_bmg.E.shape[0]), kw["d_h"], mp.depth
    relu_class = type(mp.tau).__name__ in ("ReLU", "LeakyReLU")
    G = torch.randn(nV, d_h, generator=torch.Generator().manual_seed(6))
    mp = mp.to(dev).train()
    bmg = synth.random_batch(n_mols, kind, seed=11)
    bmg.to(dev)
    plan = engine.GraphPlan.from_bmg(bmg)
    assert nE > 48 and nV > 48                                                     # more than one row tile at both kinds of site

    out, st = _engine_forward(mp, plan, bmg, (p, SEED), **ROWS)
    assert st.route == "general16", st.route
    assert abs(float(st.args.dropout_p) - p) < 1e-7 and int(st.args.dropout_seed) == SEED
    need = {k: True for k, _, _ in NAMES}
    g1 = engine.backward(st, G.to(dev), need)
    g1 = {k: (None if v is None else v.clone()) for k, v in g1.items()}
    g2 = engine.backward(st, G.to(dev), need)
    torch.cuda.synchronize()
    for k in g1:                                                                   # two backward passes on one forward: bit-identical
        assert (g1[k] is None) == (g2[k] is None) and (g1[k] is None or torch.equal(g1[k], g2[k])), k
    again, _ = _engine_forward(mp, plan, bmg, (p, SEED), **ROWS)
    other, _ = _engine_forward(mp, plan, bmg, (p, SEED2), **ROWS)
    assert torch.equal(again, out)
    assert not torch.equal(other == 0, out == 0)

    keeps = _masks(SEED, p, depth, nE, nV, d_h)
    out_c = out.detach().cpu()
    fin = keeps[-1]
    # what the finalize zeroed is what the hash says (a smooth activation is zero nowhere else); the kept H^(t) likewise
    assert bool((out_c[~fin] == 0).all())
    if not relu_class:
        assert torch.equal(out_c == 0, ~fin)
    Hs = st.Hs[:, :, :d_h].detach().cpu() if depth > 1 else None
    for t in range(depth - 1):
        assert bool((Hs[t][~keeps[t]] == 0).all()), f"update site {t}"
        if not relu_class:
            assert torch.equal(Hs[t] == 0, ~keeps[t]), f"update site {t}"
    for k in keeps:
        assert abs(float(k.double().mean()) - (1 - p)) <= 0.01

    # the output against float64 given the masks
    ref, ref_out = _reference(cpu_bmg, kw, state, p, keeps, RecordingTau)
    pre = ref.tau.pre
    assert len(pre) == depth + 1
    err_out = parity_err(out_c.numpy(), ref_out.detach().numpy())
    print(f"rows-dropout {kind}-{n_mols}-h{d_h}: output error {err_out:.3e}")
    assert err_out <= TOL, err_out

    if relu_class:
        # the engine's own 0 / 1 decisions replayed: the sign of the kept pre-activation H0, of the kept H^(t) / the output where
        # the mask kept the entry, the reference's own decision where it did not (times 0 there)
        H0 = st.H0[:, :d_h].detach().cpu()
        cond = [H0 > 0] + [torch.where(keeps[t], Hs[t] > 0, pre[t + 1] > 0) for t in range(depth - 1)] + [torch.where(fin, out_c > 0, pre[depth] > 0)]
        flips = 0
        for t in range(depth + 1):
            diff = cond[t] != (pre[t] > 0)
            flips += int(diff.sum())
            if diff.any():
                assert float(pre[t][diff].abs().max()) <= 1e-5 * float(pre[t].abs().max()), f"site {t}: a decision differs away from the kink"
        print(f"rows-dropout {kind}-{n_mols}-h{d_h}: {flips} activation decisions differ from float64's")
        assert flips <= 8, flips
        ref, ref_out = _reference(cpu_bmg, kw, state, p, keeps, lambda inner: ReplayTau(cond, _slope(mp)))
        assert parity_err(out_c.numpy(), ref_out.detach().numpy()) <= TOL
    else:
        ref, ref_out = _reference(cpu_bmg, kw, state, p, keeps, lambda inner: inner)
    (ref_out * G.double()).sum().backward()
    errs = {}
    for k, lin, n in NAMES:
        prm = getattr(getattr(ref, lin), n)
        if prm is None:
            assert g1[k] is None
            continue
        if prm.grad is None:                                                       # (depth 1: W_h takes no part; the engine answers zeros)
            assert depth == 1 and lin == "W_h" and not bool(g1[k].any()), k
            continue
        errs[k] = parity_err_unfloored(g1[k].cpu().numpy(), prm.grad.numpy())
    print(f"rows-dropout {kind}-{n_mols}-h{d_h}: gradient errors given the masks {errs}")
    assert max(errs.values()) <= 2e-5, errs


def test_the_default_general16_route_and_the_fp32_pipe_still_refuse_dropout(gpu_device):
    from chemprop_amd import engine, synth
    from chemprop_amd.nn import BondMessagePassing

    dev = gpu_device
    torch.manual_seed(5)
    mp = BondMessagePassing(d_h=400, dropout=0.2).to(dev).train()
    bmg = synth.random_batch(12, "zinc", seed=11)
    bmg.to(dev)
    plan = engine.GraphPlan.from_bmg(bmg)
    _, st = _engine_forward(mp, plan, bmg, None)
    assert st.route == "general16" and float(st.args.dropout_p) == 0.0             # (the rule's choice without dropout)
    for kw in (dict(), dict(route="general"), dict(route="general", mfma="f32")):
        with pytest.raises(engine.RouteUnavailable):
            _engine_forward(mp, plan, bmg, (0.2, 5), **kw)


# ---- 3. the same mask on two routes ---------------------------------------------------------------------------------------------------
def test_the_same_mask_on_the_lean_route_and_in_the_row_kernels(gpu_device):
    from chemprop_amd import engine, synth
    from chemprop_amd.nn import BondMessagePassing

    dev, p, seed = gpu_device, 0.3, 424242
    torch.manual_seed(8)
    mp = BondMessagePassing(d_h=128, dropout=p).to(dev).train()
    bmg = synth.random_batch(24, "zinc", seed=12)
    bmg.to(dev)
    plan = engine.GraphPlan.from_bmg(bmg)
    lean, st_l = _engine_forward(mp, plan, bmg, (p, seed), route="fused16")
    rows, st_r = _engine_forward(mp, plan, bmg, (p, seed), **ROWS)
    assert st_l.route == "fused16/lean" and st_r.route == "general16", (st_l.route, st_r.route)
    fin = _masks(seed, p, mp.depth, int(bmg.E.shape[0]), int(bmg.V.shape[0]), 128)[-1].to(dev)
    assert bool((lean[~fin] == 0).all()) and bool((rows[~fin] == 0).all())
    err = parity_err(rows.cpu().numpy(), lean.cpu().numpy())
    differ = float(((lean == 0) != (rows == 0)).float().mean())
    print(f"lean route against the row kernels, one seed: output difference {err:.3e}, zero patterns differ in {differ:.3e} of the entries")
    assert err <= TOL
    assert differ < 1e-4                                                           # (a ReLU zero at the kink; the masks are identical)


# ---- 4. the one-call step -------------------------------------------------------------------------------------------------------------
def _model(dev, **mp_kw):
    from chemprop_amd import agg as cagg
    from chemprop_amd.model import MPNN, RegressionFFN
    from chemprop_amd.nn import BondMessagePassing

    return MPNN(BondMessagePassing(dropout=0.2, **mp_kw), cagg.MeanAggregation(), RegressionFFN(input_dim=mp_kw["d_h"])).to(dev).train()


def _batch(dev, kind):
    from chemprop_amd import synth

    bmg = synth.random_batch(24, kind, seed=13)
    # targets the graph determines: a fixed readout of every molecule's mean atom features, standardised
    coef = torch.randn(bmg.V.shape[1], 1, generator=torch.Generator().manual_seed(14))
    n = len(bmg)
    m = torch.zeros(n, bmg.V.shape[1]).index_add(0, bmg.batch, bmg.V) / torch.bincount(bmg.batch, minlength=n).view(-1, 1)
    y = m @ coef
    y = (y - y.mean()) / y.std()
    bmg.to(dev)
    return bmg, y.to(dev)


STEP_MODELS = [("zinc", dict(d_h=400)), ("qm9", dict(d_h=64, activation="tanh"))]
STEP_IDS = ["zinc-relu-h400", "qm9-tanh-h64"]


@pytest.mark.parametrize("kind,kw", STEP_MODELS, ids=STEP_IDS)
def test_fused_trainer_takes_the_row_kernels_for_block_dropout(kind, kw, gpu_device):
    from chemprop_amd import engine
    from chemprop_amd.model import FusedTrainer
    from head_harness import run_head

    dev = gpu_device
    torch.manual_seed(21)
    model = _model(dev, **kw)
    bmg, y = _batch(dev, kind)
    before = copy.deepcopy(model)
    with pytest.raises(NotImplementedError):                                       # (without the keyword: at construction, or by the step)
        FusedTrainer(copy.deepcopy(model), lr=1e-3).step(bmg, y)
    tr = FusedTrainer(model, lr=1e-3, rows_dropout=True)
    torch.manual_seed(99)
    first = int(torch.randint(0, 2 ** 62, (1,), dtype=torch.int64).item())
    torch.manual_seed(99)
    loss = tr.step(bmg, y)
    torch.cuda.synchronize()
    assert tr.last_route == "general16", tr.last_route
    assert tr.last_dropout_seed == first
    step_grads = {id(p): tr._views[id(p)].detach().clone() for p in model.message_passing.parameters()}

    # the same step by hand on the parameters before it: engine.forward for that seed, the head on its output, engine.backward on gH_v
    mp = before.message_passing
    plan = engine.GraphPlan.from_bmg(bmg)
    out, st = _engine_forward(mp, plan, bmg, (0.2, first), **ROWS)
    assert st.route == "general16"
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


@pytest.mark.parametrize("kind,kw", STEP_MODELS, ids=STEP_IDS)
def test_fused_trainer_learns_with_block_dropout_in_the_row_kernels(kind, kw, gpu_device):
    from chemprop_amd.model import FusedTrainer

    dev = gpu_device
    torch.manual_seed(22)
    model = _model(dev, **kw)
    bmg, y = _batch(dev, kind)
    tr = FusedTrainer(model, lr=3e-3, rows_dropout=True)
    losses = [float(tr.step(bmg, y)[0]) for _ in range(60)]
    assert tr.last_route == "general16", tr.last_route
    print(f"rows-dropout trainer {kind}: first five losses {losses[:5]}, last five {losses[-5:]}")
    assert np.mean(losses[-5:]) < 0.7 * np.mean(losses[:5]), (losses[:5], losses[-5:])


def test_fused_trainer_eval_draws_no_seed_with_rows_dropout(gpu_device):
    from chemprop_amd.model import FusedTrainer

    dev = gpu_device
    torch.manual_seed(23)
    model = _model(dev, d_h=64, activation="tanh")
    bmg, y = _batch(dev, "qm9")
    tr = FusedTrainer(model, lr=1e-3, rows_dropout=True)
    model.eval()
    rng = torch.get_rng_state()
    part = tr._block_args(tr.mp, bmg, len(bmg), tr.acts[0], False, None, None)
    assert float(part.st.args.dropout_p) == 0.0 and torch.equal(torch.get_rng_state(), rng)
    assert not hasattr(tr, "last_dropout_seed") or tr.last_dropout_seed is None
    with pytest.raises(RuntimeError, match="eval mode"):
        tr.step(bmg, y)
