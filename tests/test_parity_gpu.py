"""Parity of the HIP path against the oracle — runs on a real MI355X only (`-m gpu`).

Every call goes through the C-ABI (ctypes -> libdmpnn_gfx950.so).  Bars:
  * integer / index work (graph plan): bit-exact against the numpy CSR restatement;
  * segment kernels (message, aggregate): bit-exact against the golden vectors of the executed
    reference (same fp32 addition order by construction);
  * contractions and whole forward: <= 1e-5 norm-wise relative (BASELINE.json north_star) —
    `max|a-b| <= 1e-5 * max(1, max|ref|)`.
"""
import numpy as np
import pytest
import torch

from conftest import TOL, parity_err


def small_fits(nV, nE):
    from chemprop_amd.engine import small_plan_fits

    return small_plan_fits(nV, nE)

from oracle import dmpnn_numpy as onp
from oracle import dmpnn_torch as ot

pytestmark = pytest.mark.gpu


def _plan(golden, dev):
    from chemprop_amd.engine import GraphPlan

    return GraphPlan(torch.from_numpy(golden["edge_index"]).to(dev), torch.from_numpy(golden["rev_edge_index"]).to(dev),
                     golden["V"].shape[0])


def test_plan_is_bit_exact(golden, gpu_device):
    plan = _plan(golden, gpu_device)
    a = {k: v.numpy() for k, v in plan.arrays().items()}
    src, dst = golden["edge_index"]
    rev = golden["rev_edge_index"]
    nV = golden["V"].shape[0]
    row_ptr, perm = onp.build_csr(dst, nV)
    assert np.array_equal(a["src"], src) and np.array_equal(a["dst"], dst) and np.array_equal(a["rev"], rev)
    assert np.array_equal(a["row_ptr"], row_ptr)
    assert np.array_equal(a["perm"], perm)
    assert bool(a["hdr"][0] & 1) == (not onp.graph_is_symmetric(src, dst, rev))
    assert not (a["hdr"][0] & 2)
    maxdeg = int(np.diff(row_ptr).max()) if len(perm) else 0
    assert a["hdr"][1] == maxdeg
    assert bool(a["hdr"][0] & 4) == (maxdeg > 24)
    # CSR-row coordinates and the row tiles of whole atoms (fused forward)
    rc = onp.row_coordinates(src, dst, rev, perm)
    for k in ("inv", "srcp", "dstp", "revp"):
        assert np.array_equal(a[k], rc[k]), k
    n_slots = len(a["tile_row"]) - 2
    tile_row, tile_atom, n_tiles, b0 = onp.tile_tables(row_ptr, len(perm), n_slots)
    assert a["hdr"][4] == n_tiles and (n_tiles == 0 or a["hdr"][5] == b0)
    assert np.array_equal(a["tile_row"], tile_row) and np.array_equal(a["tile_atom"], tile_atom)
    assert n_tiles <= n_slots and (np.diff(tile_row) <= 48).all() and (np.diff(tile_row) >= 0).all()
    # row tiles of whole connected pieces (whole-forward tile kernel); built by the single-workgroup plan
    m_slots = len(a["mtile_row"]) - 2
    from chemprop_amd.engine import small_plan_fits
    small = small_plan_fits(nV, len(perm))
    if small and onp.graph_is_symmetric(src, dst, rev):
        mrow, matom, n_m = onp.piece_tiles(src, dst, row_ptr, m_slots)
        assert bool(a["hdr"][0] & 8) == (n_m < 0)
        assert a["hdr"][6] == max(n_m, 0)
        assert np.array_equal(a["mtile_row"], mrow) and np.array_equal(a["mtile_atom"], matom)
        # pieces beyond the matrix-pipe tile are tiles of their own, counted in DMPNN_HDR_NSPILL
        n_spill = sum(1 for t in range(max(n_m, 0)) if mrow[t + 1] - mrow[t] > 48 or matom[t + 1] - matom[t] > 32)
        assert a["hdr"][8] == n_spill
    elif not small:
        assert a["hdr"][0] & 8 and a["hdr"][6] == 0


def test_light_plan_matches_full_plan(golden, gpu_device):
    """dmpnn_prepare_light writes the same row_ptr / perm / srcp / revp / tile tables / header as the full plan."""
    from chemprop_amd.engine import GraphPlan

    ei = torch.from_numpy(golden["edge_index"]).to(gpu_device)
    rev = torch.from_numpy(golden["rev_edge_index"]).to(gpu_device)
    full = GraphPlan(ei, rev, golden["V"].shape[0]).arrays()
    lp = GraphPlan(ei, rev, golden["V"].shape[0], light=True)
    light = lp.arrays()
    for k in ("row_ptr", "perm", "srcp", "revp", "tile_row", "tile_atom", "mtile_row", "mtile_atom"):
        assert torch.equal(full[k], light[k]), k
    assert torch.equal(full["hdr"][:7], light["hdr"][:7]) and int(light["hdr"][7]) == int(lp.light)


def test_message_kernel_bit_exact(golden, gpu_device):
    from chemprop_amd import engine

    if "M1" not in golden:
        pytest.skip("no stored message for this case")
    act = golden.cfg["activation"]
    plan = _plan(golden, gpu_device)
    H0 = torch.from_numpy(golden["H0"]).to(gpu_device)
    slope_t = torch.tensor([0.25], device=gpu_device) if act == "prelu" else None
    M = engine.message(plan, H0, act_on_load=act, slope=0.1, slope_t=slope_t)
    if act in ("relu", "leakyrelu", "prelu"):
        assert np.array_equal(M.cpu().numpy(), golden["M1"])
    else:  # tanhf / expm1f differ from the host libm by an ulp
        assert parity_err(M.cpu().numpy(), golden["M1"]) <= 1e-6
    # tau applied beforehand by torch + act_on_load="none" must agree bit-for-bit on exact activations
    if act == "relu":
        M2 = engine.message(plan, torch.relu(H0))
        assert torch.equal(M, M2)


def test_aggregate_kernel_bit_exact(golden, gpu_device):
    from chemprop_amd import engine

    if "H_last" not in golden:
        pytest.skip("no stored H_last for this case")
    plan = _plan(golden, gpu_device)
    H = torch.from_numpy(golden["H_last"]).to(gpu_device)
    Mv = engine.aggregate(plan, H)
    assert np.array_equal(Mv.cpu().numpy(), golden["Mv"])


def test_initialize_kernel(golden, gpu_device):
    """K1: gather + concat fused into the A-operand loader of the MFMA contraction."""
    from chemprop_amd import engine

    if "H0" not in golden:
        pytest.skip("big case")
    plan = _plan(golden, gpu_device)
    w = golden.weights()
    t = lambda a: torch.from_numpy(np.array(a)).to(gpu_device)
    b = t(w["W_i.bias"]) if "W_i.bias" in w else None
    H0 = engine.linear(t(golden["V"]), t(w["W_i.weight"]), b, A2=t(golden["E"]), gather1=plan.src32,
                       n_rows=plan.n_edges)
    assert parity_err(H0.cpu().numpy(), golden["H0"]) <= TOL


def test_forward_matches_executed_reference(golden, gpu_device):
    """Whole BondMessagePassing.forward through the mirror module (state_dict-compatible)."""
    mp = golden.module(gpu_device)
    bmg = golden.bmg(gpu_device)
    V_d = torch.from_numpy(golden["V_d"]).to(gpu_device) if "V_d" in golden else None
    before = [bmg.V.clone(), bmg.E.clone(), bmg.edge_index.clone(), bmg.rev_edge_index.clone()]
    with torch.no_grad():
        out = mp(bmg, V_d)
    assert out.shape == golden["out"].shape
    err = parity_err(out.cpu().numpy(), golden["out"])
    assert err <= TOL, f"{golden.name}: {err:.3e}"
    # forward must not mutate the batch (tests/integration/test_regression_mol.py:217-226)
    for a, b in zip(before, [bmg.V, bmg.E, bmg.edge_index, bmg.rev_edge_index]):
        assert torch.equal(a, b)


def _engine_forward(golden, dev, fused=None, keep=False, route=None, mfma=None, plan=None, form=0):
    from chemprop_amd import engine
    from chemprop_amd.nn import classify_activation

    mp = golden.module(dev)
    bmg = golden.bmg(dev)
    if plan is None:
        plan = engine.GraphPlan.from_bmg(bmg)
    act, slope, slope_t = classify_activation(mp.tau)
    V_d = torch.from_numpy(golden["V_d"]).to(dev) if "V_d" in golden else None
    has_vd = mp.W_d is not None and V_d is not None
    with torch.no_grad():
        out, st = engine.forward(plan, bmg.V, bmg.E, mp.W_i.weight, mp.W_h.weight, mp.W_o.weight, mp.W_o.bias,
                                 mp.W_i.bias, mp.W_h.bias, mp.W_d.weight if has_vd else None,
                                 mp.W_d.bias if has_vd else None, V_d if has_vd else None, depth=mp.depth, act=act,
                                 slope=slope, slope_t=slope_t, undirected=mp.undirected, keep=keep, fused=fused,
                                 route=route, mfma=mfma, form=form)
    return plan, out, st


def test_fused_route_is_bit_identical_to_general_route(golden, gpu_device):
    """The fused route (CSR-row order, segment sums in the contraction epilogues) performs the same
    fp32 operations in the same order as the general route: outputs must agree BIT FOR BIT, and the
    kept intermediates are the general route's rows permuted by ``perm``."""
    if golden.cfg.get("undirected") or golden.cfg["d_h"] % 4 or golden.cfg["d_h"] > 320:
        pytest.skip("fused route does not apply (undirected / d_h)")
    if golden["V"].shape[1] % 2 or golden["E"].shape[1] % 2:
        pytest.skip("fused route does not apply (odd feature width: 4-byte operand rows)")
    if str(golden.cfg["activation"]).lower() not in ("relu", "leakyrelu", "prelu", "tanh", "elu"):
        pytest.skip("custom activation: rows route")
    plan, out_g, st_g = _engine_forward(golden, gpu_device, fused=False, keep=True)
    if not plan.fusable():
        plan2, out_f, _ = _engine_forward(golden, gpu_device, route="fused")
        assert torch.isnan(out_f).all(), "a graph the fused tiling cannot hold must come back as NaN, loudly"
        return
    plan, out_f, st_f = _engine_forward(golden, gpu_device, route="fused", keep=True)
    assert st_f.route == "fused" and st_g.route == "general"
    assert torch.equal(out_f, out_g)
    assert parity_err(out_f.cpu().numpy(), golden["out"]) <= TOL
    if plan.n_edges:
        perm = plan.perm64
        assert torch.equal(st_f.H0, st_g.H0[perm])
        d = golden.cfg["depth"]
        for t in range(d - 1):
            assert torch.equal(st_f.Ms[t], st_g.Ms[t][perm]), f"M^({t + 1})"
            assert torch.equal(st_f.Hs[t], st_g.Hs[t][perm]), f"H^({t + 1})"
    assert torch.equal(st_f.Mv, st_g.Mv)
    # inference variant (no H stores, two ping-pong message slots) gives the same output
    _, out_i, st_i = _engine_forward(golden, gpu_device, route="fused", keep=False)
    assert torch.equal(out_i, out_f)


def test_whole_forward_tile_kernel(golden, gpu_device):
    """Route "mega": the whole forward of a tile of whole molecules in ONE launch.  The kept
    intermediates (H0, M^(t), H^(t), Mv) are bit-identical to the per-step fused route (same MFMA / k
    order); the output differs only by the summation order of the finalize contraction (the Mv columns
    are contracted before the V columns) and is held to the parity bar; a molecule larger than a tile takes the
    kernel's generic fp32 path (same bar)."""
    if golden.cfg.get("undirected") or golden.cfg["d_h"] % 4 or golden.cfg["d_h"] > 320:
        pytest.skip("fused routes do not apply (undirected / d_h)")
    if golden["V"].shape[1] % 2 or golden["E"].shape[1] % 2:
        pytest.skip("fused routes do not apply (odd feature width)")
    if str(golden.cfg["activation"]).lower() not in ("relu", "leakyrelu", "prelu", "tanh", "elu"):
        pytest.skip("custom activation: rows route")
    if not small_fits(golden["V"].shape[0], golden["E"].shape[0]):
        pytest.skip("batch beyond the single-workgroup plan")
    plan, out_m, st_m = _engine_forward(golden, gpu_device, route="mega", keep=True, mfma="f32")
    assert st_m.route == "mega"
    if not plan.mega_ok():
        assert torch.isnan(out_m).all()
        return
    assert parity_err(out_m.cpu().numpy(), golden["out"]) <= TOL
    _, out_f, st_f = _engine_forward(golden, gpu_device, route="fused", keep=True)
    assert parity_err(out_m.cpu().numpy(), out_f.cpu().numpy()) <= 2e-6
    # bit-identical where the tile kernel ran its matrix-pipe path; a piece larger than a tile takes the generic fp32 path
    # (ascending-k fmaf chains: another summation order), held to the fp32-rounding class
    same = (lambda a, b, what="": torch.equal(a, b)) if plan.header()[8] == 0 else (
        lambda a, b, what="": parity_err(a.cpu().numpy(), b.cpu().numpy()) <= 3e-6)
    if plan.n_edges:
        assert same(st_m.H0, st_f.H0)
        for t in range(golden.cfg["depth"] - 1):
            assert same(st_m.Ms[t], st_f.Ms[t]), f"M^({t + 1})"
            assert same(st_m.Hs[t], st_f.Hs[t]), f"H^({t + 1})"
    assert same(st_m.Mv, st_f.Mv)
    _, out_i, st_i = _engine_forward(golden, gpu_device, route="mega", keep=False, mfma="f32")
    assert st_i.H0 is None and torch.equal(out_i, out_m)   # inference: nothing but `out` leaves the CU


def test_whole_forward_tile_kernel_split_f16(golden, gpu_device):
    """Route "mega" on the f16 matrix pipe with the exact 3-term split (x s = hi + lo, fp32
    accumulate): held to the SAME parity bar as the fp32-MFMA path against the executed reference,
    intermediates included."""
    if golden.cfg.get("undirected") or golden.cfg["d_h"] % 4 or golden.cfg["d_h"] > 320:
        pytest.skip("fused routes do not apply (undirected / d_h)")
    if golden["V"].shape[1] % 2 or golden["E"].shape[1] % 2:
        pytest.skip("fused routes do not apply (odd feature width)")
    if str(golden.cfg["activation"]).lower() not in ("relu", "leakyrelu", "prelu", "tanh", "elu"):
        pytest.skip("custom activation: rows route")
    if not small_fits(golden["V"].shape[0], golden["E"].shape[0]):
        pytest.skip("batch beyond the single-workgroup plan")
    plan, out_s, st_s = _engine_forward(golden, gpu_device, route="mega", keep=True, mfma="split16")
    assert st_s.route == "mega16"
    if not plan.mega_ok():
        assert torch.isnan(out_s).all()
        return
    err = parity_err(out_s.cpu().numpy(), golden["out"])
    assert err <= TOL, f"{golden.name}: {err:.3e}"
    _, out_f, st_f = _engine_forward(golden, gpu_device, route="fused", keep=True)
    assert parity_err(out_s.cpu().numpy(), out_f.cpu().numpy()) <= 3e-6
    if plan.n_edges:
        assert parity_err(st_s.H0.cpu().numpy(), st_f.H0.cpu().numpy()) <= 3e-6
        from chemprop_amd import engine as _eng

        Ms_s = _eng.kept_messages(st_s)   # (round 4: the tile kernel keeps M^(t) as split rows — exactly what its next contraction read)
        for t in range(golden.cfg["depth"] - 1):
            assert parity_err(Ms_s[t].cpu().numpy(), st_f.Ms[t][:, :Ms_s.shape[-1]].cpu().numpy()) <= 3e-6, f"M^({t + 1})"
            assert parity_err(st_s.Hs[t].cpu().numpy(), st_f.Hs[t].cpu().numpy()) <= 3e-6, f"H^({t + 1})"
    assert parity_err(st_s.Mv.cpu().numpy(), st_f.Mv.cpu().numpy()) <= 3e-6
    _, out_i, _ = _engine_forward(golden, gpu_device, route="mega", keep=False, mfma="split16")
    assert torch.equal(out_i, out_s)


def test_per_step_fused_route_on_the_f16_pipe(golden, gpu_device, monkeypatch):
    """Route "fused16" (dmpnn_step16_impl.hpp): one launch per depth step, message rows kept between the steps in split
    form (hi | lo halfs + the row's scale), operand tiles fetched by LDS-DMA.  Any molecule size.  Held to the same bar
    against the executed reference as every other route; the per-atom sums it leaves in the workspace as well."""
    cfg = golden.cfg
    if cfg.get("undirected") or cfg["d_h"] % 4 or cfg["d_h"] > 320 or golden["V"].shape[1] % 2 or golden["E"].shape[1] % 2:
        pytest.skip("fused routes do not apply")
    if str(cfg["activation"]).lower() not in ("relu", "leakyrelu", "prelu", "tanh", "elu"):
        pytest.skip("custom activation: rows route")
    # Two forms of the residual H0 = W_i [V[src] || E] + b_i in the depth steps: recomputed per step from the exactly split K1
    # operand (the default where d_v + d_e <= 256, d_h <= 320 and depth >= 2: no H0 tensor exists) and written once / read back
    # (DMPNN_F_H0_RESIDUAL: what wide hidden layers and training use).  Same bar for both.
    # The finalize likewise has two forms: on the step kernel over 48-atom tiles, fed by the last step's per-atom sums as split
    # rows (the default from depth 2 on: no fp32 Mv tensor exists), and the row kernel on fp32 Mv (DMPNN_F_ROW_FINALIZE).
    from chemprop_amd._lib import F_H0_RESIDUAL, F_ROW_FINALIZE

    for form in (0, F_H0_RESIDUAL | F_ROW_FINALIZE, F_ROW_FINALIZE, F_H0_RESIDUAL):
        plan, out, st = _engine_forward(golden, gpu_device, route="fused16", form=form)
        assert st.route == "fused16"
        if not plan.fusable():
            assert torch.isnan(out).all()      # not a molecular graph: loud
            return
        err = parity_err(out.cpu().numpy(), golden["out"])
        assert err <= TOL, f"{golden.name} (form {form:#x}): {err:.3e}"
        if (form & F_ROW_FINALIZE) and "Mv" in golden and plan.n_edges:
            assert parity_err(st.Mv[:, :cfg["d_h"]].cpu().numpy(), golden["Mv"]) <= TOL
        if (form & F_H0_RESIDUAL) and "H0" in golden and plan.n_edges:     # kept rows are the plan's CSR rows (row i = edge perm[i])
            H0 = st.H0[:, :cfg["d_h"]][plan.inv32.long()]
            assert parity_err(H0.cpu().numpy(), golden["H0"]) <= TOL
        _, out2, _ = _engine_forward(golden, gpu_device, route="fused16", form=form)
        assert torch.equal(out, out2)          # deterministic (no atomics on the data path)


@pytest.mark.gpu
@pytest.mark.parametrize("kind,n_mols,kw", [("synth40", 96, dict()), ("zinc", 64, dict(d_h=512, depth=6)), ("cgr", 128, dict(d_v=106, d_e=28, bias=True)),
                                             ("qm9", 300, dict(d_h=128, depth=4, activation="tanh"))])
def test_h0_as_row_quads_on_the_per_step_fused_route(kind, n_mols, kw, gpu_device, monkeypatch):
    """Round 5 (``dmpnn_fwd_args.h0_bytes``): an inference forward of the per-step fused route keeps H0 in the layout of the step
    kernel's accumulator fragments (row quads, written by K1 from its registers, read back coalesced by every depth step) instead of
    recomputing ``W_i x`` per step (d_h <= 320) or gathering fp32 rows word by word (d_h > 320).  Both forms against the oracle at the
    1e-5 bar and against each other; tiles of every fill (partial last quads, tiles that start off a multiple of four rows); repeated
    calls identical; beyond ``kH0QuadsMaxEdges`` the library declines the form (``dmpnn_forward_h0_bytes`` == 0)."""
    import ctypes as C

    from chemprop_amd import _lib, engine, synth
    from chemprop_amd.nn import BondMessagePassing, classify_activation
    from oracle import dmpnn_torch as ot

    bmg = synth.random_batch(n_mols, kind, seed=11)
    torch.manual_seed(4)
    mp = BondMessagePassing(**kw).eval()
    with torch.no_grad():
        ref = ot.forward_bmg(bmg, ot.MPWeights.from_module(mp), depth=mp.depth, activation=kw.get("activation", "relu"))
    mp = mp.to(gpu_device)
    bmg.to(gpu_device)
    act, slope, slope_t = classify_activation(mp.tau)
    outs = {}
    for mode in ("quads", "x"):
        monkeypatch.setenv("DMPNN_H0", mode)
        plan = engine.GraphPlan.from_bmg(bmg)
        with torch.no_grad():
            out, st = engine.forward(plan, bmg.V, bmg.E, mp.W_i.weight, mp.W_h.weight, mp.W_o.weight, mp.W_o.bias, mp.W_i.bias, mp.W_h.bias,
                                     depth=mp.depth, act=act, slope=slope, slope_t=slope_t, route="fused16")
            out2, _ = engine.forward(plan, bmg.V, bmg.E, mp.W_i.weight, mp.W_h.weight, mp.W_o.weight, mp.W_o.bias, mp.W_i.bias, mp.W_h.bias,
                                     depth=mp.depth, act=act, slope=slope, slope_t=slope_t, route="fused16")
        assert st.route == "fused16" and (int(st.args.h0_bytes) > 0) == (mode == "quads")
        assert torch.equal(out, out2)
        assert parity_err(out.cpu().numpy(), ref.numpy()) <= TOL, mode
        outs[mode] = out
    assert parity_err(outs["quads"].cpu().numpy(), outs["x"].cpu().numpy()) <= 3e-6
    # the size rule is the library's
    a = _lib.FwdArgs.from_buffer_copy(bytes(st.args))
    a.flags = (a.flags | _lib.F_FUSED | _lib.F_SPLIT16) & ~(_lib.F_MEGA | _lib.F_KEEP)
    lib = _lib.load()
    assert lib.dmpnn_forward_h0_bytes(C.byref(a)) > 0
    a.n_edges = 200000
    assert lib.dmpnn_forward_h0_bytes(C.byref(a)) == 0
    a.n_edges, a.flags = int(bmg.E.shape[0]), a.flags | _lib.F_H0_RESIDUAL
    assert lib.dmpnn_forward_h0_bytes(C.byref(a)) == 0


HALF_TOL = 2e-3  # DMPNN_F_STORE16: one rounding of every message element to an 11-bit significand per depth step (stated in include/dmpnn.h)


def test_half_storage_of_the_messages_golden(golden, gpu_device, monkeypatch):
    """OPT-IN half storage (``DMPNN_STORE=f16`` -> ``DMPNN_F_STORE16``): the per-step fused route keeps the message tensor
    between the steps as one f16 per element + a power-of-two row scale.  Not fp32-class — held to its own stated bar
    (2e-3, norm-wise) on every golden the fused routes take, and it must NOT be what runs by default."""
    cfg = golden.cfg
    if cfg.get("undirected") or cfg["d_h"] % 4 or cfg["d_h"] > 320 or golden["V"].shape[1] % 2 or golden["E"].shape[1] % 2:
        pytest.skip("fused routes do not apply")
    if str(cfg["activation"]).lower() not in ("relu", "leakyrelu", "prelu", "tanh", "elu"):
        pytest.skip("custom activation: rows route")
    plan, out_exact, st = _engine_forward(golden, gpu_device, route="fused16")
    assert st.route == "fused16"                      # (the default storage: exact hi + lo pairs)
    if not plan.fusable():
        pytest.skip("not a molecular graph")
    monkeypatch.setenv("DMPNN_STORE", "f16")
    _, out, st_h = _engine_forward(golden, gpu_device, route="fused16")
    assert st_h.route == "fused16/f16-storage"
    err = parity_err(out.cpu().numpy(), golden["out"])
    assert err <= HALF_TOL, f"{golden.name}: {err:.3e}"
    if cfg["depth"] > 1 and plan.n_edges:
        assert not torch.equal(out, out_exact)        # the flag did change the arithmetic
    _, out2, _ = _engine_forward(golden, gpu_device, route="fused16")
    assert torch.equal(out, out2)


@pytest.mark.parametrize("kind,n_mols,kw", [("synth40", 512, dict()), ("zinc", 512, dict(d_h=512, depth=6)), ("cgr", 256, dict(d_v=106, d_e=28)),
                                            ("qm9", 4096, dict(activation="tanh", bias=True))])
def test_half_storage_at_size(kind, n_mols, kw, gpu_device, monkeypatch):
    from chemprop_amd import synth
    from chemprop_amd.nn import BondMessagePassing
    from oracle import dmpnn_torch as ot

    torch.manual_seed(12)
    mp = BondMessagePassing(**kw).eval()
    b = synth.random_batch(n_mols, kind, seed=21)
    with torch.no_grad():
        ref = ot.forward_bmg(b, ot.MPWeights.from_module(mp), depth=mp.depth, activation=kw.get("activation", "relu"))
    mp = mp.to(gpu_device)
    b.to(gpu_device)
    monkeypatch.setenv("DMPNN_STORE", "f16")
    monkeypatch.setenv("DMPNN_MEGA", "0")             # (QM9-sized molecules would take the whole-forward tile kernel, which has no messages in memory)
    with torch.no_grad():
        for _ in range(3):                            # past the validated first batches
            out = mp(b)
    assert mp.__dict__.get("_dmpnn_route") == "fused16/f16-storage", mp.__dict__.get("_dmpnn_route")
    err = parity_err(out.cpu().numpy(), ref.numpy())
    print(f"half storage {kind}-{n_mols}: {err:.2e}")
    assert err <= HALF_TOL, f"{kind}-{n_mols}: {err:.3e}"
    monkeypatch.setenv("DMPNN_STORE", "f32")
    with torch.no_grad():
        out_exact = mp(b)
    assert parity_err(out_exact.cpu().numpy(), ref.numpy()) <= TOL
    assert mp.__dict__.get("_dmpnn_route") == "fused16"


def test_a_launch_with_fewer_workgroups_than_the_plan_has_tiles_is_loud(gpu_device):
    """``dmpnn_fwd_args.n_tiles_launch`` may be an upper BOUND of the tile count (the module's steady path passes the batch's molecule
    count: a tile holds at least one molecule).  A bound that turns out too small must not leave rows nobody computed: every output NaN."""
    from chemprop_amd import engine, synth
    from chemprop_amd.nn import BondMessagePassing

    torch.manual_seed(5)
    mp = BondMessagePassing().eval().to(gpu_device)
    b = synth.random_batch(64, "qm9", seed=31)
    b.to(gpu_device)

    def run(n_launch):
        plan = engine.GraphPlan.from_bmg(b, light="tiles")
        plan.loader_tiles = n_launch   # (what engine.forward passes as n_tiles_launch; the plan itself came from the batch vector)
        with torch.no_grad():
            out, st = engine.forward(plan, b.V, b.E, mp.W_i.weight, mp.W_h.weight, mp.W_o.weight, mp.W_o.bias, depth=3, route="mega", mfma="split16")
        assert st.route == "mega16"
        n_tiles = int(plan.buf[6].item())   # DMPNN_HDR_NMTILES
        return out, n_tiles

    ref, n_tiles = run(0)
    assert 0 < n_tiles <= 64 and torch.isfinite(ref).all()
    exact, _ = run(n_tiles)
    assert torch.equal(exact, ref)                      # the exact count, and any bound above it (the molecule count): the same launch
    bound, _ = run(64)
    assert torch.equal(bound, ref)
    short, _ = run(n_tiles - 1)
    assert torch.isnan(short).all()


HALF_OPERANDS_TOL = 2e-3  # DMPNN_F_STORE16 on the tile route: operands, messages AND weights as one f16 per element (stated in include/dmpnn.h)


def test_half_operands_on_the_tile_kernel_golden(golden, gpu_device, monkeypatch):
    """``DMPNN_STORE=f16`` on the whole-forward tile kernel (round 6, ``k_mpnn_tile16<..., LP>``): every matrix product on the hi
    halves alone — one MFMA pass instead of three, half the weight stream.  Opt-in, not fp32-class: held to its own stated bar on
    every golden the tile route takes, deterministic, and NOT what runs by default."""
    cfg = golden.cfg
    if cfg.get("undirected") or cfg["d_h"] % 4 or cfg["d_h"] > 320 or golden["V"].shape[1] % 2 or golden["E"].shape[1] % 2 or "V_d" in golden:
        pytest.skip("tile route does not apply")
    if str(cfg["activation"]).lower() not in ("relu", "leakyrelu", "prelu", "tanh", "elu"):
        pytest.skip("custom activation: rows route")
    plan, out_exact, st = _engine_forward(golden, gpu_device, route="mega", mfma="split16")
    if not plan.fusable():
        pytest.skip("not a molecular graph")
    assert st.route == "mega16"
    assert parity_err(out_exact.cpu().numpy(), golden["out"]) <= TOL
    monkeypatch.setenv("DMPNN_STORE", "f16")
    _, out, st_h = _engine_forward(golden, gpu_device, route="mega", mfma="split16")
    assert st_h.route == "mega16/f16-operands"
    err = parity_err(out.cpu().numpy(), golden["out"])
    print(f"half operands {golden.name}: {err:.2e}")
    assert err <= HALF_OPERANDS_TOL, f"{golden.name}: {err:.3e}"
    if plan.n_edges and golden.name.startswith("qm9"):
        assert not torch.equal(out, out_exact)        # the flag did change the arithmetic (a molecule beyond the tile takes the generic fp32 path either way)
    _, out2, _ = _engine_forward(golden, gpu_device, route="mega", mfma="split16")
    assert torch.equal(out, out2)


@pytest.mark.parametrize("n_mols,kw", [(512, dict()), (64, dict()), (2048, dict(activation="tanh", bias=True)), (300, dict(d_h=128, depth=4))])
def test_half_operands_at_size(n_mols, kw, gpu_device, monkeypatch):
    """The module's own forward under ``DMPNN_STORE=f16`` at BASELINE's batch: the tile kernel's hi-halves form, against the oracle —
    and against the SAME oracle under torch's bf16 autocast (what ``configs[1]``'s "bf16" means for the reference): the f16 operands
    (11-bit significands) must not be further from fp32 than bf16's 8 bits are."""
    from chemprop_amd import synth
    from chemprop_amd.nn import BondMessagePassing
    from oracle import dmpnn_torch as ot

    torch.manual_seed(13)
    mp = BondMessagePassing(**kw).eval()
    b = synth.random_batch(n_mols, "qm9", seed=22)
    with torch.no_grad():
        w = ot.MPWeights.from_module(mp)
        ref = ot.forward_bmg(b, w, depth=mp.depth, activation=kw.get("activation", "relu"))
        with torch.autocast("cpu", dtype=torch.bfloat16):
            ref_bf16 = ot.forward_bmg(b, w, depth=mp.depth, activation=kw.get("activation", "relu")).float()
    err_bf16 = parity_err(ref_bf16.numpy(), ref.numpy())
    mp = mp.to(gpu_device)
    b.to(gpu_device)
    monkeypatch.setenv("DMPNN_STORE", "f16")
    with torch.no_grad():
        for _ in range(3):                            # past the validated first batches: the steady (replay) path
            out = mp(b)
    route = str(mp.__dict__.get("_dmpnn_route"))
    assert route.startswith("mega16"), route
    err = parity_err(out.cpu().numpy(), ref.numpy())
    print(f"half operands qm9-{n_mols} {kw}: {err:.2e} (the oracle under bf16 autocast: {err_bf16:.2e})")
    assert err <= HALF_OPERANDS_TOL, f"qm9-{n_mols}: {err:.3e}"
    assert err <= err_bf16, f"f16 operands {err:.3e} further from fp32 than bf16 autocast {err_bf16:.3e}"
    monkeypatch.setenv("DMPNN_STORE", "f32")
    with torch.no_grad():
        for _ in range(2):
            out_exact = mp(b)
    assert parity_err(out_exact.cpu().numpy(), ref.numpy()) <= TOL
    assert not torch.equal(out, out_exact)


@pytest.mark.parametrize("d_h,depth,act,bias,kind,n", [(384, 3, "relu", False, "zinc", 64), (448, 2, "tanh", True, "qm9", 160),
                                                       (512, 4, "leakyrelu", False, "synth40", 36), (640, 3, "elu", True, "cgr", 80),
                                                       (324, 3, "relu", False, "qm9", 160), (64, 1, "relu", False, "zinc", 64)])
def test_per_step_fused_route_wide_hidden_layers(d_h, depth, act, bias, kind, n, gpu_device):
    """d_h beyond the 320 columns of a 4-wave workgroup (hpopt searches 300-2400, cli/hpopt.py:73): 8-wave workgroups cover
    up to 640 columns, K1 runs on the update kernel over an operand split into rows first.  Against the oracle."""
    from chemprop_amd import synth
    from chemprop_amd.nn import BondMessagePassing

    dims = dict(d_v=106, d_e=28) if kind == "cgr" else {}
    bmg = synth.random_batch(n, kind, seed=d_h)   # (>= 2 048 directed edges: where the route rule takes the per-step fused route)
    assert bmg.E.shape[0] >= 2048
    torch.manual_seed(d_h)
    mp = BondMessagePassing(d_h=d_h, depth=depth, activation=act, bias=bias, **dims).eval()
    with torch.no_grad():
        ref = ot.forward_bmg(bmg, ot.MPWeights.from_module(mp), depth=depth, activation=act).numpy()
    mp = mp.to(gpu_device)
    bmg.to(gpu_device)
    with torch.no_grad():
        for i in range(3):
            out = mp(bmg)
            assert mp.__dict__.get("_dmpnn_route") == "fused16", mp.__dict__.get("_dmpnn_route")
            assert parity_err(out.cpu().numpy(), ref) <= TOL, (d_h, i)


def _closed_tile_mask(a, src, dst, rev, n_atoms):
    """What the tile kernel checks on a tile plan, in numpy: per atom, does its tile hold exactly its own edges
    (caller ids mtile_row[t] .. mtile_row[t+1]) with both atoms and the reverse edge inside the tile?"""
    n_t = int(a["hdr"][6])
    ok = np.ones(n_atoms, dtype=bool)
    mrow, matom = a["mtile_row"].numpy(), a["mtile_atom"].numpy()
    for t in range(n_t):
        e0, e1, a0, a1 = mrow[t], mrow[t + 1], matom[t], matom[t + 1]
        e = np.arange(e0, e1)
        good = ((src[e] >= a0) & (src[e] < a1) & (dst[e] >= a0) & (dst[e] < a1) & (rev[e] >= e0) & (rev[e] < e1)).all()
        ok[a0:a1] = good
    return ok


@pytest.mark.parametrize("use_batch", [False, True], ids=["pieces", "molecules"])
def test_tile_plan_and_forward_on_caller_order_edges(golden, use_batch, gpu_device):
    """dmpnn_prepare_tiles writes the same piece-tile tables as the full plan and nothing else; the tile kernel then
    works on the batch's own int64 index arrays (rows = edges in the caller's order) and gives the full-plan result;
    tiles that are not closed in the caller's edge order (shuffled edge layouts) return NaN for their atoms."""
    from chemprop_amd import engine
    from chemprop_amd.engine import GraphPlan, small_plan_fits

    cfg = golden.cfg
    if cfg.get("undirected") or cfg["d_h"] % 4 or cfg["d_h"] > 320 or golden["V"].shape[1] % 2 or golden["E"].shape[1] % 2:
        pytest.skip("fused routes do not apply")
    if str(cfg["activation"]).lower() not in ("relu", "leakyrelu", "prelu", "tanh", "elu"):
        pytest.skip("custom activation: rows route")
    bmg = golden.bmg(gpu_device)
    nV, nE = bmg.V.shape[0], bmg.E.shape[0]
    if not small_plan_fits(nV, nE):
        pytest.skip("batch beyond the single-workgroup plan")
    full = GraphPlan.from_bmg(bmg)
    lean = GraphPlan.from_bmg(bmg, light="tiles", use_batch=use_batch)  # tiles of connected pieces / of whole molecules (batch vector)
    assert lean.tiles_only
    af, al = full.arrays(), lean.arrays()
    assert al["hdr"][7] == 2 and (al["hdr"][0] & 16)
    if af["hdr"][0] & 2:  # indices out of range: both say so, nothing else is defined
        assert al["hdr"][0] & 2
        return
    if not use_batch:
        assert bool(al["hdr"][0] & 8) == bool(af["hdr"][0] & 8) and al["hdr"][6] == af["hdr"][6]
        assert torch.equal(al["mtile_row"], af["mtile_row"]) and torch.equal(al["mtile_atom"], af["mtile_atom"])
    else:  # molecules: every tile boundary is a molecule boundary, tiles hold <= 48 edges / <= 32 atoms and cover the batch
        n_t = int(al["hdr"][6])
        ma, mr = al["mtile_atom"].numpy(), al["mtile_row"].numpy()
        if not (al["hdr"][0] & 8):
            b = golden["batch"]
            assert ma[0] == 0 and ma[n_t] == nV and mr[0] == 0 and mr[n_t] == nE
            assert (np.diff(ma[:n_t + 1]) >= 0).all()
            assert all(v == 0 or v == nV or b[v] != b[v - 1] for v in ma[:n_t + 1])
            n_spill = 0
            for t in range(n_t):  # <= 48 edges / <= 32 atoms, or exactly ONE molecule beyond that
                if ma[t + 1] - ma[t] > 32 or mr[t + 1] - mr[t] > 48:
                    assert b[ma[t]] == b[ma[t + 1] - 1], "an oversize tile is one molecule"
                    n_spill += 1
            assert al["hdr"][8] == n_spill
    _, out_l, st = _engine_forward(golden, gpu_device, route="mega", keep=False, mfma="split16", plan=lean)
    assert st.route == "mega16"
    if al["hdr"][0] & 8:
        assert torch.isnan(out_l).all()
        return
    closed = _closed_tile_mask(al, golden["edge_index"][0], golden["edge_index"][1], golden["rev_edge_index"], nV)
    out_l = out_l.cpu().numpy()
    assert np.isnan(out_l[~closed]).all(), "atoms of a tile that is not closed must be NaN"
    if closed.any():
        assert parity_err(out_l[closed], golden["out"][closed]) <= TOL
        if not (af["hdr"][0] & (1 | 8)):
            _, out_f, _ = _engine_forward(golden, gpu_device, route="mega", keep=False, mfma="split16")
            assert parity_err(out_l[closed], out_f.cpu().numpy()[closed]) <= 3e-6
    assert closed.all() or "shuffled" in golden.name or "garbage" in golden.name, f"{golden.name}: unexpected open tiles"


def test_full_plan_with_molecule_tiles_beyond_the_single_workgroup_plan(gpu_device, monkeypatch):
    """dmpnn_prepare_with_batch: the FULL plan of a batch beyond the single-workgroup plan, with the molecule tiles of the
    batch-vector planner in it — the tables of the tile plan of the same batch (a tile's first edge in the caller's order
    IS its first row, collate.py:51-56), row_ptr-consistent; the same forward as the tile plan; training takes the tile
    kernels.  A batch whose edges are not in molecule order, or with a bond between two molecules, has no piece tiles
    (the tile kernels return NaN) and every other route is unaffected."""
    from chemprop_amd import engine, synth
    from chemprop_amd.engine import GraphPlan, small_plan_fits

    bmg = synth.random_batch(1024, "qm9", seed=21)
    bmg.to(gpu_device)
    nV, nE = bmg.V.shape[0], bmg.E.shape[0]
    assert not small_plan_fits(nV, nE)
    full = GraphPlan.from_bmg(bmg)
    lean = GraphPlan.from_bmg(bmg, light="tiles")
    assert full.any_size and not full.tiles_only and not full.light and lean.tiles_only
    af, al = full.arrays(), lean.arrays()
    assert af["hdr"][0] == 0 and af["hdr"][7] == 0 and al["hdr"][0] == 16
    assert af["hdr"][6] == al["hdr"][6] > 0 and af["hdr"][8] == al["hdr"][8] == 0
    assert torch.equal(af["mtile_row"], al["mtile_row"]) and torch.equal(af["mtile_atom"], al["mtile_atom"])
    n_t = int(af["hdr"][6])
    assert torch.equal(af["mtile_row"][:n_t + 1].long(), af["row_ptr"][af["mtile_atom"][:n_t + 1].long()].long())
    from oracle import collate_numpy as oc
    ei_h = bmg.edge_index.cpu().numpy()
    assert oc.full_plan_tiles_ok(ei_h[0], ei_h[1], nV, af["mtile_row"][:n_t + 1].numpy(), af["mtile_atom"][:n_t + 1].numpy())
    plain = GraphPlan.from_bmg(bmg, use_batch=False)   # (without the batch vector: the plain full plan, no molecule tiles)
    ap = plain.arrays()
    assert not plain.any_size and ap["hdr"][0] == 8 and ap["hdr"][6] == 0
    for k in ("src", "dst", "rev", "row_ptr", "perm", "inv", "srcp", "dstp", "revp", "tile_row", "tile_atom"):
        assert torch.equal(af[k], ap[k]), k
    torch.manual_seed(2)
    W = dict(W_i=torch.randn(300, bmg.V.shape[1] + bmg.E.shape[1]) * 0.1, W_h=torch.randn(300, 300) * 0.05,
             W_o=torch.randn(300, bmg.V.shape[1] + 300) * 0.05, b_o=torch.randn(300) * 0.1)
    W = {k: v.to(gpu_device) for k, v in W.items()}
    run = lambda plan, **kw: engine.forward(plan, bmg.V, bmg.E, W["W_i"], W["W_h"], W["W_o"], W["b_o"], None, None, depth=3, act="relu", **kw)
    out_t, st_t = run(lean, route="mega", mfma="split16")
    out_f, st_f = run(full, keep=True)
    out_g, st_g = run(plain, keep=True)
    assert st_t.route == st_f.route == "mega16" and st_g.route in ("general16", "fused")
    assert parity_err(out_t.cpu().numpy(), out_f.cpu().numpy()) <= 3e-6  # (rows of a tile in the caller's order vs in row order)
    assert parity_err(out_f.cpu().numpy(), out_g.cpu().numpy()) <= 3e-6

    # a bond between two molecules of different tiles: no piece tiles
    ei, rev, batch = bmg.edge_index.clone(), bmg.rev_edge_index.clone(), bmg.batch
    e = int(nE // 2)
    r = int(rev[e])
    far = int(af["mtile_atom"][n_t - 1])  # an atom of the last tile
    ei[0, e] = far
    ei[1, r] = far
    bad = GraphPlan(ei, rev, nV, batch=batch)
    assert bad.any_size and bad.flags() & 8
    assert not oc.full_plan_tiles_ok(ei[0].cpu().numpy(), ei[1].cpu().numpy(), nV, af["mtile_row"][:n_t + 1].numpy(), af["mtile_atom"][:n_t + 1].numpy())
    out_b, st_b = run(bad, keep=True, max_level=1)
    assert st_b.route in ("general16", "fused") and torch.isfinite(out_b).all()
    # the edges of the batch in another order (pairs kept): row ranges no longer match the caller-order edge ranges
    perm = torch.arange(nE, device=ei.device).view(-1, 2).flip(0).reshape(-1)
    inv = torch.empty_like(perm)
    inv[perm] = torch.arange(nE, device=ei.device)
    ei2, rev2 = bmg.edge_index[:, perm].contiguous(), inv[bmg.rev_edge_index[perm]].contiguous()
    bad2 = GraphPlan(ei2, rev2, nV, batch=batch)
    assert bad2.flags() & 8 and not bad2.flags() & 7


def test_module_switches_to_the_tile_plan_after_validation(gpu_device):
    from chemprop_amd import engine, synth
    from chemprop_amd.nn import BondMessagePassing, _tile_plan_ok

    torch.manual_seed(1)
    mp = BondMessagePassing().to(gpu_device).eval()
    outs = []
    with torch.no_grad():
        for i in range(4):
            bmg = synth.random_batch(64, "qm9", seed=50)
            bmg.to(gpu_device)
            outs.append(mp(bmg))
        assert mp._dmpnn_batches_checked >= 2 and _tile_plan_ok(mp, bmg.V.shape[0], bmg.E.shape[0], 64)
    assert parity_err(outs[3].cpu().numpy(), outs[0].cpu().numpy()) <= 3e-6   # full plan (validated) vs tile plan
    assert torch.equal(outs[2], outs[3])


@pytest.mark.parametrize("M,N,K", [(1, 1, 1), (5, 7, 3), (16, 64, 32), (33, 300, 300), (257, 300, 86),
                                   (130, 129, 372), (1000, 320, 45), (48, 2400, 100)])
def test_linear_kernel_vs_torch_fp32(M, N, K, gpu_device):
    """fp32-MFMA contraction (with an ASYMMETRIC W so a transposed tile cannot pass) vs torch fp32 on CPU."""
    from chemprop_amd import engine

    g = torch.Generator().manual_seed(M * 1000 + N * 10 + K)
    A = torch.randn(M, K, generator=g)
    W = torch.randn(N, K, generator=g) * (1 + torch.arange(N).float().unsqueeze(1) / N)
    b = torch.randn(N, generator=g)
    Cadd = torch.randn(M, N, generator=g)
    ref = torch.relu(Cadd.double() + (A.double() @ W.double().T + b.double())).float()
    out = engine.linear(A.to(gpu_device), W.to(gpu_device), b.to(gpu_device), Cadd=Cadd.to(gpu_device), act="relu")
    assert parity_err(out.cpu().numpy(), ref.numpy()) <= TOL


@pytest.mark.parametrize("M,N,K1,K2,gather", [(1, 2, 2, 0, False), (5, 7, 4, 2, False), (48, 64, 32, 0, False), (33, 300, 300, 0, False),
                                               (257, 300, 72, 14, True), (130, 130, 372, 0, False), (1000, 320, 46, 0, False),
                                               (100, 512, 512, 0, False), (49, 1000, 100, 28, True), (9120, 300, 300, 0, False)])
def test_split_linear_kernel_vs_torch_fp64(M, N, K1, K2, gather, gpu_device):
    """The per-step contraction on the f16 pipe with the exact 3-term split (dmpnn_linear16_fwd): bias, residual,
    activation, gather, concat, several 128-column operand groups and several column blocks — against fp64, held
    to the fp32 parity bar (and, where fp32 itself is the limit, at least as close as torch's fp32 product)."""
    from chemprop_amd import engine

    g = torch.Generator().manual_seed(M * 1000 + N * 10 + K1 + K2)
    n_src = 37 if gather else M
    A1 = torch.randn(n_src, K1, generator=g) * 3.0
    A2 = torch.randn(M, K2, generator=g) if K2 else None
    idx = torch.randint(0, n_src, (M,), generator=g).int() if gather else None
    W = torch.randn(N, K1 + K2, generator=g) * (1 + torch.arange(N).float().unsqueeze(1) / N)
    b = torch.randn(N, generator=g)
    Cadd = torch.randn(M, N, generator=g)
    rows = A1[idx.long()] if gather else A1
    A = torch.cat((rows, A2), 1) if K2 else rows
    ref = torch.relu(A.double() @ W.double().t() + b.double() + Cadd.double())
    d = gpu_device
    out = engine.linear(A1.to(d), W.to(d), b.to(d), A2=A2.to(d) if K2 else None, gather1=idx.to(d) if gather else None,
                        n_rows=M, Cadd=Cadd.to(d), act="relu", mfma="split16")
    err = parity_err(out.cpu().numpy(), ref.numpy())
    err32 = parity_err(torch.relu(A @ W.t() + b + Cadd).numpy(), ref.numpy())
    assert err <= max(TOL / 10, 2 * err32), f"{err:.3e} (torch fp32: {err32:.3e})"


@pytest.mark.parametrize("n_mols,kind,seed", [(512, "qm9", 0), (4096, "qm9", 1), (512, "synth40", 2), (512, "zinc", 3),
                                              (64, "cgr", 4), (512, "cgr", 5), (4096, "synth40", 6)])
def test_forward_full_size_vs_oracle(n_mols, kind, seed, gpu_device):
    """BASELINE.json sizes: batch of 512 QM9-shaped molecules (configs[1]), ZINC-shaped h 512 depth 6 (configs[2]), 40-atom
    molecules (configs[3]), condensed reaction graphs d_v 106 / d_e 28 at the notebook's 64 and at 512 (configs[4],
    featurizers/molgraph/reaction.py:77-78), against the CPU oracle."""
    from chemprop_amd import synth
    from chemprop_amd.nn import BondMessagePassing

    depth, d_h = (6, 512) if kind == "zinc" else (3, 300)
    bmg = synth.random_batch(n_mols, kind, seed=seed)
    torch.manual_seed(seed)
    dims = dict(d_v=106, d_e=28) if kind == "cgr" else {}
    mp = BondMessagePassing(d_h=d_h, depth=depth, **dims).eval()
    with torch.no_grad():
        ref = ot.forward_bmg(bmg, ot.MPWeights.from_module(mp), depth=depth)
    mp = mp.to(gpu_device)
    bmg.to(gpu_device)
    with torch.no_grad():
        out = mp(bmg)
    err = parity_err(out.cpu().numpy(), ref.numpy())
    from conftest import parity_err_unfloored

    err_u = parity_err_unfloored(out.cpu().numpy(), ref.numpy())
    print(f"{kind}-{n_mols}: max|out - ref| / max(1, max|ref|) = {err:.2e};  / max|ref| (un-floored) = {err_u:.2e};  max|ref| = {float(ref.abs().max()):.3g}")
    assert err <= TOL, f"{kind}-{n_mols}: {err:.3e}"
    assert err_u <= TOL, f"{kind}-{n_mols}: un-floored {err_u:.3e}"


@pytest.mark.parametrize("n_mols,kind,kw", [(4096, "qm9", {}), (512, "cgr", {}), (512, "synth40", {}),
                                            (512, "zinc", dict(d_h=512, depth=6))])   # BASELINE configs[2] at its own shape
def test_relu_gradients_at_size(n_mols, kind, kw, gpu_device):
    """ReLU gradients at BASELINE sizes (round-1 VERDICT: the at-size gradient cases used smooth activations).

    A kinked activation makes a gradient only as reproducible as its masks: ONE mask flip at |z| ~ 1e-7 moves a row of a
    weight gradient by 1e-3 of the largest entry — measured here for the engine AND for the reference's own fp32 (its
    gradients on the 40-atom batch are 4e-4 away from fp64 autograd of the same ops).  So the check has two halves:
      * the masks the engine's forward actually used (from its kept tensors) differ from the masks of the fp64 forward
        only where the fp64 pre-activation is within rounding of the kink, and only for a vanishing share of the entries;
      * GIVEN those masks the backward pass is linear algebra: the engine's gradients equal fp64 autograd with the same
        masks to 2e-5 (they come out at 1e-6)."""
    from chemprop_amd import synth
    from chemprop_amd.nn import BondMessagePassing

    dims = dict(dict(d_v=106, d_e=28) if kind == "cgr" else {}, **kw)
    h, n_upd = dims.get("d_h", 300), dims.get("depth", 3) - 1
    bmg = synth.random_batch(n_mols, kind, seed=13)
    torch.manual_seed(4)
    ref_mp = BondMessagePassing(**dims)
    nV, nE = bmg.V.shape[0], bmg.E.shape[0]
    G = torch.randn(nV, h, generator=torch.Generator().manual_seed(6))
    src, dst, rev = bmg.edge_index[0], bmg.edge_index[1], bmg.rev_edge_index
    V64, E64 = bmg.V.double(), bmg.E.double()

    def forward64(masks=None):
        """base.py:196-212 in fp64; ``masks`` replaces every ReLU by a fixed 0/1 factor (else records the true masks)."""
        ps = [p.detach().double().requires_grad_(True) for p in (ref_mp.W_i.weight, ref_mp.W_h.weight, ref_mp.W_o.weight, ref_mp.W_o.bias)]
        Wi, Wh, Wo, bo = ps
        pre, used = [], []

        def tau(z):
            pre.append(z.detach())
            m = (z.detach() > 0).double() if masks is None else masks[len(used)]
            used.append(m)
            return z * m

        H0 = torch.cat((V64[src], E64), 1) @ Wi.t()
        H = tau(H0)
        for _ in range(n_upd):
            S = torch.zeros(nV, h, dtype=torch.float64).index_add_(0, dst, H)
            H = tau(H0 + (S[src] - H[rev]) @ Wh.t())
        Mv = torch.zeros(nV, h, dtype=torch.float64).index_add_(0, dst, H)
        out = tau(torch.cat((V64, Mv), 1) @ Wo.t() + bo)
        return out, ps, pre, used

    mp = BondMessagePassing(**dims)
    mp.load_state_dict(ref_mp.state_dict())
    mp = mp.to(gpu_device).train()
    bmg.to(gpu_device)
    out = mp(bmg)
    st = out.grad_fn.st                                        # the kept tensors of this forward (FusedMP)
    rows = st.route in ("mega", "mega16", "fused", "fused16", "fused16/lean")  # kept edge tensors in CSR-row order (row i = edge perm[i])
    to_edges = (lambda X: X[st.plan.inv32.long()]) if rows else (lambda X: X)
    if st.route == "fused16/lean":   # (round 4: molecules beyond the tile train on the per-step fused route, which keeps SIGN BITS, not rows)
        from chemprop_amd import engine as _eng

        sb = _eng.lean_sign_bits(st)
        masks = [to_edges(sb[t]).double().cpu() for t in range(n_upd + 1)]
    else:
        masks = [(to_edges(st.H0[:, :h]) > 0).double().cpu()]
        masks += [(to_edges(st.Hs[t][:, :h]) > 0).double().cpu() for t in range(n_upd)]
    masks.append((out.detach() > 0).double().cpu())
    (out * G.to(gpu_device)).sum().backward()
    if kind == "qm9":  # beyond the single-workgroup plan: the full plan carries molecule tiles (dmpnn_prepare_with_batch)
        assert st.route == "mega16" and st.plan.any_size, st.route
    if kind in ("cgr", "synth40"):  # >= 20 000 directed edges, molecules beyond the tile, ReLU, d_h 300: the lean per-step fused route
        assert st.route == "fused16/lean", st.route

    o64, _, pre, true_masks = forward64()
    assert parity_err(out.detach().cpu().numpy(), o64.detach().numpy()) <= TOL
    total = flips = 0
    for z, m_true, m_eng in zip(pre, true_masks, masks):
        diff = m_true != m_eng
        total += diff.numel()
        flips += int(diff.sum())
        if diff.any():  # a differing mask sits on the kink: |z| within fp32 rounding of the values that were summed
            assert float(z[diff].abs().max()) <= 1e-5 * max(1.0, float(z.abs().max())), "a mask differs away from the kink"
    assert flips <= max(8, 2e-6 * total), f"{flips} mask flips of {total}"
    om, ps, _, _ = forward64(masks)
    (om * G.double()).sum().backward()
    got = [mp.W_i.weight.grad, mp.W_h.weight.grad, mp.W_o.weight.grad, mp.W_o.bias.grad]
    errs = {n: parity_err(g.cpu().numpy(), p.grad.numpy()) for n, g, p in zip(("W_i", "W_h", "W_o", "b_o"), got, ps)}
    print(f"{kind}-{n_mols} route={st.route} mask flips {flips}/{total}  gradient errors given the masks: {errs}")
    assert max(errs.values()) <= 2e-5, errs


def test_size_independent_properties_at_scale(gpu_device):
    """32 768 QM9-shaped molecules (E ~ 6e5, working set > Infinity Cache): properties that need no oracle.
      * conservation: column sums of Mv equal column sums of H (every edge has exactly one destination);
      * the message of a symmetric graph satisfies  sum_e M[e] = sum_v (deg(v) - 1) * S[v];
      * linearity: message(a*H + b*G) == a*message(H) + b*message(G) to rounding;
      * determinism: two runs are bit-identical (no atomics on the data path).
    """
    from chemprop_amd import engine, synth

    bmg = synth.random_batch(32768, "qm9", seed=7)
    bmg.to(gpu_device)
    plan = engine.GraphPlan.from_bmg(bmg)
    E = bmg.E.shape[0]
    g = torch.Generator(device=gpu_device).manual_seed(0)
    H = torch.randn(E, 300, device=gpu_device, generator=g)
    G = torch.randn(E, 300, device=gpu_device, generator=g)
    Mv = engine.aggregate(plan, H)
    assert parity_err(Mv.double().sum(0).cpu().numpy(), H.double().sum(0).cpu().numpy()) <= 1e-6
    M = engine.message(plan, H)
    deg = torch.bincount(bmg.edge_index[1], minlength=bmg.V.shape[0]).double().unsqueeze(1)
    lhs = M.double().sum(0)
    rhs = ((deg - 1) * Mv.double()).sum(0)
    assert parity_err(lhs.cpu().numpy(), rhs.cpu().numpy()) <= 1e-6
    M_lin = engine.message(plan, 0.5 * H - 2.0 * G)
    M_g = engine.message(plan, G)
    assert parity_err(M_lin.cpu().numpy(), (0.5 * M - 2.0 * M_g).cpu().numpy()) <= 1e-5
    assert torch.equal(engine.message(plan, H), M)


@pytest.mark.parametrize("kind,n_mols,kw,route", [("qm9", 32768, dict(), "mega16"), ("synth40", 8192, dict(), "fused16"),
                                                   ("zinc", 4096, dict(d_h=512, depth=6), "fused16")])
def test_whole_forward_properties_at_scale(kind, n_mols, kw, route, gpu_device):
    """The WHOLE forward at sizes no CPU oracle run is cheap for (0.6 M - 0.7 M directed edges), through properties the
    domain gives for free — molecules do not interact (no edge crosses a molecule, data/collate.py:48-56):
      * the atoms of the first 512 molecules get the same output inside the big batch as in a batch of their own, which IS
        checked against the oracle (tiles, row tiles and scales differ between the two: rounding class, <= 1e-5);
      * a permutation of the molecules permutes the output;
      * a checksum of checksums: the per-molecule output sums of the permuted batch match, molecule by molecule;
      * two runs are bit-identical (no atomics on the data path)."""
    from chemprop_amd import synth
    from chemprop_amd.data import BatchMolGraph
    from chemprop_amd.nn import BondMessagePassing

    mgs = synth.random_molgraphs(n_mols, kind, seed=31)
    torch.manual_seed(31)
    mp = BondMessagePassing(**kw).eval()
    head = BatchMolGraph(mgs[:512])
    with torch.no_grad():
        ref_head = ot.forward_bmg(head, ot.MPWeights.from_module(mp), depth=mp.depth).numpy()
    mp = mp.to(gpu_device)
    big = BatchMolGraph(mgs)
    perm = np.random.default_rng(5).permutation(n_mols)
    shuffled = BatchMolGraph([mgs[i] for i in perm])
    n_at = np.array([len(m.V) for m in mgs])
    off = np.concatenate([[0], np.cumsum(n_at)])
    for b in (head, big, shuffled):
        b.to(gpu_device)
    with torch.no_grad():
        for _ in range(3):                      # (past the synchronously validated first batches: the steady routes)
            out_head = mp(head)
        for _ in range(2):
            out_big = mp(big)
        assert str(mp.__dict__.get("_dmpnn_route") or route).startswith(route[:5]) or mp.__dict__.get("_dmpnn_replay") is not None
        out_shuf = mp(shuffled)
        assert torch.equal(mp(big), out_big)
    assert parity_err(out_head.cpu().numpy(), ref_head) <= TOL
    n_head = int(off[512])
    assert parity_err(out_big[:n_head].cpu().numpy(), ref_head) <= TOL
    # atom rows of molecule perm[j] in the shuffled batch = rows off[perm[j]] .. of the original
    idx = np.concatenate([np.arange(off[i], off[i + 1]) for i in perm])
    want = out_big.cpu().numpy()[idx]
    got = out_shuf.cpu().numpy()
    assert parity_err(got, want) <= TOL
    mol_of_atom = torch.from_numpy(np.repeat(np.arange(n_mols), n_at[perm])).to(gpu_device)
    sums_shuf = torch.zeros(n_mols, out_shuf.shape[1], device=gpu_device, dtype=torch.float64).index_add_(0, mol_of_atom, out_shuf.double())
    mol_of_atom0 = torch.from_numpy(np.repeat(np.arange(n_mols), n_at)).to(gpu_device)
    sums_big = torch.zeros(n_mols, out_big.shape[1], device=gpu_device, dtype=torch.float64).index_add_(0, mol_of_atom0, out_big.double())
    assert parity_err(sums_shuf.cpu().numpy(), sums_big[torch.from_numpy(perm).to(gpu_device)].cpu().numpy()) <= TOL


@pytest.mark.parametrize("warm", [3, 7, 8])
def test_steady_forward_under_hipgraph_capture(warm, gpu_device):
    """The steady inference forward is capture safe at ANY call count (the C ABI neither allocates nor synchronises; the spill
    monitor's occasional host copy must stay out of a capture): captured after `warm` eager calls, replayed, same bits."""
    from chemprop_amd import synth
    from chemprop_amd.nn import BondMessagePassing

    torch.manual_seed(9)
    mp = BondMessagePassing().eval().to(gpu_device)
    b = synth.random_batch(256, "qm9", seed=4)
    b.to(gpu_device)
    from chemprop_amd.data import BatchMolGraph

    b = BatchMolGraph.from_tensors(b.V, b.E, b.edge_index, b.rev_edge_index, b.batch, len(b))  # (bare tensors: the monitor is live)
    with torch.no_grad():
        side = torch.cuda.Stream(device=gpu_device)
        side.wait_stream(torch.cuda.current_stream(gpu_device))
        with torch.cuda.stream(side):
            for _ in range(warm):
                eager = mp(b)
        torch.cuda.current_stream(gpu_device).wait_stream(side)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            out = mp(b)
        g.replay()
        torch.cuda.synchronize(gpu_device)
        assert torch.equal(out, eager)
        g3 = torch.cuda.CUDAGraph()      # several steps as ONE graph (bench.py's K-steps-per-launch leg): every step keeps its own output
        with torch.cuda.graph(g3):
            outs = [mp(b) for _ in range(3)]
        g3.replay()
        torch.cuda.synchronize(gpu_device)
        assert all(torch.equal(o, eager) for o in outs) and len({o.data_ptr() for o in outs}) == 3
        for _ in range(20):
            assert torch.equal(mp(b), eager)      # and the eager path (monitor included) goes on working afterwards


def test_cpu_tensors_fail_loudly(gpu_device):
    from chemprop_amd import synth
    from chemprop_amd.nn import BondMessagePassing

    mp = BondMessagePassing(d_h=32)
    bmg = synth.random_batch(2, "qm9", seed=0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        mp(bmg)


def test_invalid_vd_shape_raises(gpu_device):
    from chemprop_amd import synth
    from chemprop_amd.nn import BondMessagePassing, InvalidShapeError

    mp = BondMessagePassing(d_h=32, d_vd=3).to(gpu_device)
    bmg = synth.random_batch(2, "qm9", seed=0)
    bmg.to(gpu_device)
    with pytest.raises(InvalidShapeError):
        mp(bmg, torch.zeros(bmg.V.shape[0], 4, device=gpu_device))


def test_custom_activation_and_dropout_rows_route(gpu_device):
    """Arbitrary nn.Module activation (reference tests use Softplus) and eval-mode dropout."""
    from chemprop_amd import synth
    from chemprop_amd.nn import BondMessagePassing

    bmg = synth.random_batch(8, "qm9", seed=5)
    torch.manual_seed(5)
    mp = BondMessagePassing(d_h=64, depth=4, activation=torch.nn.Softplus(), dropout=0.3).eval()
    with torch.no_grad():
        ref = ot.forward_bmg(bmg, ot.MPWeights.from_module(mp), depth=4, activation=torch.nn.functional.softplus)
    mp = mp.to(gpu_device)
    bmg.to(gpu_device)
    with torch.no_grad():
        out = mp(bmg)
    assert parity_err(out.cpu().numpy(), ref.numpy()) <= TOL


@pytest.mark.parametrize("n_mols,d_h,depth,bias", [(8, 64, 3, True), (8, 30, 2, False), (64, 64, 3, False)],
                         ids=["qm9x8-h64-bias", "qm9x8-h30-scalar-paths", "qm9x64-h64-wgrad-f16"])
def test_custom_activation_rows_route_gradients(n_mols, d_h, depth, bias, gpu_device):
    """An ``nn.Module`` activation in training mode: the block runs on the row-level autograd functions of
    ``chemprop_amd/backward.py`` (``dmpnn_linear_wgrad``, ``dmpnn_message_bwd``, ``dmpnn_aggregate_bwd`` and the forward kernels'
    transposes).  Every parameter gradient of ``(out * G).sum()`` against autograd through the oracle in float64, unfloored, with the
    float32 run of the same oracle as the yardstick (``rows_harness.compare``).  ``d_h = 30``: every row kernel on its scalar path;
    64 molecules: more than 1 024 edge rows, the weight gradients of ``W_i`` and ``W_h`` on the f16 pipe."""
    import rows_harness as rh
    from chemprop_amd import synth
    from chemprop_amd.nn import BondMessagePassing

    bmg = synth.random_batch(n_mols, "qm9", seed=5)
    assert (int(bmg.E.shape[0]) > 1024) == (n_mols == 64)
    torch.manual_seed(5)
    mp = BondMessagePassing(d_h=d_h, depth=depth, bias=bias, activation=torch.nn.Softplus(), dropout=0.0).train()
    G = torch.randn(int(bmg.V.shape[0]), d_h, generator=torch.Generator().manual_seed(6))
    names = [k for k, _ in mp.named_parameters()]

    def oracle(dtype):
        p = {k: v.detach().to(dtype).requires_grad_() for k, v in mp.named_parameters()}
        w = ot.MPWeights(p["W_i.weight"], p["W_h.weight"], p["W_o.weight"], p["W_o.bias"], p.get("W_i.bias"), p.get("W_h.bias"))
        out = ot.forward(bmg.V.to(dtype), bmg.E.to(dtype), bmg.edge_index, bmg.rev_edge_index, w, depth=depth,
                         activation=torch.nn.functional.softplus)
        (out * G.to(dtype)).sum().backward()
        return out.detach(), {k: v.grad for k, v in p.items()}

    out64, g64 = oracle(torch.float64)
    out32, g32 = oracle(torch.float32)
    mp = mp.to(gpu_device)
    bmg.to(gpu_device)
    out = mp(bmg)
    (out * G.to(gpu_device)).sum().backward()
    assert all(p.grad is not None for p in mp.parameters())
    got = {k: p.grad.cpu() for k, p in mp.named_parameters()}
    assert sorted(got) == sorted(names) and (("W_h.bias" in got) == bias)
    cid = f"softplus-rows-route-{n_mols}x-h{d_h}"
    fails = rh.compare(cid, dict(out=out.detach().cpu()), dict(out=out64), rh.yardstick(dict(out=out64), dict(out=out32)), "fwd")
    fails += rh.compare(cid, got, g64, rh.yardstick(g64, g32), "grad")
    assert not fails, "; ".join(fails)


# ------------------------------------------------------------------------------------------------
# K6: gradients
# ------------------------------------------------------------------------------------------------
def _check_grads(golden, named_grads, tol):
    checked = 0
    for key, g in named_grads.items():
        g = g.detach().cpu().numpy()
        if "g." + key in golden:
            err = parity_err(g, golden["g." + key])
            assert err <= tol, f"{golden.name}: d{key} {err:.3e}"
            checked += 1
        elif "gs." + key in golden:
            idx = np.random.default_rng(golden.meta["seed"]).choice(g.size, size=2048, replace=False)
            ref = golden["gs." + key]
            scale = max(1.0, float(golden["gsum." + key][1]) / g.size * 50)  # sampled: scale by the tensor's magnitude
            assert float(np.max(np.abs(g.ravel()[idx] - ref))) <= tol * max(scale, float(np.max(np.abs(ref)))), key
            checked += 1
    return checked


def test_backward_matches_executed_reference(golden, gpu_device):
    """Parameter gradients of sum(out * G) against autograd of the executed reference."""
    mp = golden.module(gpu_device).train()  # dropout p = 0 in every golden case
    bmg = golden.bmg(gpu_device)
    V_d = torch.from_numpy(golden["V_d"]).to(gpu_device) if "V_d" in golden else None
    G = torch.from_numpy(golden["G"]).to(gpu_device)
    out = mp(bmg, V_d)
    assert parity_err(out.detach().cpu().numpy(), golden["out"]) <= TOL
    (out * G).sum().backward()
    grads = {k: (p.grad if p.grad is not None else torch.zeros_like(p)) for k, p in mp.named_parameters()}
    if golden.name.startswith("garbage"):
        # not a molecular graph: the engine refuses (loudly, NaN) to differentiate through it
        assert torch.isnan(grads["W_h.weight"]).any() and torch.isnan(grads["W_i.weight"]).any()
        assert parity_err(grads["W_o.weight"].cpu().numpy(), golden["g.W_o.weight"]) <= TOL
        return
    assert _check_grads(golden, grads, 2e-5) >= 4


@pytest.mark.parametrize("n_mols,kind,kw", [
    (512, "qm9", dict()),
    (2048, "qm9", dict(activation="tanh", bias=True)),   # beyond the single-workgroup plan: tile kernels on a full plan with tiles
    # (smooth activation: at this size a single ReLU mask flip at |z| ~ 1e-8 between two fp32-class arithmetics moves
    #  a bias-gradient entry by ~1e-3 of the largest one, which says nothing about the kernels)
    (256, "synth40", dict(bias=True, undirected=True, activation="tanh")),
    (64, "zinc", dict(d_h=128, depth=5, activation="elu")),
    (512, "zinc", dict(d_h=512, depth=6, activation="tanh")),              # BASELINE configs[2] at its own shape (d_h > 320 training route)
    (64, "qm9", dict(d_h=96, depth=4, activation=torch.nn.Softplus())),   # rows route (custom module)
    (64, "qm9", dict(d_h=64, activation="prelu")),                         # rows route (learnable slope)
])
def test_backward_full_size_vs_oracle_autograd(n_mols, kind, kw, gpu_device):
    from chemprop_amd import synth
    from chemprop_amd.nn import BondMessagePassing

    bmg = synth.random_batch(n_mols, kind, seed=11)
    torch.manual_seed(3)
    ref_mp = BondMessagePassing(**kw)
    mp = BondMessagePassing(**kw)
    mp.load_state_dict(ref_mp.state_dict())
    act = kw.get("activation", "relu")
    G = torch.randn(bmg.V.shape[0], ref_mp.output_dim, generator=torch.Generator().manual_seed(5))
    w = ot.MPWeights(ref_mp.W_i.weight, ref_mp.W_h.weight, ref_mp.W_o.weight, ref_mp.W_o.bias,
                     ref_mp.W_i.bias, ref_mp.W_h.bias)
    act_fn = ref_mp.tau if isinstance(act, torch.nn.Module) or act == "prelu" else act
    ref = ot.forward_bmg(bmg, w, depth=ref_mp.depth, activation=act_fn, undirected=ref_mp.undirected)
    (ref * G).sum().backward()
    mp = mp.to(gpu_device).train()
    bmg.to(gpu_device)
    out = mp(bmg)
    (out * G.to(gpu_device)).sum().backward()
    assert parity_err(out.detach().cpu().numpy(), ref.detach().numpy()) <= TOL
    for (k, p), (_, q) in zip(mp.named_parameters(), ref_mp.named_parameters()):
        err = parity_err(p.grad.cpu().numpy(), q.grad.numpy())
        assert err <= 2e-5, f"{k}: {err:.3e}"


@pytest.mark.parametrize("d_h,depth,act,bias,kind,n_mols", [(800, 3, "tanh", False, "qm9", 128), (1200, 2, "tanh", True, "qm9", 160),
                                                            (2400, 2, "elu", False, "synth40", 48), (1200, 3, "relu", False, "zinc", 64)])
def test_hpopt_hidden_widths_forward_and_gradients(d_h, depth, act, bias, kind, n_mols, gpu_device):
    """The widths the reference's own hyper-parameter search reaches (cli/hpopt.py:73: message_hidden_dim 300 .. 2400 in steps of
    100; base.py:238-251 for the shapes): beyond the 640 columns of the per-step fused kernels the route rule takes the general
    route with its contractions on the f16 pipe (k_rows16, 256-column blocks).  The whole forward (eval) AND the training forward +
    every parameter gradient against the oracle and its autograd, at the same bars as everywhere else.  (Smooth activations for
    the gradient cases — a ReLU mask flip at |z| ~ 1e-8 says nothing about the kernels, test_relu_gradients_at_size — and one ReLU
    case, forward only.)"""
    from chemprop_amd import synth
    from chemprop_amd.nn import BondMessagePassing

    bmg = synth.random_batch(n_mols, kind, seed=d_h + depth)
    torch.manual_seed(d_h)
    kw = dict(d_h=d_h, depth=depth, activation=act, bias=bias)
    ref_mp = BondMessagePassing(**kw)
    mp = BondMessagePassing(**kw)
    mp.load_state_dict(ref_mp.state_dict())
    G = torch.randn(bmg.V.shape[0], d_h, generator=torch.Generator().manual_seed(5))
    w = ot.MPWeights(ref_mp.W_i.weight, ref_mp.W_h.weight, ref_mp.W_o.weight, ref_mp.W_o.bias, ref_mp.W_i.bias, ref_mp.W_h.bias)
    ref = ot.forward_bmg(bmg, w, depth=depth, activation=act)
    mp = mp.to(gpu_device)
    bmg.to(gpu_device)
    with torch.no_grad():
        out_eval = mp.eval()(bmg)
    assert mp.__dict__.get("_dmpnn_route") == "general16", mp.__dict__.get("_dmpnn_route")
    assert parity_err(out_eval.cpu().numpy(), ref.detach().numpy()) <= TOL, (d_h, "eval")
    if act == "relu":
        return
    (ref * G).sum().backward()
    out = mp.train()(bmg)
    (out * G.to(gpu_device)).sum().backward()
    assert parity_err(out.detach().cpu().numpy(), ref.detach().numpy()) <= TOL, (d_h, "train")
    for (k, p_), (_, q) in zip(mp.named_parameters(), ref_mp.named_parameters()):
        err = parity_err(p_.grad.cpu().numpy(), q.grad.numpy())
        assert err <= 2e-5, f"d_h {d_h} {k}: {err:.3e}"


@pytest.mark.parametrize("n_mols,act,depth,d_h,mixed", [(512, "relu", 3, 300, False), (200, "leakyrelu", 4, 128, False), (96, "relu", 2, 64, False),
                                                       (40, "relu", 3, 300, True), (64, "relu", 1, 300, False)])
def test_kept_sign_bits_give_the_same_gradients_as_kept_rows(n_mols, act, depth, d_h, mixed, gpu_device):
    """dmpnn_fwd_args.keep_bits: on a tile plan with a ReLU-class activation the training forward keeps H0 / H^(t) as ONE bit per
    element ([x > 0], straight from the matrix-pipe fragments) instead of fp32 rows.  tau' only ever looked at that sign: every
    gradient is BIT-IDENTICAL to the run that kept the rows — at any size, kinks or not (a molecule beyond the tile keeps fp32 rows
    either way: the kernels' generic path)."""
    from chemprop_amd import engine, synth
    from chemprop_amd.nn import BondMessagePassing

    bmg = _mixed_batch(n_mols, "synth40", 33) if mixed else synth.random_batch(n_mols, "qm9", seed=33)
    bmg.to(gpu_device)
    torch.manual_seed(8)
    mp = BondMessagePassing(d_h=d_h, depth=depth, activation=act, bias=True).to(gpu_device)
    slope = 0.1 if act == "leakyrelu" else 0.0
    G = torch.randn(bmg.V.shape[0], d_h, device=gpu_device)
    need = {k: True for k in ("W_i", "b_i", "W_h", "b_h", "W_o", "b_o")}
    res = []
    for bits in (True, False):
        plan = engine.GraphPlan.from_bmg(bmg, light="tiles")
        assert plan.tiles_only
        out, st = engine.forward(plan, bmg.V, bmg.E, mp.W_i.weight, mp.W_h.weight, mp.W_o.weight, mp.W_o.bias, mp.W_i.bias, mp.W_h.bias,
                                 depth=depth, act=act, slope=slope, keep=True, keep_bits=bits)
        assert st.route == "mega16" and bool(st.args.keep_bits) == bits
        grads = engine.backward(st, G, need)
        grads = grads[0] if isinstance(grads, tuple) else grads
        torch.cuda.synchronize()
        res.append((out.clone(), {k: v.clone() for k, v in grads.items() if v is not None}))
    assert torch.equal(res[0][0], res[1][0])
    for k in res[1][1]:
        assert torch.isfinite(res[0][1][k]).all(), k
        assert torch.equal(res[0][1][k], res[1][1][k]), k


def _mixed_batch(n_small, big_kind, seed):
    """QM9-shaped molecules with ONE molecule beyond the tile in the middle, as bare tensors (``oversize`` unknown to the host)."""
    from chemprop_amd import synth
    from chemprop_amd.data import BatchMolGraph

    mgs = synth.random_molgraphs(n_small, "qm9", seed=seed)
    mgs.insert(n_small // 2, synth.random_molgraphs(1, big_kind, seed=seed + 1)[0])
    b = BatchMolGraph(mgs)
    return BatchMolGraph.from_tensors(b.V, b.E, b.edge_index, b.rev_edge_index, b.batch, len(mgs))


@pytest.mark.parametrize("case,kw", [
    ("qm9-512", dict(activation="elu")),
    ("qm9-96", dict(d_h=64, depth=4, activation="leakyrelu", bias=True)),
    ("qm9-2048", dict(activation="tanh", bias=True)),      # beyond the single-workgroup plan: the tile table from the batch vector
    ("qm9-200-depth1", dict(depth=1, activation="elu")),
    ("mixed-40+1", dict(activation="tanh")),               # a molecule beyond the tile: the kernels' generic path, forward and backward
    ("shuffled-rev-64", dict(activation="tanh", bias=True)),  # rev is NOT an involution inside the molecules: exact all the same
])
def test_training_on_the_tile_plan(case, kw, gpu_device, monkeypatch):
    """DMPNN_F_TILE_PLAN: a training forward + backward whose K0 is the tile table alone — kept tensors in the caller's edge order,
    src / dst / rev of a tile read from the batch's own arrays by both tile kernels, the caller's src array as the gather of W_i's
    weight-gradient operand.  Output and every gradient against the oracle's autograd, and against the same step on the full
    (CSR) plan."""
    from chemprop_amd import _lib, synth
    from chemprop_amd.nn import BondMessagePassing

    monkeypatch.setenv("DMPNN_VALIDATE", "never")   # (the first batches of a module are validated on full plans)
    if case.startswith("mixed"):
        bmg = _mixed_batch(40, "synth40", 21)
    else:
        bmg = synth.random_batch({"qm9-512": 512, "qm9-96": 96, "qm9-2048": 2048, "qm9-200-depth1": 200, "shuffled-rev-64": 64}[case], "qm9", seed=12)
    if case.startswith("shuffled"):
        # a rev map that permutes the edges of each molecule at random (closed inside the molecule, not an involution, src(rev e) != dst e)
        g = torch.Generator().manual_seed(2)
        e_mol = bmg.batch[bmg.edge_index[0]]
        rev = bmg.rev_edge_index.clone()
        for m in range(len(bmg)):
            idx = (e_mol == m).nonzero().flatten()
            rev[idx] = idx[torch.randperm(idx.numel(), generator=g)]
        from chemprop_amd.data import BatchMolGraph
        bmg = BatchMolGraph.from_tensors(bmg.V, bmg.E, bmg.edge_index, rev, bmg.batch, len(bmg))
    torch.manual_seed(4)
    ref_mp = BondMessagePassing(**kw)
    G = torch.randn(bmg.V.shape[0], ref_mp.output_dim, generator=torch.Generator().manual_seed(6))
    w = ot.MPWeights(ref_mp.W_i.weight, ref_mp.W_h.weight, ref_mp.W_o.weight, ref_mp.W_o.bias, ref_mp.W_i.bias, ref_mp.W_h.bias)
    ref = ot.forward_bmg(bmg, w, depth=ref_mp.depth, activation=kw.get("activation", "relu"))
    (ref * G).sum().backward()
    bmg.to(gpu_device)
    Gd = G.to(gpu_device)
    res = {}
    for plan_kind in ("tiles", "full"):
        if case.startswith("shuffled") and plan_kind == "full":
            continue   # (the CSR plan's kernels assume a molecular graph and say NaN otherwise: nothing to compare)
        monkeypatch.setenv("DMPNN_TRAIN_PLAN", plan_kind)
        mp = BondMessagePassing(**kw)
        mp.load_state_dict(ref_mp.state_dict())
        mp = mp.to(gpu_device).train()
        out = mp(bmg)
        st = out.grad_fn.st
        assert st.route == "mega16" and bool(st.plan.tiles_only) == (plan_kind == "tiles")
        assert bool(st.args.flags & _lib.F_TILE_PLAN) == (plan_kind == "tiles")
        (out * Gd).sum().backward()
        res[plan_kind] = (out.detach().cpu().numpy(), {k: p.grad.cpu().numpy() for k, p in mp.named_parameters()})
        assert parity_err(res[plan_kind][0], ref.detach().numpy()) <= TOL, plan_kind
        for k, q in ref_mp.named_parameters():
            if q.grad is None:   # (depth 1: W_h takes no part)
                continue
            err = parity_err(res[plan_kind][1][k], q.grad.numpy())
            assert err <= 2e-5, f"{plan_kind} {k}: {err:.3e}"
    if "full" in res:
        assert parity_err(res["tiles"][0], res["full"][0]) <= 2e-6
        for k in res["full"][1]:
            assert parity_err(res["tiles"][1][k], res["full"][1][k]) <= 5e-6, k


@pytest.mark.parametrize("n_mols,kind,kw", [(96, "synth40", dict(activation="tanh", bias=True)), (64, "zinc", dict(d_h=512, depth=4, activation="elu")),
                                            (200, "qm9", dict(depth=1, activation="elu"))])   # (smooth activations: kinks are test_relu_gradients_at_size's)
def test_training_forward_on_the_per_step_fused_route(n_mols, kind, kw, gpu_device):
    """DMPNN_F_FUSED | DMPNN_F_SPLIT16 | DMPNN_F_KEEP (on demand, ``route="fused16"``): k_step16 keeps H^(t) and an fp32 copy of each
    message beside the split rows; dmpnn_backward reads them in the plan's row order.  Output and every gradient against the
    general route of the same build (both fp32-class) and against the restated reference."""
    from chemprop_amd import engine, synth
    from chemprop_amd.nn import BondMessagePassing, classify_activation

    bmg = synth.random_batch(n_mols, kind, seed=19)
    torch.manual_seed(6)
    ref_mp = BondMessagePassing(**kw)
    G = torch.randn(bmg.V.shape[0], ref_mp.output_dim, generator=torch.Generator().manual_seed(8))
    w = ot.MPWeights(ref_mp.W_i.weight, ref_mp.W_h.weight, ref_mp.W_o.weight, ref_mp.W_o.bias, ref_mp.W_i.bias, ref_mp.W_h.bias)
    ref = ot.forward_bmg(bmg, w, depth=ref_mp.depth, activation=kw.get("activation", "relu"))
    (ref * G).sum().backward()
    mp = BondMessagePassing(**kw)
    mp.load_state_dict(ref_mp.state_dict())
    mp = mp.to(gpu_device)
    bmg.to(gpu_device)
    act, slope, slope_t = classify_activation(mp.tau)
    need = dict(W_i=True, b_i=mp.W_i.bias is not None, W_h=True, b_h=mp.W_h.bias is not None, W_o=True, b_o=True)
    got = {}
    for route in ("fused16", "general"):
        plan = engine.GraphPlan.from_bmg(bmg)
        out, st = engine.forward(plan, bmg.V, bmg.E, mp.W_i.weight, mp.W_h.weight, mp.W_o.weight, mp.W_o.bias, mp.W_i.bias, mp.W_h.bias,
                                 depth=mp.depth, act=act, slope=slope, keep=True, route=route, keep_bits=False)   # (keep_bits=False: the fp32-copies form)
        assert st.route == ("fused16" if route == "fused16" else st.route) and (route != "fused16" or st.args.msplit)
        got[route] = (out, engine.backward(st, G.to(gpu_device), need))
    out16, g16 = got["fused16"]
    outg, gg = got["general"]
    assert parity_err(out16.detach().cpu().numpy(), ref.detach().numpy()) <= TOL
    assert parity_err(out16.detach().cpu().numpy(), outg.detach().cpu().numpy()) <= 3e-6
    names = dict(W_i=ref_mp.W_i.weight, b_i=ref_mp.W_i.bias, W_h=ref_mp.W_h.weight, b_h=ref_mp.W_h.bias, W_o=ref_mp.W_o.weight, b_o=ref_mp.W_o.bias)
    for k, p in names.items():
        if p is None or g16[k] is None or p.grad is None:   # (depth 1: W_h takes no part)
            continue
        e_ref = parity_err(g16[k].cpu().numpy(), p.grad.numpy())
        e_gen = parity_err(g16[k].cpu().numpy(), gg[k].cpu().numpy())
        assert e_ref <= 2e-5 and e_gen <= 2e-5, f"{k}: vs reference {e_ref:.2e}, vs general route {e_gen:.2e}"


def test_every_weight_update_is_seen_also_through_param_data(gpu_device):
    """Nothing about the weights is cached between forwards (round 4: the f16 pre-split rides in K0's launch, every call): an update
    through the tensor API, ``load_state_dict`` AND a write through ``param.data`` — which bumps no autograd version: the EMA / SWA
    swap that went stale silently behind rounds 1-3's version-keyed cache — change the very next forward, on the steady (replayed)
    path and on the slow path alike."""
    from chemprop_amd import synth
    from chemprop_amd.nn import BondMessagePassing

    bmg = synth.random_batch(16, "qm9", seed=5)
    bmg.to(gpu_device)
    torch.manual_seed(3)
    mp = BondMessagePassing(d_h=300).to(gpu_device).eval()

    def fresh_out():
        f = BondMessagePassing(d_h=300).to(gpu_device).eval()
        f.load_state_dict(mp.state_dict())
        return f(bmg)

    with torch.no_grad():
        for _ in range(4):   # validated batches, then the steady path
            a = mp(bmg)
        assert mp.__dict__.get("_dmpnn_replay") is not None and torch.equal(a, mp(bmg))
        mp.W_h.weight.mul_(1.5)                       # the tensor API
        c = mp(bmg)
        assert not torch.equal(a, c) and parity_err(c.cpu().numpy(), fresh_out().cpu().numpy()) <= 3e-6
        v = mp.W_o.weight._version
        mp.W_o.weight.data.mul_(0.5)                  # through .data: no version bump
        mp.W_i.weight.data.add_(0.01)
        assert mp.W_o.weight._version == v
        d = mp(bmg)
        assert mp.__dict__.get("_dmpnn_replay") is not None          # (still the steady path)
        assert not torch.equal(c, d) and parity_err(d.cpu().numpy(), fresh_out().cpu().numpy()) <= 3e-6
        ema = {k: t * 0.9 for k, t in mp.state_dict().items()}
        for k, p in mp.named_parameters():            # an EMA swap the way callbacks do it
            p.data.copy_(ema[k])
        e = mp(bmg)
        assert parity_err(e.cpu().numpy(), fresh_out().cpu().numpy()) <= 3e-6 and not torch.equal(d, e)


def test_frozen_encoder_and_no_grad(gpu_device):
    """requires_grad_(False) on the block (cli/train.py:1826-1828) and torch.no_grad() both work."""
    from chemprop_amd import synth
    from chemprop_amd.nn import BondMessagePassing

    bmg = synth.random_batch(8, "qm9", seed=2)
    bmg.to(gpu_device)
    mp = BondMessagePassing(d_h=32).to(gpu_device)
    mp.W_i.requires_grad_(False)
    mp.W_h.requires_grad_(False)
    out = mp(bmg)
    out.sum().backward()
    assert mp.W_i.weight.grad is None and mp.W_h.weight.grad is None and mp.W_o.weight.grad is not None
    mp.requires_grad_(False)
    assert not mp(bmg).requires_grad


def test_overfit_small_regression(gpu_device):
    """Analogue of tests/integration/test_regression_mol.py:56-89: the gradients are good enough to train."""
    from chemprop_amd import synth
    from chemprop_amd.nn import BondMessagePassing

    torch.manual_seed(0)
    bmg = synth.random_batch(48, "qm9", seed=9)
    bmg.to(gpu_device)
    y = torch.randn(48, 1, device=gpu_device)
    mp = BondMessagePassing(d_h=64).to(gpu_device)
    head = torch.nn.Linear(64, 1).to(gpu_device)
    opt = torch.optim.Adam(list(mp.parameters()) + list(head.parameters()), lr=3e-3)
    n_mols = len(bmg)
    losses = []
    for _ in range(300):
        opt.zero_grad()
        Hv = mp(bmg)
        pooled = torch.zeros(n_mols, 64, device=gpu_device).index_add_(0, bmg.batch, Hv)
        pooled = pooled / torch.bincount(bmg.batch, minlength=n_mols).unsqueeze(1)
        loss = torch.nn.functional.mse_loss(head(pooled), y)
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    assert losses[-1] <= 0.05 and losses[-1] < 0.1 * losses[0], (losses[0], losses[-1])


@pytest.mark.parametrize("mode", ["never", "always", "first"])
def test_validate_modes_give_the_same_function(mode, gpu_device, monkeypatch):
    """DMPNN_VALIDATE decides when the plan's verdict is read (and which plan a forward builds), not the result:
    `never` takes the tile plan from the first batch on, `always` keeps reading a full / light plan."""
    from chemprop_amd import synth
    from chemprop_amd.nn import BondMessagePassing
    from oracle import dmpnn_torch as ot

    monkeypatch.setenv("DMPNN_VALIDATE", mode)
    bmg = synth.random_batch(96, "qm9", seed=31)
    torch.manual_seed(4)
    mp = BondMessagePassing().eval()
    with torch.no_grad():
        ref = ot.forward_bmg(bmg, ot.MPWeights.from_module(mp), depth=mp.depth).numpy()
    mp = mp.to(gpu_device)
    bmg.to(gpu_device)
    with torch.no_grad():
        for i in range(4):
            assert parity_err(mp(bmg).cpu().numpy(), ref) <= TOL, (mode, i)
    replay = mp.__dict__.get("_dmpnn_replay") is not None
    assert replay == (mode != "always")  # the steady tile-plan path exists unless every batch is validated
    assert getattr(mp, "_dmpnn_batches_checked", 0) == {"never": 0, "always": 4, "first": 2}[mode]


# ------------------------------------------------------------------------------------------------
# round 4: training of molecules beyond the tile on the per-step FUSED route — the lean forward + the backward step kernels
# ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("n_mols,kind,kw", [(48, "synth40", dict(d_h=64)),
                                            (24, "zinc", dict(d_h=128, depth=4, bias=True, activation="leakyrelu")),
                                            (40, "cgr", dict(d_v=106, d_e=28, d_h=96, depth=2)),
                                            (64, "qm9", dict(d_h=300)),
                                            (300, "synth40", dict(d_h=300))])
def test_lean_fused16_training_route_matches_the_general_route(n_mols, kind, kw, gpu_device):
    """``route="fused16"`` with ``keep`` (ReLU-class activation): split message rows of every step + sign bits are all the forward
    keeps; ``dmpnn_backward`` runs the backward step kernels (csrc/dmpnn_bstep16.hip) and the weight-gradient products on operands
    written tile by tile.  Output, the kept signs and every gradient against the per-step GENERAL route (fp32 MFMA: the reference's
    op order) on the same batch, and the gradients against the oracle's autograd."""
    from chemprop_amd import engine, synth
    from chemprop_amd.nn import BondMessagePassing, classify_activation

    bmg = synth.random_batch(n_mols, kind, seed=17)
    torch.manual_seed(8)
    cpu = BondMessagePassing(**kw)
    mp = BondMessagePassing(**kw)
    mp.load_state_dict(cpu.state_dict())
    mp = mp.to(gpu_device)
    bmg.to(gpu_device)
    act, slope, _ = classify_activation(mp.tau)
    W = lambda l, n: getattr(getattr(mp, l), n)
    args = (bmg.V, bmg.E, W("W_i", "weight"), W("W_h", "weight"), W("W_o", "weight"), W("W_o", "bias"), W("W_i", "bias"), W("W_h", "bias"))
    plan = engine.GraphPlan.from_bmg(bmg)
    G = torch.randn(int(bmg.V.shape[0]), mp.output_dim, generator=torch.Generator().manual_seed(3)).to(gpu_device)
    need = dict(W_i=True, b_i=True, W_h=True, b_h=True, W_o=True, b_o=True)
    o_gen, st_gen = engine.forward(plan, *args, depth=mp.depth, act=act, slope=slope, keep=True, route="general", mfma="f32")
    g_gen = engine.backward(st_gen, G, need)
    o_lean, st = engine.forward(plan, *args, depth=mp.depth, act=act, slope=slope, keep=True, route="fused16")
    assert st.route == "fused16/lean", st.route
    g_lean = engine.backward(st, G, need)
    torch.cuda.synchronize()
    assert parity_err(o_lean.cpu().numpy(), o_gen.cpu().numpy()) <= TOL
    # the kept signs against the general route's kept tensors (caller's edge order there, CSR rows here)
    h = mp.W_h.weight.shape[0]
    sb = engine.lean_sign_bits(st)[:, st.plan.inv32.long()]
    ref_pos = [st_gen.H0[:, :h] > 0] + [st_gen.Hs[t][:, :h] > 0 for t in range(mp.depth - 1)]
    flips = sum(int((sb[t] != ref_pos[t]).sum()) for t in range(mp.depth))
    assert flips <= 2, flips   # (two arithmetics: a pre-activation within rounding of the kink may land on either side)
    errs = {k: parity_err(g_lean[k].cpu().numpy(), g_gen[k].cpu().numpy()) for k in g_gen if g_gen[k] is not None}
    print(f"lean-{kind}-{n_mols}: sign flips {flips}, gradient errors vs the general route {errs}")
    if flips == 0:
        assert max(errs.values()) <= 2e-5, errs
    # ... and against the oracle's autograd (the restated ATen op sequence on the CPU)
    w = ot.MPWeights(cpu.W_i.weight, cpu.W_h.weight, cpu.W_o.weight, cpu.W_o.bias, cpu.W_i.bias, cpu.W_h.bias)
    cb = synth.random_batch(n_mols, kind, seed=17)
    ref = ot.forward_bmg(cb, w, depth=cpu.depth, activation=cpu.tau)   # (a callable: the module's own activation)
    (ref * G.cpu()).sum().backward()
    assert parity_err(o_lean.cpu().numpy(), ref.detach().numpy()) <= TOL
    if flips == 0:
        for k, prm in (("W_i", cpu.W_i.weight), ("W_h", cpu.W_h.weight), ("W_o", cpu.W_o.weight), ("b_o", cpu.W_o.bias)):
            assert parity_err(g_lean[k].cpu().numpy(), prm.grad.numpy()) <= 2e-5, k


@pytest.mark.gpu
def test_lean_fused16_is_the_default_for_training_at_size_and_repeats(gpu_device):
    """The route rule: a TRAINING forward of >= 20 000 directed edges whose molecules exceed the tile (40-atom molecules: BASELINE
    configs[3]) takes the lean per-step fused route by default; two backward passes give bit-identical gradients (no atomics); a
    tanh block (not a ReLU-class activation) keeps the per-step general route."""
    from chemprop_amd import synth
    from chemprop_amd.nn import BondMessagePassing

    bmg = synth.random_batch(512, "synth40", seed=2)
    bmg.to(gpu_device)
    torch.manual_seed(0)
    mp = BondMessagePassing().to(gpu_device).train()
    G = torch.randn(int(bmg.V.shape[0]), 300, device=gpu_device)
    grads = []
    for _ in range(3):
        mp.zero_grad()
        out = mp(bmg)
        assert out.grad_fn.st.route == "fused16/lean", out.grad_fn.st.route
        out.backward(G)
        grads.append([p.grad.clone() for p in mp.parameters()])
    torch.cuda.synchronize()
    assert all(torch.isfinite(g).all() for g in grads[-1])
    assert all(torch.equal(a, b) for a, b in zip(grads[1], grads[2]))
    mp2 = BondMessagePassing(activation="tanh").to(gpu_device).train()
    assert mp2(bmg).grad_fn.st.route == "general16"


@pytest.mark.parametrize("case,kw", [
    ("qm9-512", dict(activation="tanh", bias=True)),       # bias gradients = column sums of the gradient rows (jobs of the same launch)
    ("qm9-512", dict()),                                    # ReLU, sign bits
    ("qm9-96", dict(d_h=64, depth=4, activation="elu")),
    ("mixed-40+1", dict(activation="tanh")),                # a molecule beyond the tile: its fp32 rows converted at the end of its tile
    ("qm9-300-masked", dict(activation="tanh", bias=True)),  # half of the atoms without gradient, the rest at 1e-6: all-zero tiles beside tiny ones
    ("qm9-256-fullplan", dict(activation="elu", bias=True)),  # the CSR plan: kept rows in the plan's row order, the operands gathered through it
    ("qm9-128-vd", dict(activation="tanh", d_vd=3)),          # W_d behind the finalize (full plan): gHO comes through W_d's transpose first
], ids=["qm9-512-tanh-bias", "qm9-512-relu", "qm9-96-d4-h64", "mixed-40+1", "masked-tiny-gradients", "full-plan", "with-W_d"])
def test_tile_kernels_with_every_weight_gradient_on_split_rows(case, kw, gpu_device, monkeypatch):
    """Round 4: a training forward of the tile kernel that keeps M^(t) as SPLIT ROWS (`msplit`), the backward tile kernel writing gZ^(t) /
    gH0 / gZO as split rows, [V[src] || E] and [V || Mv] split by k_rows2sr, ALL products (and the bias gradients, as column-sum jobs) in
    one k_wgrad16r launch — against the same step on block operands (k_wsplit16 + k_wgrad16), which the executed-reference tests hold.
    Both are exact-split fp32-class products of the same operands: equal to rounding, masks included (the kept tensors are the same)."""
    from chemprop_amd import engine, synth
    from chemprop_amd.nn import BondMessagePassing

    monkeypatch.setenv("DMPNN_VALIDATE", "never")
    if "fullplan" in case:
        monkeypatch.setenv("DMPNN_TRAIN_PLAN", "full")
    if case.startswith("mixed"):
        bmg = _mixed_batch(40, "synth40", 21)
    else:
        bmg = synth.random_batch(int(case.split("-")[1]), "qm9", seed=12)
    bmg.to(gpu_device)
    torch.manual_seed(4)
    mp0 = BondMessagePassing(**kw)
    V_d = torch.randn(bmg.V.shape[0], kw["d_vd"], generator=torch.Generator().manual_seed(8)).to(gpu_device) if kw.get("d_vd") else None
    G = torch.randn(bmg.V.shape[0], mp0.output_dim, generator=torch.Generator().manual_seed(6)).to(gpu_device)
    if "masked" in case:
        G = G * 1e-6
        G[bmg.batch < len(bmg) // 2] = 0.0   # the first half of the molecules without gradient: all-zero gradient tiles (scale 1 by convention) beside 1e-6 ones
    res = {}
    for rows in ("1", "0"):
        monkeypatch.setenv("DMPNN_KEEP_ROWS", rows)
        mp = BondMessagePassing(**kw)
        mp.load_state_dict(mp0.state_dict())
        mp = mp.to(gpu_device).train()
        out = mp(bmg, V_d)
        st = out.grad_fn.st
        assert st.route == "mega16" and bool(st.args.msplit) == (rows == "1"), (rows, st.route)
        assert bool(st.plan.tiles_only) == ("fullplan" not in case and V_d is None)
        out.backward(G)
        res[rows] = (out.detach(), {k: p.grad.clone() for k, p in mp.named_parameters()})
    assert torch.equal(res["1"][0], res["0"][0])
    for k, v in res["0"][1].items():
        assert torch.isfinite(res["1"][1][k]).all(), k
        err = parity_err(res["1"][1][k].cpu().numpy(), v.cpu().numpy())
        assert err <= 5e-6, f"{k}: {err:.3e}"


def test_split_rows_are_kept_from_a_size_on(gpu_device):
    """The default rule (engine.KEEP_ROWS_MIN message rows; round 6: 4 096, was 32 768): 512 QM9-shaped molecules keep split rows, 64 the
    fp32 rows of the block path."""
    from chemprop_amd import engine, synth
    from chemprop_amd.nn import BondMessagePassing

    mp = BondMessagePassing().to(gpu_device).train()
    for n, want in ((64, False), (512, True)):
        bmg = synth.random_batch(n, "qm9", seed=3)
        bmg.to(gpu_device)
        out = mp(bmg)
        st = out.grad_fn.st
        assert st.route == "mega16" and bool(st.args.msplit) == want, (n, st.route)
        assert (int(bmg.E.shape[0]) * 2 >= engine.KEEP_ROWS_MIN) == want
        out.sum().backward()
        assert all(torch.isfinite(p.grad).all() for p in mp.parameters())
