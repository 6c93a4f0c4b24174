"""Gradients with respect to the block's inputs ``V``, ``E`` and ``V_d`` on the MI355X, against float64 — at three levels: the
row kernel (``dmpnn_src_sum`` through ctypes and ``Mat``), the C entry (``dmpnn_backward_inputs`` behind a kept forward of the per-step
general route) and the modules (``BondMessagePassing`` / ``AtomMessagePassing`` with their inputs as leaves that require grad).

The rule is the suite's own (``rows_harness.compare``): float64 reference, yardstick ``e32`` = the same computation in plain fp32
torch, ``err = max|got - ref| / max|ref| <= min(MARGIN max(e32, 2**-23), CAP["grad"])`` — ``MARGIN = 16``, ``CAP["grad"] = 2e-5``.

``gV`` comes from ``k_input_grad_v`` (a workgroup per ``FUSED_TILE`` atoms, ``[GO || S]`` through LDS in chunks of ``FUSED_KCHUNK``
columns, f16 pipe with the exact operand split) where the dispatch rule takes the call (``d_v <= FUSED_MAX_DV``), else from the composed
form: ``k_src_sum``, then the row contraction kernels (``ROW_TILE`` rows a tile) — which also form ``gE`` and ``gV_d``, on the f16 pipe
where ``linear16_ok`` takes the call (even ``d_h``), else on the fp32 MFMA kernel.  The shapes below sit on both sides of those seams:
``FUSED_TILE`` / ``ROW_TILE`` - 1, exact, + 1 atoms; ``d_h`` below, at and beyond one K-chunk (whole and partial quads); even / odd
``d_h``; ``d_v`` and ``d_e`` around the 16-column MFMA tile; ``d_v`` at and one beyond ``FUSED_MAX_DV`` (the first the fused kernel
refuses: the composed form runs); ``n_edges == 0``."""
import ctypes as C

import pytest
import torch
from torch import nn

from chemprop_amd import _lib
from oracle import dmpnn_torch as ot
from input_grad_shapes import FUSED_KCHUNK, FUSED_MAX_DV, FUSED_TILE, ROW_TILE
from rows_harness import CAP, MARGIN, Mat, _call, chain_graph, compare, degree_graph, make_plan, yardstick

pytestmark = pytest.mark.gpu

assert MARGIN == 16.0 and CAP["grad"] == 2e-5


# ---- row level: dmpnn_src_sum ---------------------------------------------------------------------------------------------------------
def _src_sum_ref(bmg, G, dtype):
    """``S[v] = sum_{e: src(e) = v} G[e]`` in ``dtype`` on the CPU."""
    return torch.zeros(int(bmg.V.shape[0]), G.shape[1], dtype=dtype).index_add_(0, bmg.edge_index[0], G.to(dtype))


def _run_src_sum(dev, plan, G, ld_g=None, ld_s=None, off_g=0, off_s=0):
    lib = _lib.load()
    h = int(G.shape[1])
    mg = Mat(dev, int(G.shape[0]), h, ld_g, off_g, G)
    ms = Mat(dev, plan.n_atoms, h, ld_s, off_s)
    rc, msg, launches = _call(dev, lib.dmpnn_src_sum, plan.buf.data_ptr(), plan.n_atoms, plan.n_edges, h, mg.ptr, mg.ld, ms.ptr, ms.ld)
    return rc, msg, launches, ms


_GRAPHS = {
    "degrees": lambda: degree_graph([0, 1, 2, 4, 12, 0, 2], seed=3),     # in-degrees 0, 1, 2, 4, 12; two single-atom molecules
    "one atom": lambda: degree_graph([0], seed=1),
    "no edges": lambda: degree_graph([0, 0, 0], seed=2),
}


@pytest.mark.parametrize("d_h", (1, 3, 4, 30, 31, 300))
@pytest.mark.parametrize("layout", ("dense", "padded quads", "padded off 1", "padded off 2"))
def test_src_sum_against_float64(d_h, layout, gpu_device):
    """Every graph at this width and layout: the sums against float64, padding and guard words untouched, two calls bit-equal."""
    pad4 = (d_h + 3) // 4 * 4 + 4
    ld_g, ld_s, off_g, off_s = {"dense": (None, None, 0, 0), "padded quads": (pad4, pad4 + 4, 0, 0),
                                "padded off 1": (d_h + 3, d_h + 1, 1, 0), "padded off 2": (d_h + 2, d_h + 5, 2, 2)}[layout]
    fails = []
    for name, make in _GRAPHS.items():
        bmg = make()
        plan, _ = make_plan(bmg, gpu_device)
        nE = int(bmg.edge_index.shape[1])
        G = torch.randn(nE, d_h, generator=torch.Generator().manual_seed(17 + d_h)) * (1 + torch.arange(d_h).float() / d_h)
        rc, msg, launches, ms = _run_src_sum(gpu_device, plan, G, ld_g, ld_s, off_g, off_s)
        assert rc == 0 and launches == 1, (name, rc, msg, launches)
        got = ms.read(f"S ({name})")
        ref = dict(S=_src_sum_ref(bmg, G, torch.float64))
        e32 = yardstick(ref, dict(S=_src_sum_ref(bmg, G, torch.float32)))
        fails += [f"{name}: {f}" for f in compare(f"src_sum[{d_h},{layout},{name}]", dict(S=got), ref, e32, "grad")]
        if nE == 0:
            assert bool((got == 0).all())
        rc2, _, _, ms2 = _run_src_sum(gpu_device, plan, G, ld_g, ld_s, off_g, off_s)
        assert rc2 == 0 and torch.equal(ms2.read().view(torch.int32), got.view(torch.int32)), name
    assert not fails, fails


def test_src_sum_is_nan_on_an_asymmetric_plan(gpu_device):
    """A hand-built graph whose ``rev`` is not the reverse edge: the plan says so (header bit 0) and every row of ``S`` is NaN."""
    from chemprop_amd import engine

    bmg = chain_graph(2, 4, seed=5)
    rev = torch.roll(bmg.rev_edge_index, 1)     # still a permutation of the edges, no longer src(rev e) == dst(e)
    plan = engine.GraphPlan(bmg.edge_index.to(gpu_device), rev.to(gpu_device), int(bmg.V.shape[0]))
    assert plan.flags() & 1
    for d_h in (4, 7):
        G = torch.randn(plan.n_edges, d_h, generator=torch.Generator().manual_seed(d_h))
        rc, msg, _, ms = _run_src_sum(gpu_device, plan, G, None, d_h + 2, 0, 0)
        assert rc == 0, msg
        assert bool(torch.isnan(ms.read()).all())


# ---- ABI level: dmpnn_backward_inputs behind engine.forward(route="general", keep=True) ---------------------------------------------------
_PARAMS = ("W_i", "b_i", "W_h", "b_h", "W_o", "b_o", "W_d", "b_d")


def _case_tensors(bmg, d_v, d_e, d_h, d_vd, bias, seed):
    gen = torch.Generator().manual_seed(100 + seed)
    nV, nE = int(bmg.V.shape[0]), int(bmg.edge_index.shape[1])
    u = lambda *shape, fan: (2 * torch.rand(*shape, generator=gen) - 1) / fan ** 0.5
    t = dict(V=torch.randn(nV, d_v, generator=gen), E=torch.randn(nE, d_e, generator=gen),
             W_i=u(d_h, d_v + d_e, fan=d_v + d_e), W_h=u(d_h, d_h, fan=d_h), W_o=u(d_h, d_v + d_h, fan=d_v + d_h), b_o=u(d_h, fan=d_v + d_h),
             b_i=u(d_h, fan=d_v + d_e) if bias else None, b_h=u(d_h, fan=d_h) if bias else None)
    if d_vd:
        t.update(V_d=torch.randn(nV, d_vd, generator=gen), W_d=u(d_h + d_vd, d_h + d_vd, fan=d_h + d_vd), b_d=u(d_h + d_vd, fan=d_h + d_vd))
    else:
        t.update(V_d=None, W_d=None, b_d=None)
    t["G"] = torch.randn(nV, d_h + d_vd, generator=gen)
    return t


def _oracle_grads(bmg, t, depth, act, undirected, dtype, atom=False):
    """Autograd through ``oracle.dmpnn_torch.forward`` in ``dtype``: the gradients of ``<out, G>`` w.r.t. the inputs and parameters."""
    leaves = {k: v.to(dtype).requires_grad_() for k, v in t.items() if v is not None and k != "G"}
    w = ot.MPWeights(leaves["W_i"], leaves["W_h"], leaves["W_o"], leaves["b_o"], leaves.get("b_i"), leaves.get("b_h"), leaves.get("W_d"), leaves.get("b_d"))
    fwd = ot.atom_forward if atom else ot.forward
    out = fwd(leaves["V"], leaves["E"], bmg.edge_index, bmg.rev_edge_index, w, depth=depth, activation=act, undirected=undirected, V_d=leaves.get("V_d"))
    (out * t["G"].to(dtype)).sum().backward()
    g = {k: (v.grad if v.grad is not None else torch.zeros_like(v)).detach() for k, v in leaves.items()}
    g["out"] = out.detach()
    return g


def _kept_forward(dev, bmg, t, depth, act, undirected, mfma):
    from chemprop_amd import engine

    plan, _ = make_plan(bmg, dev)
    d = {k: (v.to(dev) if v is not None else None) for k, v in t.items()}
    out, st = engine.forward(plan, d["V"], d["E"], d["W_i"], d["W_h"], d["W_o"], d["b_o"], d["b_i"], d["b_h"], d["W_d"], d["b_d"], d["V_d"],
                             depth=depth, act=act, slope=0.1 if act == "leakyrelu" else 0.0, undirected=undirected, keep=True, route="general", mfma=mfma)
    assert st.route == ("general16" if mfma == "split16" else "general"), st.route
    return plan, d, out, st


def _run_inputs(dev, st, gout, need, want, pad=True):
    """One ``dmpnn_backward_inputs`` call over the block ``engine.backward`` builds: the outputs ``want`` in ``Mat`` buffers (padded
    rows, 4-byte aligned pointers: padding and guards are checked on read) -> (rc, msg, parameter gradients, {name: Mat})."""
    from chemprop_amd import engine

    lib = _lib.load()
    grads, b, refs = engine.backward(st, gout, need, launch=False)
    a = _lib.BwdInputsArgs()
    a.b = b
    nb = int(lib.dmpnn_backward_inputs_ws_bytes(C.byref(st.args)))
    ws = torch.empty(nb // 4 + 1, dtype=torch.float32, device=dev)
    a.b.ws, a.b.ws_bytes = ws.data_ptr(), nb
    nV, nE, dims = int(st.args.n_atoms), int(st.args.n_edges), st.dims
    outs = {}
    for name, rows, width, field in (("V", nV, dims["d_v"], "ldgv"), ("E", nE, dims["d_e"], "ldge"), ("V_d", nV, dims["d_vd"], "ldgvd")):
        if name in want:
            m = outs[name] = Mat(dev, rows, width, width + 3 if pad else None, 1 if pad else 0)
            setattr(a, "g" + name, m.ptr)
            setattr(a, field, m.ld)
    rc, msg, _ = _call(dev, lib.dmpnn_backward_inputs, C.byref(a))
    return rc, msg, grads, outs


# (graph, d_v, d_e, d_h, d_vd, depth, act, undirected, bias, mfma)
_ABI_CASES = {
    "tile exact, d_v 16": (lambda: chain_graph(6, 8, seed=1), 16, 14, 16, 0, 3, "relu", False, False, "split16"),
    "tile - 1, d_v 15, W_d": (lambda: chain_graph(1, ROW_TILE - 1, seed=2), 15, 15, 30, 5, 2, "leakyrelu", True, True, "split16"),
    "tile + 1, d_v 17, d_h 4": (lambda: chain_graph(7, 7, seed=3), 17, 1, 4, 0, 4, "tanh", False, True, "f32"),
    "depth 1, d_v 72, W_d": (lambda: degree_graph([0, 1, 2, 4, 12, 3], seed=4), 72, 14, 30, 5, 1, "elu", False, False, "f32"),
    "d_v 133, d_h 300, W_d": (lambda: degree_graph([0, 1, 2, 4, 12, 5, 6], seed=5), 133, 14, 300, 5, 3, "relu", False, True, "split16"),
    "odd d_h 31 (fp32 contraction)": (lambda: chain_graph(5, 10, seed=6), 16, 15, 31, 0, 2, "relu", True, False, "f32"),
    "odd d_h 31, W_d": (lambda: degree_graph([2, 4, 1, 0, 7], seed=7), 15, 14, 31, 5, 3, "tanh", False, True, "f32"),
    "d_h 300, d_e 1": (lambda: chain_graph(4, 13, seed=8), 72, 1, 300, 0, 2, "elu", False, False, "split16"),
    "d_h 300 on the fp32 forward": (lambda: chain_graph(3, 17, seed=9), 16, 14, 300, 5, 2, "leakyrelu", False, True, "f32"),
    "undirected, depth 4": (lambda: degree_graph([3, 3, 2, 1], seed=10), 17, 15, 16, 0, 4, "elu", True, True, "split16"),
    "no edges": (lambda: degree_graph([0, 0, 0, 0], seed=11), 16, 14, 16, 5, 3, "relu", False, True, "f32"),
    # k_input_grad_v's own seams: atoms per tile, the K-chunk, the widest d_v it takes and the first it refuses
    "fused tile - 1": (lambda: chain_graph(1, FUSED_TILE - 1, seed=12), 16, 14, 16, 0, 2, "relu", False, False, "split16"),
    "fused tile exact": (lambda: chain_graph(2, FUSED_TILE // 2, seed=13), 17, 15, 30, 0, 2, "tanh", False, True, "split16"),
    "fused tile + 1": (lambda: chain_graph(1, FUSED_TILE + 1, seed=14), 15, 1, 4, 5, 3, "elu", True, False, "f32"),
    "one K-chunk exactly": (lambda: degree_graph([0, 1, 2, 4, 12, 3], seed=15), 72, 14, FUSED_KCHUNK, 0, 2, "relu", False, True, "split16"),
    "K-chunk + half a quad": (lambda: degree_graph([2, 4, 1, 0, 7], seed=16), 16, 14, FUSED_KCHUNK + 2, 0, 2, "leakyrelu", False, False, "split16"),
    "K-chunk + one quad": (lambda: chain_graph(3, 7, seed=17), 133, 15, FUSED_KCHUNK + 4, 5, 2, "relu", False, True, "f32"),
    "widest fused d_v": (lambda: chain_graph(3, 6, seed=18), FUSED_MAX_DV, 14, 30, 0, 2, "relu", False, True, "split16"),
    "first d_v the fused kernel refuses": (lambda: chain_graph(3, 6, seed=19), FUSED_MAX_DV + 1, 14, 30, 0, 2, "relu", False, True, "split16"),
}


@pytest.mark.parametrize("name", list(_ABI_CASES))
def test_backward_inputs_against_float64(name, gpu_device):
    """``gV``, ``gE``, ``gV_d`` and every parameter gradient against float64 autograd through the oracle."""
    make, d_v, d_e, d_h, d_vd, depth, act, undirected, bias, mfma = _ABI_CASES[name]
    bmg = make()
    t = _case_tensors(bmg, d_v, d_e, d_h, d_vd, bias, seed=len(name))
    ref = _oracle_grads(bmg, t, depth, act, undirected, torch.float64)
    e32 = yardstick(ref, _oracle_grads(bmg, t, depth, act, undirected, torch.float32))
    plan, d, out, st = _kept_forward(gpu_device, bmg, t, depth, act, undirected, mfma)
    present = [k for k in _PARAMS if t[k] is not None]
    want = ["V", "E"] + (["V_d"] if d_vd else [])
    rc, msg, grads, outs = _run_inputs(gpu_device, st, d["G"], {k: True for k in present}, want)
    assert rc == 0, msg
    got = {k: outs[k].read("g" + k) for k in want}
    got.update({k: grads[k].cpu() for k in present})
    got["out"] = out.cpu()
    kinds = {k: "grad" for k in got}
    kinds["out"] = "fwd"
    fails = compare(f"backward_inputs[{name}]", got, ref, e32, kinds)
    assert not fails, fails
    if int(bmg.edge_index.shape[1]) == 0:
        assert got["E"].numel() == 0


@pytest.mark.parametrize("name", ("tile exact, d_v 16", "d_v 133, d_h 300, W_d", "odd d_h 31, W_d"))
def test_parameter_gradients_are_bitwise_those_of_dmpnn_backward(name, gpu_device):
    """``gV == gE == gV_d == NULL``: the parameter gradients of the same kept state, bit for bit those of ``dmpnn_backward``."""
    from chemprop_amd import engine

    make, d_v, d_e, d_h, d_vd, depth, act, undirected, bias, mfma = _ABI_CASES[name]
    bmg = make()
    t = _case_tensors(bmg, d_v, d_e, d_h, d_vd, bias, seed=3)
    plan, d, out, st = _kept_forward(gpu_device, bmg, t, depth, act, undirected, mfma)
    need = {k: True for k in _PARAMS if t[k] is not None}
    base = engine.backward(st, d["G"], need)
    rc, msg, grads, _ = _run_inputs(gpu_device, st, d["G"], need, ())
    assert rc == 0, msg
    for k in need:
        assert torch.equal(grads[k].view(torch.int32), base[k].view(torch.int32)), k
    # ... and beside the input gradients as well
    rc, msg, grads2, _ = _run_inputs(gpu_device, st, d["G"], need, ("V", "E"))
    assert rc == 0, msg
    for k in need:
        assert torch.equal(grads2[k].view(torch.int32), base[k].view(torch.int32)), k


@pytest.mark.parametrize("name", ("tile + 1, d_v 17, d_h 4", "d_h 300, d_e 1", "tile - 1, d_v 15, W_d"))
def test_input_gradients_alone(name, gpu_device):
    """Every parameter-gradient pointer NULL (a frozen block): the data-gradient chain still runs and ``gV`` / ``gE`` come back right."""
    make, d_v, d_e, d_h, d_vd, depth, act, undirected, bias, mfma = _ABI_CASES[name]
    bmg = make()
    t = _case_tensors(bmg, d_v, d_e, d_h, d_vd, bias, seed=5)
    ref = _oracle_grads(bmg, t, depth, act, undirected, torch.float64)
    e32 = yardstick(ref, _oracle_grads(bmg, t, depth, act, undirected, torch.float32))
    plan, d, out, st = _kept_forward(gpu_device, bmg, t, depth, act, undirected, mfma)
    rc, msg, grads, outs = _run_inputs(gpu_device, st, d["G"], {}, ("V", "E"), pad=False)
    assert rc == 0, msg
    assert all(g is None for g in grads.values())
    fails = compare(f"inputs_alone[{name}]", {k: outs[k].read("g" + k) for k in ("V", "E")}, ref, e32, "grad")
    assert not fails, fails


@pytest.mark.parametrize("d_v", (16, FUSED_MAX_DV + 1), ids=("fused", "composed"))
def test_gv_is_nan_on_an_asymmetric_plan(d_v, gpu_device):
    """The backward pass of a kept forward handed a plan of the same sizes whose ``rev`` is not the reverse edge (header bit 0):
    every element of ``gV`` is NaN, from ``k_input_grad_v`` and from the composed form alike — never a wrong number."""
    from chemprop_amd import engine

    bmg = chain_graph(2, 4, seed=5)
    t = _case_tensors(bmg, d_v, 14, 16, 0, False, seed=2)
    plan, d, out, st = _kept_forward(gpu_device, bmg, t, 2, "relu", False, "split16")
    bad = engine.GraphPlan(bmg.edge_index.to(gpu_device), torch.roll(bmg.rev_edge_index, 1).to(gpu_device), int(bmg.V.shape[0]))
    assert bad.flags() & 1 and (bad.n_atoms, bad.n_edges) == (plan.n_atoms, plan.n_edges)
    st.args.plan = bad.buf.data_ptr()
    rc, msg, _, outs = _run_inputs(gpu_device, st, d["G"], {}, ("V",))
    assert rc == 0, msg
    assert bool(torch.isnan(outs["V"].read("gV")).all())


def test_engine_backward_returns_the_input_gradients(gpu_device):
    """``engine.backward(..., inputs={"V", "E", "V_d"})`` and ``engine.src_sum``: the Python wrappers of the two entries."""
    from chemprop_amd import engine

    make, d_v, d_e, d_h, d_vd, depth, act, undirected, bias, mfma = _ABI_CASES["tile - 1, d_v 15, W_d"]
    bmg = make()
    t = _case_tensors(bmg, d_v, d_e, d_h, d_vd, bias, seed=9)
    ref = _oracle_grads(bmg, t, depth, act, undirected, torch.float64)
    e32 = yardstick(ref, _oracle_grads(bmg, t, depth, act, undirected, torch.float32))
    plan, d, out, st = _kept_forward(gpu_device, bmg, t, depth, act, undirected, mfma)
    grads = engine.backward(st, d["G"], {"W_o": True}, inputs={"V", "E", "V_d"})
    got = {k: grads[k].cpu() for k in ("V", "E", "V_d", "W_o")}
    assert not (fails := compare("engine.backward(inputs)", got, ref, e32, "grad")), fails
    G = torch.randn(plan.n_edges, 6, generator=torch.Generator().manual_seed(1))
    S = engine.src_sum(plan, G.to(gpu_device)).cpu()
    r = dict(S=_src_sum_ref(bmg, G, torch.float64))
    assert not (fails := compare("engine.src_sum", dict(S=S), r, yardstick(r, dict(S=_src_sum_ref(bmg, G, torch.float32))), "grad")), fails


# ---- module level -----------------------------------------------------------------------------------------------------------------------
def _bmg_with_features(index_bmg, V, E, dev):
    from chemprop_amd.data import BatchMolGraph

    n_mols = int(index_bmg.batch.max()) + 1
    b = BatchMolGraph.from_tensors(V.clone(), E.clone(), index_bmg.edge_index.clone(), index_bmg.rev_edge_index.clone(), index_bmg.batch.clone(), n_mols)
    b.to(dev)
    return b


def _block_classes():
    from chemprop_amd.nn import BondMessagePassing

    classes = [("BondMessagePassing", BondMessagePassing)]
    try:
        from chemprop_amd.integration import hip_bond_message_passing_class

        classes.append(("HipBondMessagePassing", hip_bond_message_passing_class()))
    except ImportError:
        pass   # (the subclass of the reference's class exists only where the reference is importable)
    return classes


class _RecordingDropout(nn.Dropout):
    """``nn.Dropout`` that keeps the masks it emitted (drawn from the device generator: ``torch.manual_seed`` fixes them)."""

    def __init__(self, p):
        super().__init__(p)
        self.masks = []

    def forward(self, x):
        if not self.training or self.p == 0:
            return x
        m = (torch.rand_like(x) >= self.p).to(x.dtype) / (1.0 - self.p)
        self.masks.append(m.detach())
        return x * m


def _module_reference(bmg, mp, t, masks, dtype, atom=False):
    """base.py:196-212 in ``dtype`` on the CPU with the block's own ``tau`` (a copy in ``dtype``) and the recorded dropout masks
    replayed in call order (none recorded: dropout inactive) — the oracle's pieces; gradients of ``<out, G>``."""
    import copy

    tau = copy.deepcopy(mp.tau).cpu().to(dtype)
    state = {k: v.detach().cpu().to(dtype).requires_grad_() for k, v in mp.state_dict().items() if not k.startswith("tau.")}
    leaves = {k: t[k].to(dtype).requires_grad_() for k in ("V", "E", "V_d") if t.get(k) is not None}
    w = ot.MPWeights(state["W_i.weight"], state["W_h.weight"], state["W_o.weight"], state["W_o.bias"], state.get("W_i.bias"), state.get("W_h.bias"),
                     state.get("W_d.weight"), state.get("W_d.bias"))
    it = iter(masks)
    drop = (lambda x: x * next(it).cpu().to(dtype)) if masks else (lambda x: x)
    src, dst, rev = bmg.edge_index[0], bmg.edge_index[1], bmg.rev_edge_index
    nV = int(leaves["V"].shape[0])
    H0 = ot.atom_initialize(leaves["V"], src, w) if atom else ot.initialize(leaves["V"], leaves["E"], src, w)
    H = tau(H0)
    for _ in range(1, mp.depth):
        if mp.undirected:
            H = (H + H[rev]) / 2
        M = ot.atom_message(H, leaves["E"], src, dst, nV) if atom else ot.message(H, src, dst, rev, nV)
        H = drop(tau(H0 + torch.nn.functional.linear(M, w.W_h, w.b_h)))
    Mv = ot.segment_sum_dst(H, dst, nV)
    Hv = drop(tau(torch.nn.functional.linear(torch.cat((leaves["V"], Mv), 1), w.W_o, w.b_o)))
    if "V_d" in leaves:
        Hv = drop(torch.nn.functional.linear(torch.cat((Hv, leaves["V_d"]), 1), w.W_d, w.b_d))
    (Hv * t["G"].to(dtype)).sum().backward()
    g = {k: (v.grad if v.grad is not None else torch.zeros_like(v)).detach() for k, v in leaves.items()}
    g.update({k: (v.grad if v.grad is not None else torch.zeros_like(v)).detach() for k, v in state.items()})
    for k, v in tau.named_parameters():
        g["tau." + k] = v.grad.detach()
    g["out"] = Hv.detach()
    return g


def _run_module(dev, mp, index_bmg, t, frozen=False, record=False):
    """One forward + ``autograd.grad`` of ``<out, G>`` w.r.t. the input leaves (and the parameters unless ``frozen``)."""
    mp = mp.to(dev)
    if frozen:
        mp.eval()
        for p in mp.parameters():
            p.requires_grad_(False)
    else:
        mp.train()
    if record:
        mp.dropout = _RecordingDropout(mp.dropout.p).train()
    bmg = _bmg_with_features(index_bmg, t["V"], t["E"], dev)
    bmg.V.requires_grad_()
    bmg.E.requires_grad_()
    V_d = t["V_d"].to(dev).requires_grad_() if t.get("V_d") is not None else None
    out = mp(bmg, V_d)
    loss = (out * t["G"].to(dev)).sum()
    leaves = dict(V=bmg.V, E=bmg.E)
    if V_d is not None:
        leaves["V_d"] = V_d
    leaves.update({k: p for k, p in mp.named_parameters() if p.requires_grad})
    grads = torch.autograd.grad(loss, list(leaves.values()), allow_unused=True, retain_graph=True)
    got = {k: (g if g is not None else torch.zeros_like(v)).detach().cpu() for (k, v), g in zip(leaves.items(), grads)}
    got["out"] = out.detach().cpu()
    return got, loss, leaves, (mp.dropout.masks if record else [])


def _check_module(case, got, index_bmg, mp, t, masks, atom=False):
    ref = _module_reference(index_bmg, mp, t, masks, torch.float64, atom)
    e32 = yardstick(ref, _module_reference(index_bmg, mp, t, masks, torch.float32, atom))
    kinds = {k: "grad" for k in got}
    kinds["out"] = "fwd"
    fails = compare(case, got, ref, e32, kinds)
    assert not fails, fails


def _module_tensors(index_bmg, d_v, d_e, d_out, d_vd, seed):
    gen = torch.Generator().manual_seed(300 + seed)
    nV, nE = int(index_bmg.V.shape[0]), int(index_bmg.edge_index.shape[1])
    return dict(V=torch.randn(nV, d_v, generator=gen), E=torch.randn(nE, d_e, generator=gen),
                V_d=torch.randn(nV, d_vd, generator=gen) if d_vd else None, G=torch.randn(nV, d_out, generator=gen))


@pytest.mark.parametrize("cls_name", [n for n, _ in _block_classes()])
@pytest.mark.parametrize("mode", ("train", "eval frozen"))
@pytest.mark.parametrize("kw", [dict(d_v=16, d_e=14, d_h=32, depth=3), dict(d_v=17, d_e=15, d_h=30, depth=2, d_vd=5, bias=True, activation="tanh"),
                                dict(d_v=16, d_e=14, d_h=31, depth=3, undirected=True, activation="elu")],
                         ids=("relu", "tanh W_d", "elu undirected odd"))
def test_block_input_gradients_on_the_general_route(cls_name, mode, kw, gpu_device):
    """``V``, ``E`` (and ``V_d``) as leaves that require grad — the case the block refused: ``train()`` with trainable weights, and
    ``eval()`` with the block frozen (attributions), where the module must still take the general route."""
    cls = dict(_block_classes())[cls_name]
    torch.manual_seed(11)
    mp = cls(**kw)
    index_bmg = degree_graph([0, 1, 2, 4, 12, 3, 3], seed=21)
    t = _module_tensors(index_bmg, kw["d_v"], kw["d_e"], mp.output_dim, kw.get("d_vd"), seed=kw["d_h"])
    got, loss, leaves, _ = _run_module(gpu_device, mp, index_bmg, t, frozen=(mode == "eval frozen"))
    assert mp.__dict__.get("_dmpnn_route") in ("general", "general16"), mp.__dict__.get("_dmpnn_route")
    _check_module(f"block[{cls_name},{mode}]", got, index_bmg, mp, t, [])
    # the kept workspace went with the first backward
    with pytest.raises(RuntimeError, match="second time"):
        torch.autograd.grad(loss, [leaves["V"]])


@pytest.mark.parametrize("case", ("prelu", "softplus", "dropout", "dropout frozen"))
def test_block_input_gradients_on_the_rows_route(case, gpu_device):
    """What the fused backward does not carry — PReLU, a custom activation module, active dropout (the masks recorded on the device
    under ``torch.manual_seed`` and replayed in the reference) — takes the row kernels, whose gathered ``W_i`` product now has a
    data gradient (``engine.src_sum``)."""
    from chemprop_amd.nn import BondMessagePassing

    kw = dict(d_v=16, d_e=14, d_h=32, depth=3, bias=True)
    if case == "prelu":
        kw["activation"] = "prelu"
    elif case == "softplus":
        kw["activation"] = nn.Softplus()
    else:
        kw.update(dropout=0.25, d_vd=5, activation="tanh")
    torch.manual_seed(13)
    mp = BondMessagePassing(**kw)
    index_bmg = degree_graph([0, 1, 2, 4, 12, 3], seed=22)
    t = _module_tensors(index_bmg, kw["d_v"], kw["d_e"], mp.output_dim, kw.get("d_vd"), seed=7)
    record = case.startswith("dropout")
    frozen = case == "dropout frozen"
    torch.manual_seed(1234)
    if frozen:   # parameters frozen, dropout still active: train() mode with requires_grad off
        for p in mp.parameters():
            p.requires_grad_(False)
    got, _, _, masks = _run_module(gpu_device, mp, index_bmg, t, frozen=False, record=record)
    if record:
        assert len(masks) == (mp.depth - 1) + 2
    if frozen:
        got = {k: v for k, v in got.items() if k in ("V", "E", "V_d", "out")}
    _check_module(f"rows[{case}]", got, index_bmg, mp, t, masks)


def test_atom_block_input_gradients(gpu_device):
    """``AtomMessagePassing`` with ``V`` and ``E`` requiring grad on the rows route: ``E.grad`` is there (the bond-feature half of the
    message was formed under ``no_grad``) and right, against ``oracle.dmpnn_torch.atom_forward``'s pieces."""
    from chemprop_amd.nn import AtomMessagePassing

    for frozen in (False, True):
        kw = dict(d_v=16, d_e=14, d_h=32, depth=3, bias=True)
        torch.manual_seed(17)
        mp = AtomMessagePassing(**kw)
        index_bmg = degree_graph([0, 1, 2, 4, 12, 3], seed=23)
        t = _module_tensors(index_bmg, kw["d_v"], kw["d_e"], mp.output_dim, None, seed=9)
        got, _, leaves, _ = _run_module(gpu_device, mp, index_bmg, t, frozen=frozen)
        assert mp.__dict__.get("_dmpnn_route") == "rows/atom"
        assert float(got["E"].abs().max()) > 0
        _check_module(f"atom[frozen={frozen}]", got, index_bmg, mp, t, [], atom=True)
        # the oracle's own forward agrees with the restated pieces the reference above is made of
        w = ot.MPWeights(*(mp.state_dict()[k].cpu().double() for k in ("W_i.weight", "W_h.weight", "W_o.weight", "W_o.bias", "W_i.bias", "W_h.bias")))
        o = ot.atom_forward(t["V"].double(), t["E"].double(), index_bmg.edge_index, index_bmg.rev_edge_index, w, depth=3, activation="relu")
        o = o.detach()
        assert float((o - got["out"].double()).abs().max()) <= 1e-5 * float(o.abs().max())
