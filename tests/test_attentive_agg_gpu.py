"""AttentiveAggregation's kernels (``dmpnn_molagg_attn_fwd`` / ``_bwd``, csrc/dmpnn_attn.hip) through the C ABI against the float64
restatement (``oracle.agg_torch.attentive`` + autograd), and the module on top of them.

Bars: ``attn_harness`` — per tensor ``max|got - ref64| / max|ref64| <= min(32 max(e32, 2**-23), cap)``, caps 1e-5 (out) / 2e-5
(gradients); ``|gb| <= 32 * 2**-23 * sum_v |dl_v|``.  One line per tensor is printed before it is judged.

The quad build and the single-float build hand a row to the lanes differently (lane l holds columns 4l .. 4l + 3 against l, l + 64,
...), so their wave reductions add in another order: they are NOT promised to be bit-identical; both are held to the bars.
"""
import numpy as np
import pytest
import torch

import attn_harness as ah
from conftest import TOL, parity_err

pytestmark = pytest.mark.gpu

_cache = {}


def _case(case):
    """Inputs and the float64 yardstick of a case, computed once and shared (never modified)."""
    if case.id not in _cache:
        inp = ah.build(case)
        _cache[case.id] = (inp, *ah.yardstick(inp))
    return _cache[case.id]


def bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("case", ah.agg_cases(), ids=lambda c: c.id)
def test_kernels_against_float64(case, gpu_device):
    inp, r64, e32 = _case(case)
    got = ah.run(inp, gpu_device, pad=case.pad, offset=case.offset)
    fails = ah.compare(case.id, got, r64, e32)
    assert got["padding_ok"], "columns beyond the width (or rows outside the views) were written"
    assert got["n_fwd"] == 1, f"the forward pass took {got['n_fwd']} launches"
    # molecules without atoms: exactly zero rows, and Z = 0 kept for them
    empty = [i for i, n in enumerate(case.sizes + (0,) * case.extra_mols) if n == 0]
    assert bool((got["out"][empty] == 0).all())
    # the kept s / Z are the softmax's terms
    al = got["s"][: inp["H"].shape[0]].double() / got["Z"][: case.n_mols].double()[inp["batch"]]
    seg = torch.zeros(case.n_mols, dtype=torch.float64).index_add(0, inp["batch"], al)
    assert bool(((seg - 1).abs()[[i for i in range(case.n_mols) if i not in empty]] <= 1e-5).all())
    assert not fails, fails


def test_vector_and_scalar_builds_on_the_same_inputs(gpu_device):
    """The same inputs aligned (16-byte quads) and at ``ld + 1`` (single floats): both within the bars.  The builds hand a row to the
    lanes differently, so the wave reductions add in another order: no promise of equal bits, and none is asserted."""
    for d in (44, 300, ah.NARROW_VEC + 4):
        case = ah.AggCase(f"vs-d{d}", ah.BASE_SIZES, d)
        inp, r64, e32 = _case(case)
        vec, sca = ah.run(inp, gpu_device), ah.run(inp, gpu_device, pad=1)
        fails = ah.compare(case.id + "-vec", vec, r64, e32) + ah.compare(case.id + "-scalar", sca, r64, e32)
        print(f"ATTNBAR {case.id} vec-vs-scalar max|d out| = {float((vec['out'] - sca['out']).abs().max()):.3e}")
        assert not fails, fails


def test_two_calls_give_the_same_bits_and_null_outputs_change_nothing(gpu_device):
    """1 025 molecules of 1 .. 3 atoms: gW spans every partial row (one more molecule than rows: one wave walks two)."""
    gen = torch.Generator().manual_seed(3)
    sizes = tuple(int(x) for x in torch.randint(1, 4, (ah.PARTIAL_ROWS + 1,), generator=gen))
    case = ah.AggCase("det-1025", sizes, 44)
    inp, r64, e32 = _case(case)
    a, b = ah.run(inp, gpu_device), ah.run(inp, gpu_device)
    fails = ah.compare(case.id, a, r64, e32)
    for k in ("out", "gH", "gW", "gb", "s", "Z"):
        assert torch.equal(bits(a[k]), bits(b[k])), k
    for want_gW, want_gb in ((False, True), (True, False), (False, False)):
        c = ah.run(inp, gpu_device, want_gW=want_gW, want_gb=want_gb)
        assert torch.equal(bits(c["out"]), bits(a["out"])) and torch.equal(bits(c["gH"]), bits(a["gH"]))
        assert torch.equal(bits(c["gW"]), bits(a["gW"])) if want_gW else bool(torch.isnan(c["gW"]).all())   # (not wanted: not written)
        assert torch.equal(bits(c["gb"]), bits(a["gb"])) if want_gb else bool(torch.isnan(c["gb"]).all())
    # inference: no keep buffers, the same aggregate
    f = ah.run(inp, gpu_device, keep=False, backward=False)
    assert torch.equal(bits(f["out"]), bits(a["out"])) and bool(torch.isnan(f["s"]).all()) and bool(torch.isnan(f["Z"]).all())
    # bounds == NULL: the table is built from the batch vector inside the call (one more launch), the same bits
    o = ah.run(inp, gpu_device, own_bounds=True)
    assert o["n_fwd"] == 2
    for k in ("out", "gH", "gW", "gb"):
        assert torch.equal(bits(o[k]), bits(a[k])), k
    assert not fails, fails


@pytest.mark.parametrize("bad", ["decreasing", "out-of-range"])
def test_invalid_batch_vector_poisons_every_output(bad, gpu_device):
    """Handled errors: the table's flag turns out, gH, gW and gb into NaN; nothing is read through the broken bounds."""
    inp = ah.build(ah.AggCase("bad", (2, 1, 3), 8))
    inp = dict(inp, batch=torch.tensor([0, 1, 0, 2, 2, 2]) if bad == "decreasing" else torch.tensor([0, 0, 1, 2, 2, 7]))
    got = ah.run(inp, gpu_device)
    for k in ("out", "gH", "gW", "gb"):
        assert bool(torch.isnan(got[k]).all()), k
    assert got["padding_ok"]


def test_no_atoms_or_no_molecules_zero_the_requested_gradients(gpu_device):
    import ctypes as C

    from chemprop_amd import _lib, engine

    lib = _lib.load()
    dev = gpu_device
    d = 8
    gW, gb = torch.full((d,), float("nan"), device=dev), torch.full((1,), float("nan"), device=dev)
    out = torch.full((3, d), float("nan"), device=dev)
    W, b = torch.randn(d, device=dev), torch.randn(1, device=dev)
    batch = torch.zeros(0, dtype=torch.int64, device=dev)
    table = ah.bounds_table(batch, 3)
    s, Z = torch.zeros(1, device=dev), torch.zeros(3, device=dev)
    gout = torch.randn(3, d, device=dev)
    a = _lib.MolAggAttnArgs()
    a.n_atoms, a.n_mols, a.d_h = 0, 3, d
    a.ldh = a.ldo = a.ldgo = a.ldgh = d
    a.bounds, a.W, a.b, a.out = table.data_ptr(), W.data_ptr(), b.data_ptr(), out.data_ptr()
    a.keep_s, a.keep_Z, a.gout, a.gW, a.gb = s.data_ptr(), Z.data_ptr(), gout.data_ptr(), gW.data_ptr(), gb.data_ptr()
    ws = torch.empty(int(lib.dmpnn_molagg_attn_ws_bytes(C.byref(a))), dtype=torch.uint8, device=dev)
    a.ws, a.ws_bytes = ws.data_ptr(), ws.numel()
    with engine._OnDevice(dev):
        _lib.check(lib.dmpnn_molagg_attn_fwd(C.byref(a), engine._stream_ptr(dev)), "fwd")
        _lib.check(lib.dmpnn_molagg_attn_bwd(C.byref(a), engine._stream_ptr(dev)), "bwd")
    torch.cuda.synchronize()
    assert bool((out == 0).all()) and bool((gW == 0).all()) and bool((gb == 0).all())


# ---- the module ---------------------------------------------------------------------------------------------------------------
def _golden_cases():
    import glob
    import os

    from conftest import GOLDEN_DIR

    return sorted(glob.glob(os.path.join(GOLDEN_DIR, "agg", "*.npz")))


def _module_run(z, dev):
    from chemprop_amd import agg

    d = z["H"].shape[1]
    mod = agg.AttentiveAggregation(output_size=d)
    mod.load_state_dict({"W.weight": torch.from_numpy(z["att_W"]), "W.bias": torch.from_numpy(z["att_b"])})
    mod = mod.to(dev)
    H = torch.from_numpy(z["H"]).to(dev).requires_grad_(True)
    b = torch.from_numpy(z["batch"]).to(dev)
    from chemprop_amd import _lib

    lib = _lib.load()
    n0 = int(lib.dmpnn_last_launch_count())
    out = mod(H, b)
    n_fwd = int(lib.dmpnn_last_launch_count()) - n0
    (out * torch.from_numpy(z["G"]).to(dev)).sum().backward()
    return dict(out=out.detach().cpu(), gH=H.grad.cpu(), gW=mod.W.weight.grad.cpu(), gb=mod.W.bias.grad.cpu(), n_fwd=n_fwd,
                node=type(out.grad_fn).__name__)


@pytest.mark.parametrize("path", _golden_cases(), ids=lambda p: p.rsplit("/", 1)[-1][:-4])
def test_module_against_the_goldens_and_the_chain(path, gpu_device, monkeypatch):
    """``AttentiveAggregation`` forward + backward on the new node against the executed reference's goldens at the bars of
    tests/test_agg.py, against the ``DMPNN_ATTN=chain`` run in the same process within those bars, and two launches forward: the
    bounds table and the attention (the library's own launch counter)."""
    z = dict(np.load(path))
    new = _module_run(z, gpu_device)
    monkeypatch.setenv("DMPNN_ATTN", "chain")
    old = _module_run(z, gpu_device)
    assert new["node"].startswith("_Attentive") and not old["node"].startswith("_Attentive")
    assert new["n_fwd"] == 2, new["n_fwd"]
    print(f"ATTNMOD launches forward: new {new['n_fwd']} chain {old['n_fwd']} (the chain's torch ops are not counted by the library)")
    for k, gk, bar in (("out", "out_att", TOL), ("gH", "gH_att", 2e-5), ("gW", "gW_att", 2e-5), ("gb", "gb_att", 2e-5)):
        e_gold, e_chain = parity_err(new[k].numpy(), z[gk]), parity_err(new[k].numpy(), old[k].numpy())
        print(f"ATTNMOD {k} vs golden {e_gold:.3e} vs chain {e_chain:.3e} bar {bar:.0e}")
        assert e_gold <= bar and e_chain <= bar, k
