"""SELU (``DMPNN_ACT_SELU``) through every row entry of ``include/dmpnn.h`` that takes an activation code — ``dmpnn_linear_fwd``,
``dmpnn_linear16_fwd``, ``dmpnn_linear16_dropout_fwd``, ``dmpnn_update_fwd``, and ``dmpnn_message_fwd`` / ``dmpnn_aggregate_fwd``, which
apply one on load — against ``F.selu`` in float64.  The runners are the harness's (``tests/rows_harness.py``: they look the code up in
``_lib.ACT``); its references call ``oracle.dmpnn_torch.activation_fn`` by module attribute, which this file extends with ``"selu"``
at run time (``monkeypatch``), the oracle itself untouched.

Shapes: the harness's smallest activation shape (M 17, N 7, K1 5, K2 3: the scalar epilogue of the fp32 kernel; the f16 pipe needs
even widths: K1 6, K2 2) and 130 x 66 x (56 + 14), which crosses a tile in each of M, N and K on both pipes.

Every case asserts on its float64 pre-activations, before anything runs on the device: at least a quarter negative, at least a quarter
positive, one below -5, one exactly 0 placed by hand (a zero operand row whose ``Cadd`` entry is minus the bias) — there the output must
be exactly 0.  The stock inputs do not reach -5; ``Cadd`` is scaled by 4, which does.

Judged by the suite's rule: ``err = max|got - ref| / max|ref|`` within ``min(rows_harness.MARGIN max(e32, 2**-23), cap)``, one ROWSBAR
line per tensor printed before judging.  Measured on the MI355X (24 comparisons): the worst ``err / max(e32, 2**-23)`` is 1.00
(``M_next`` of ``update_fwd`` at ``d_h`` 68 and the two ``message_fwd`` cases at ``h`` 64: the kernel's error IS the float32 restatement's), every
other tensor below 0.9; the bars are 1.9e-6 .. 2.3e-6."""
import math

import pytest
import torch
import torch.nn.functional as F

import rows_harness as rh
from chemprop_amd import _lib
from oracle import dmpnn_torch as ot

pytestmark = pytest.mark.gpu

LA = 1.0507009873554804934193349852946 * 1.6732632423543772848170429916717   # lambda alpha: tau'(0) from the left, -tau(-inf)


@pytest.fixture(autouse=True)
def _selu_in_the_oracle(monkeypatch):
    orig = ot.activation_fn
    monkeypatch.setattr(ot, "activation_fn", lambda name, w=None: F.selu if str(name).lower() == "selu" else orig(name, w))


def condition(z, zero_at=None):
    """The condition on a case's float64 pre-activations (checked on the CPU)."""
    z = z.double()
    n = z.numel()
    assert int((z < 0).sum()) * 4 >= n and int((z > 0).sum()) * 4 >= n, (int((z < 0).sum()), int((z > 0).sum()), n)
    assert bool((z < -5).any()), float(z.min())
    assert bool((z == 0).any())
    if zero_at is not None:
        assert float(z[zero_at]) == 0.0


SHAPES = {"f32": ((17, 7, 5, 3), (130, 66, 56, 14)), "f16": ((17, 7, 6, 2), (130, 66, 56, 14))}
R0, C0 = 3, 2   # where the exact zero is placed


def _linear_inputs(M, N, K1, K2):
    inp = rh.linear_inputs(M, N, K1, K2, seed=M + N)
    inp["Cadd"] = inp["Cadd"] * 4.0
    inp["A1"][R0] = 0.0
    inp["A2"][R0] = 0.0
    inp["Cadd"][R0, C0] = -inp["bias"][C0]
    return inp


def _linear_case(M, N, K1, K2):
    inp = _linear_inputs(M, N, K1, K2)
    r64, r32 = rh.linear_ref(inp, "selu"), rh.linear_ref(inp, "selu", torch.float32)
    condition(r64["Zpre"], (R0, C0))
    assert torch.equal(r64["C"], F.selu(r64["Zpre"])) and float(r64["C"][R0, C0]) == 0.0
    assert float(r64["C"].min()) < -0.99 * LA         # (the saturated branch is there)
    return inp, r64, r32


@pytest.mark.parametrize("pipe,shape", [(p, s) for p in ("f32", "f16") for s in SHAPES[p]], ids=lambda v: v if isinstance(v, str) else "x".join(map(str, v)))
def test_selu_linear_fwd(pipe, shape, gpu_device):
    inp, r64, r32 = _linear_case(*shape)
    res = rh.run_linear(gpu_device, inp, "selu", pipe)
    assert res["rc"] == 0, res["msg"]
    assert res["launches"] == (1 if pipe == "f32" else 2)
    got = {k: m.read(k) for k, m in res["outs"].items()}
    fails = rh.compare(f"selu-linear-{pipe}-{'x'.join(map(str, shape))}", got, r64, rh.yardstick(r64, r32), "fwd")
    assert not fails, "; ".join(fails)
    assert float(got["C"][R0, C0]) == 0.0 and float(got["Zpre"][R0, C0]) == 0.0
    assert bool((got["C"] >= -LA * (1 + 2.0 ** -22)).all())


@pytest.mark.parametrize("shape", SHAPES["f16"], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("p", [0.25])
def test_selu_linear16_dropout_fwd(shape, p, gpu_device):
    """The DROP builds of the row kernel: a kept entry is the unmasked SELU output times the float scale, a dropped one +0; against
    float64 given the hash mask."""
    from oracle import dropout_hash as dh
    from test_rows_dropout_gpu import _run16, _scale32

    seed, site = 0x5E1F_0123_4567, 2
    M, N = shape[0], shape[1]
    inp, r64, r32 = _linear_case(*shape)
    Cd, Zd = _run16(gpu_device, inp, "selu", (p, seed, site))
    Cp, Zp = _run16(gpu_device, inp, "selu")
    keep = torch.from_numpy(dh.keep_mask(seed, site, M, N, p))
    bits = lambda t: t.contiguous().view(torch.int32)
    assert bool((bits(Cd)[~keep] == 0).all()) and torch.equal(bits(Zd), bits(Zp))
    assert torch.equal(bits(Cd)[keep], bits(Cp * _scale32(p))[keep])
    s = _scale32(p)
    ref = dict(C=torch.where(keep, r64["C"] * s, torch.zeros((), dtype=torch.float64)), Zpre=r64["Zpre"])
    ref32 = dict(C=torch.where(keep, r32["C"] * s, torch.zeros(())), Zpre=r32["Zpre"])
    fails = rh.compare(f"selu-linear16-dropout-{'x'.join(map(str, shape))}", dict(C=Cd, Zpre=Zd), ref, rh.yardstick(ref, ref32), "fwd")
    assert not fails, "; ".join(fails)


# ---- dmpnn_update_fwd, dmpnn_message_fwd, dmpnn_aggregate_fwd: on a graph -------------------------------------------------------------
def _graph():
    return rh.degree_graph((0, 1, 2, 3, 4, 5, 6, 7, 12) * 2)   # 98 atoms, 160 directed edges: several row tiles


@pytest.mark.parametrize("d_h", [4, 68], ids=["h4", "h68-two-column-blocks"])   # (the entry takes multiples of 4)
def test_selu_update_fwd(d_h, gpu_device):
    bmg = _graph()
    plan, arr = rh.make_plan(bmg, gpu_device)
    nE = int(bmg.edge_index.shape[1])
    inp = rh.update_inputs(nE, d_h, True, seed=d_h)
    inp["H0"] = inp["H0"] * 4.0
    inp["M"][R0] = 0.0
    inp["H0"][R0, C0] = -inp["b_h"][C0]
    z = (inp["M"].double() @ inp["W_h"].double().t() + inp["b_h"].double() + inp["H0"].double())   # (CSR-row order, as the inputs are)
    condition(z, (R0, C0))
    r64, r32 = rh.update_ref(bmg, arr["perm"], inp, "selu"), rh.update_ref(bmg, arr["perm"], inp, "selu", torch.float32)
    assert torch.allclose(r64["H_out"], F.selu(z), rtol=0, atol=1e-12)   # (the oracle adds in another order)
    rc, msg, outs = rh.run_update(gpu_device, plan, inp, "selu")
    assert rc == 0, msg
    got = {k: m.read(k) for k, m in outs.items()}
    fails = rh.compare(f"selu-update_fwd-h{d_h}", got, r64, rh.yardstick(r64, r32), "fwd")
    assert not fails, "; ".join(fails)
    assert float(got["H_out"][R0, C0]) == 0.0


@pytest.mark.parametrize("h,undirected", [(3, False), (64, False), (64, True)], ids=["h3-scalar", "h64-vector", "h64-undirected"])
def test_selu_on_load_of_message_and_aggregate(h, undirected, gpu_device):
    bmg = _graph()
    plan, _ = rh.make_plan(bmg, gpu_device)
    nE = int(bmg.edge_index.shape[1])
    Hin = torch.randn(nE, h, generator=torch.Generator().manual_seed(h)) * 4.0
    Hin[R0, C0] = 0.0
    condition(Hin, (R0, C0))
    for which in ("message", "aggregate"):
        und = undirected and which == "message"
        r64 = rh.segment_fwd_ref(bmg, Hin, which, "selu", und)
        r32 = rh.segment_fwd_ref(bmg, Hin, which, "selu", und, torch.float32)
        rc, msg, out = rh.run_segment_fwd(gpu_device, plan, which, Hin, act="selu", undirected=und)
        assert rc == 0, msg
        fails = rh.compare(f"selu-{which}_fwd-h{h}{'-undirected' if und else ''}", dict(out=out.read(which)), dict(out=r64),
                           rh.yardstick(dict(out=r64), dict(out=r32)), "fwd")
        assert not fails, "; ".join(fails)


def test_the_references_are_selu_on_the_cpu_side():
    """(needs no device, but lives with the cases it guards) the patched oracle gives ``F.selu``; the unpatched names are untouched."""
    x = torch.linspace(-8, 3, 23, dtype=torch.float64)
    assert torch.equal(ot.activation_fn("selu")(x), F.selu(x)) and torch.equal(ot.activation_fn("elu")(x), F.elu(x))
    assert math.isclose(float(F.selu(torch.tensor(-50.0, dtype=torch.float64))), -LA, rel_tol=1e-15)
    assert _lib.ACT["selu"] == 6
