"""SELU as a built-in activation (``DMPNN_ACT_SELU = 6``), the host side that needs no GPU: the code and its name, the classification
of ``nn.SELU``, what the one-call step / the head / the inference head accept, the refusal texts, the route rules (``selu`` answers as
``elu`` does on the shape grid of ``tests/test_host.py``), and the argument checks of every entry that takes a block or predictor
activation — code 6 passes them, code 7 is still ``DMPNN_EINVAL``, PReLU is still refused where it was."""
import ctypes as C
import os
import re

import pytest
from torch import nn

from chemprop_amd import _lib, engine
from chemprop_amd import agg as cagg
from chemprop_amd.model import MPNN, HeadSpec, RegressionFFN, fused_block
from chemprop_amd.nn import AtomMessagePassing, BondMessagePassing, classify_activation, get_activation_function
from chemprop_amd.predict import PredictSpec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, ENOSPC = -1, -3
PTR = 4096


# ---- the code ----------------------------------------------------------------------------------------------------------------------
def test_the_code_is_6_and_the_header_says_so():
    assert _lib.ACT["selu"] == 6
    src = open(os.path.join(ROOT, "include", "dmpnn.h")).read()
    m = re.search(r"DMPNN_ACT_SELU\s*=\s*(\d+)", src)
    assert m and int(m.group(1)) == _lib.ACT["selu"]
    for name, code in _lib.ACT.items():   # (every other code as the header has it: nothing moved)
        m = re.search(r"DMPNN_ACT_%s\s*=\s*(\d+)" % name.upper(), src)
        assert m and int(m.group(1)) == code, name
    assert "1.6732632423543772848170429916717" in src and "1.0507009873554804934193349852946" in src
    assert _lib.ABI_VERSION == 15 and int(_lib.load().dmpnn_version()) == 15
    assert engine.act_code("selu") == engine.act_code("SELU") == 6


def test_classify_activation():
    assert classify_activation(nn.SELU()) == ("selu", 0.0, None)
    assert classify_activation(get_activation_function("selu")) == ("selu", 0.0, None)

    class MySELU(nn.SELU):
        pass

    assert classify_activation(MySELU())[0] == "custom"
    assert classify_activation(nn.ELU())[0] == "elu" and classify_activation(nn.ELU(alpha=1.6732632423543772))[0] == "custom"
    assert classify_activation(nn.CELU())[0] == "custom" and classify_activation(nn.AlphaDropout())[0] == "custom"


# ---- what takes a SELU model -------------------------------------------------------------------------------------------------------
def _model(activation="selu", p=0.0, ffn_p=0.0, d_h=64):
    return MPNN(BondMessagePassing(d_h=d_h, activation=activation, dropout=p), cagg.MeanAggregation(),
                RegressionFFN(input_dim=d_h, hidden_dim=32, activation=activation, dropout=ffn_p))


def test_fused_block_takes_selu_as_it_takes_elu():
    assert fused_block(BondMessagePassing(d_h=64, activation="selu")) == ("selu", 0.0)
    assert fused_block(BondMessagePassing(d_h=64, activation="selu", undirected=True), undirected=True)[0] == "selu"
    assert fused_block(AtomMessagePassing(d_h=64, activation="selu"), atom_messages=True)[0] == "selu"
    assert fused_block(BondMessagePassing(d_h=64, d_vd=5, activation="selu"))[0] == "selu"
    drop = BondMessagePassing(d_h=64, activation="selu", dropout=0.2)
    with pytest.raises(NotImplementedError, match="selu"):       # (the text tells the caller what would take it)
        fused_block(drop)
    assert fused_block(drop, rows_dropout=True) == ("selu", 0.0)
    for act in ("tanh", "elu"):                                   # (SELU's twins: the same answers)
        with pytest.raises(NotImplementedError):
            fused_block(BondMessagePassing(d_h=64, activation=act, dropout=0.2))
    alpha = BondMessagePassing(d_h=64, activation="selu", dropout=0.2)
    alpha.dropout = nn.AlphaDropout(0.2)                          # (not nn.Dropout: its own semantics, the module path)
    with pytest.raises(NotImplementedError):
        fused_block(alpha, rows_dropout=True)


def test_head_spec_and_predict_spec_take_a_selu_predictor():
    spec = HeadSpec(_model())
    assert spec.f_act == "selu" and spec.f_slope == 0.0
    assert _lib.ACT[spec.f_act] == 6
    with pytest.raises(NotImplementedError):
        HeadSpec(_model(ffn_p=0.2))
    assert HeadSpec(_model(ffn_p=0.2), ffn_dropout=True).f_act == "selu"
    assert PredictSpec(_model()).f_act == "selu" and PredictSpec(_model(ffn_p=0.2)).f_act == "selu"
    with pytest.raises(NotImplementedError):
        HeadSpec(_model(activation="prelu"))


def test_refusal_texts():
    assert engine.rows_dropout_refusal(72, 14, 400, 3, "selu") is None
    assert engine.rows_dropout_refusal(72, 14, 302, 1, "selu", undirected=True, undirected_dropout=True) is None
    assert engine.rows_dropout_refusal(72, 14, 64, 3, "selu", atom=True) is None
    assert "selu" in engine.rows_dropout_refusal(72, 14, 400, 3, "prelu")          # (the list of what it takes names it)
    why = engine.lean_dropout_refusal(72, 14, 300, 3, "selu")
    assert why is not None and "selu" in why and "sign bit" in why


# ---- the route rules: selu answers as elu does ---------------------------------------------------------------------------------------
def test_train_route_answers_for_selu_as_for_elu(monkeypatch):
    for k in ("DMPNN_KEEP_ROWS", "DMPNN_MEGA", "DMPNN_MFMA"):
        monkeypatch.delenv(k, raising=False)
    fields = ("plan_kind", "route", "keep_rows", "keep_bits", "lean")
    seen = set()
    for (nV, nE, n_mols) in ((4636, 9120, 512), (37000, 72800, 4096), (20500, 43800, 512), (166000, 355702, 4096), (9, 16, 1), (60, 130, 2)):
        for d_h in (300, 320, 512, 302):
            for (undirected, has_vd, p) in ((False, False, 0.0), (True, False, 0.0), (False, True, 0.0), (False, False, 0.2)):
                for (have_batch, have_table) in ((False, False), (True, False), (False, True)):
                    for oversize in (None, False, True):
                        for cap in (2, 1):
                            for atom in (False, True):
                                kw = dict(undirected=undirected, has_vd=has_vd, dropout_p=p, have_batch=have_batch, have_table=have_table,
                                          oversize=oversize, max_level=cap, atom=atom)
                                a = engine.train_route(nV, nE, 72, 14, d_h, 3, "selu", n_mols, **kw)
                                b = engine.train_route(nV, nE, 72, 14, d_h, 3, "elu", n_mols, **kw)
                                got, want = tuple(getattr(a, f) for f in fields), tuple(getattr(b, f) for f in fields)
                                assert got == want, (nV, d_h, kw, got, want)
                                assert not a.keep_bits and not a.lean                    # (no sign bits, never the lean route)
                                assert not (p > 0 and a.plan_kind == 2)                  # (no mask in the tile kernels)
                                seen.add((a.plan_kind, _lib.ROUTES[a.route]))
    assert (2, "mega16") in seen and (0, "general16") in seen


def test_forward_route_answers_for_selu_as_for_elu():
    lib = _lib.load()

    def args(nV, nE, act, d_h=300, d_v=72, d_e=14, flags=0, **kw):
        a = _lib.FwdArgs()
        a.n_atoms, a.n_edges, a.d_v, a.d_e, a.d_h, a.depth, a.flags = nV, nE, d_v, d_e, d_h, 3, flags
        a.ldv, a.lde, a.ldh, a.ldout = d_v, d_e, (d_h + 3) // 4 * 4, d_h
        for f in ("V", "E", "W_i", "W_h", "H0", "Ms", "Mv"):
            setattr(a, f, PTR)
        a.act = _lib.ACT[act]
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    shapes = [dict(nV=4636, nE=9120), dict(nV=37000, nE=73000, flags=_lib.F_LOADER_TILES), dict(nV=300, nE=600),
              dict(nV=12000, nE=25000, d_h=512), dict(nV=12000, nE=25000, d_h=1024), dict(nV=300, nE=600, d_h=1024),
              dict(nV=4636, nE=9120, flags=_lib.F_UNDIRECTED), dict(nV=37000, nE=73000, flags=_lib.F_UNDIRECTED),
              dict(nV=4636, nE=9120, d_e=13), dict(nV=37000, nE=73000, flags=_lib.F_LOADER_TILES, depth=1),
              dict(nV=37000, nE=73000, flags=_lib.F_LOADER_TILES, dropout_p=0.5),
              dict(nV=4636, nE=9120, W_d=PTR, d_vd=8, V_d=PTR, ldvd=8)]
    seen = set()
    for s in shapes:
        for keep in (0, 1):
            for cap in (2, 1, 0):
                for plan in (0, 1, 2):
                    for arith in (0, 1):
                        r = [lib.dmpnn_forward_route(C.byref(args(act=act, **s)), keep, cap, plan, arith) for act in ("selu", "elu")]
                        assert r[0] == r[1], (s, keep, cap, plan, arith, r)
                        seen.add(r[0])
    # training at size beyond the tile: the per-step general route on the f16 pipe, not the lean step kernels (ReLU class only)
    big = dict(nV=37000, nE=73000, flags=_lib.F_LOADER_TILES)
    R = {n: i for i, n in enumerate(_lib.ROUTES)}
    assert lib.dmpnn_forward_route(C.byref(args(act="selu", **big)), 1, 1, 0, 0) == R["general16"]
    assert lib.dmpnn_forward_route(C.byref(args(act="relu", **big)), 1, 1, 0, 0) == R["fused16"]
    assert {R["mega16"], R["mega"], R["fused16"], R["fused"], R["general16"], R["general"], -1} <= seen
    # the sign-bit workspace rule: none for selu (dmpnn_forward_keep_bits_bytes), as for elu
    need = _lib.F_TILE_PLAN | _lib.F_KEEP | _lib.F_MEGA | _lib.F_SPLIT16 | _lib.F_FUSED
    lib.dmpnn_forward_keep_bits_bytes.restype = C.c_size_t
    assert lib.dmpnn_forward_keep_bits_bytes(C.byref(args(4636, 9120, "relu", flags=need))) > 0
    assert lib.dmpnn_forward_keep_bits_bytes(C.byref(args(4636, 9120, "selu", flags=need))) == 0
    lean = _lib.F_KEEP | _lib.F_SPLIT16 | _lib.F_FUSED
    assert lib.dmpnn_forward_keep_bits_bytes(C.byref(args(37000, 73000, "relu", flags=lean))) > 0
    assert lib.dmpnn_forward_keep_bits_bytes(C.byref(args(37000, 73000, "selu", flags=lean))) == 0


# ---- the argument checks: every case is answered on the host, before any device work -------------------------------------------------
def _fwd(act, flags=0, p=0.0, d_h=300, **ptrs):
    a = _lib.FwdArgs()
    a.n_atoms, a.n_edges, a.d_v, a.d_e, a.d_h, a.depth, a.flags = 200, 420, 72, 14, d_h, 3, flags
    a.ldv, a.lde, a.ldh, a.ldout = 72, 14, (d_h + 3) // 4 * 4, d_h
    a.act, a.dropout_p = act, p
    for f in ("plan", "V", "E", "W_i", "W_h", "W_o", "b_o", "H0", "Hs", "Ms", "Mv", "out", "msplit", "wsplit"):
        setattr(a, f, ptrs.get(f, PTR))
    a.n_mslots = a.n_hslots = 2
    a.wsplit_bytes = 1 << 40
    return a


def _msg():
    return _lib.load().dmpnn_last_error_string().decode(errors="replace")


def test_forward_takes_code_6_and_refuses_code_7():
    lib = _lib.load()
    # (a null weight is the first check behind the activation's: reaching it says the activation passed)
    assert int(lib.dmpnn_forward(C.byref(_fwd(6, W_i=None)), None)) == EINVAL and "null weight" in _msg()
    assert int(lib.dmpnn_forward(C.byref(_fwd(5, W_i=None)), None)) == EINVAL and "null weight" in _msg()
    for bad in (7, 0, -1, 100):
        assert int(lib.dmpnn_forward(C.byref(_fwd(bad, W_i=None)), None)) == EINVAL and f"activation {bad} is not built in" in _msg(), bad
    assert int(lib.dmpnn_forward(C.byref(_fwd(3, W_i=None)), None)) == EINVAL and "PReLU needs act_slope_ptr" in _msg()


def test_a_dropout_forward_with_mega_and_selu_is_refused():
    """The mask of the tile kernels is recovered from a sign: a smooth activation cannot carry it (the rule is a whitelist)."""
    lib = _lib.load()
    tile = _lib.F_FUSED | _lib.F_MEGA | _lib.F_SPLIT16 | _lib.F_KEEP
    for act in (4, 5, 6):
        for flags in (tile, tile | _lib.F_TILE_PLAN):
            rc = int(lib.dmpnn_forward(C.byref(_fwd(act, flags=flags, p=0.2)), None))
            msg = _msg()
            assert rc == EINVAL and "dropout inside the kernels" in msg and "ReLU-class" in msg, (act, rc, msg)


def test_the_row_kernels_dropout_rule_takes_selu_and_not_prelu():
    lib = _lib.load()
    rows = _lib.F_SPLIT16 | _lib.F_KEEP
    a = _fwd(3, flags=rows, p=0.2, d_h=400)
    a.act_slope_ptr = PTR
    assert int(lib.dmpnn_forward(C.byref(a), None)) == EINVAL and "selu (not PReLU)" in _msg()
    # SELU: past the activation rule of rows_dropout_check, stopped by the one behind it (d_h <= 1024)
    assert int(lib.dmpnn_forward(C.byref(_fwd(6, flags=rows, p=0.2, d_h=1028)), None)) == EINVAL and "d_h <= 1024" in _msg()


def _bwd(act, gout=PTR):
    b = _lib.BwdArgs()
    b.f = _fwd(act, flags=_lib.F_KEEP)
    b.gout, b.ldgout = gout, b.f.d_h
    b.gW_i = b.gW_h = b.gW_o = b.gb_o = PTR
    b.ws, b.ws_bytes = PTR, 1 << 40
    return b


def test_backward_takes_code_6_and_refuses_code_7_and_prelu():
    lib = _lib.load()
    for act in (5, 6):   # (a null gout is a later check)
        assert int(lib.dmpnn_backward(C.byref(_bwd(act, gout=None)), None)) == EINVAL and "null gout" in _msg(), act
    for bad in (7, 3, 0):
        assert int(lib.dmpnn_backward(C.byref(_bwd(bad, gout=None)), None)) == EINVAL and f"activation {bad} has no fused backward" in _msg(), bad


def test_backward_inputs_takes_code_6_and_refuses_code_7_and_prelu():
    lib = _lib.load()

    def call(act):
        a = _lib.BwdInputsArgs()
        C.memmove(C.byref(a.b), C.byref(_bwd(act)), C.sizeof(_lib.BwdArgs))
        a.b.f.W_i = None   # (null weights: a later check)
        a.gV, a.ldgv = PTR, 72
        return int(lib.dmpnn_backward_inputs(C.byref(a), None)), _msg()

    for act in (5, 6):
        rc, msg = call(act)
        assert rc == EINVAL and "null weights" in msg, (act, msg)
    rc, msg = call(7)
    assert rc == EINVAL and "activation 7 has no fused backward" in msg
    rc, msg = call(3)
    assert rc == EINVAL and "PReLU" in msg


def _head(act, loss=0):
    h = _lib.HeadArgs()
    h.n_atoms, h.n_mols, h.d_h, h.batch = 10, 4, 8, PTR
    h.n_layers, h.act = 2, act
    for i, v in enumerate((8, 8, 1)):
        h.dims[i] = v
    h.W[0] = h.W[1] = PTR
    h.preds, h.targets, h.loss_out, h.loss = PTR, PTR, PTR, loss
    return h


def test_head_and_predict_head_take_code_6_and_refuse_code_7_and_prelu():
    lib = _lib.load()
    for act in (0, 5, 6):
        # well-formed: stopped by the workspace rule, which comes behind every argument rule
        assert lib.dmpnn_head(C.byref(_head(act)), PTR, 8, None) == ENOSPC and "workspace" in _msg(), act
        # ... and an unknown criterion is the rule right behind the activation's
        assert lib.dmpnn_head(C.byref(_head(act, loss=99)), PTR, 8, None) == EINVAL and "unknown criterion" in _msg(), act
        p = _lib.PredictArgs()
        C.memmove(C.byref(p.head), C.byref(_head(act)), C.sizeof(_lib.HeadArgs))
        assert lib.dmpnn_predict_head(C.byref(p), PTR, 8, None) == ENOSPC and "workspace" in _msg(), act
    for bad in (7, 3, -1):
        assert lib.dmpnn_head(C.byref(_head(bad)), PTR, 8, None) == EINVAL and f"activation {bad} is not built in" in _msg(), bad
        p = _lib.PredictArgs()
        C.memmove(C.byref(p.head), C.byref(_head(bad)), C.sizeof(_lib.HeadArgs))
        assert lib.dmpnn_predict_head(C.byref(p), PTR, 8, None) == EINVAL and f"activation {bad} is not built in" in _msg(), bad
