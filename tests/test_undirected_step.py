"""Undirected bond blocks on the one-call step, the host side that needs no GPU: ``fused_block(mp, undirected=True)``, the argument
checks of ``dmpnn_forward`` / ``dmpnn_backward`` around ``DMPNN_F_UNDIRECTED_MASK`` (dropout in the row kernels of the per-step general
route with undirected messages), which run before anything reaches the device, and the host's own statement of the conditions.

``dmpnn_backward``: its flag check sits among the first argument checks, and for a block without ``W_d`` whose forward was neither the
lean form nor a tile-kernel forward the dropout check (``rows_drop``) is reached before the first launch (csrc/dmpnn_backward.hip:
``backward_impl``) — so both are called here on placeholder pointers, like the forward."""
import ctypes as C
import os
import re

import pytest
from torch import nn

from chemprop_amd import _lib, engine
from test_rows_dropout import EINVAL, ROWS, _args, _call

UND = ROWS | _lib.F_UNDIRECTED
MASK = _lib.F_UNDIRECTED_MASK
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- fused_block ----------------------------------------------------------------------------------------------------------------------
def _bond(**kw):
    from chemprop_amd.nn import BondMessagePassing

    return BondMessagePassing(d_h=kw.pop("d_h", 64), undirected=True, **kw)


ALL = dict(rows_dropout=True, vd_dropout=True, atom_messages=True, undirected=True)


def test_fused_block_refuses_an_undirected_block_by_default():
    from chemprop_amd.model import fused_block

    for kw in (dict(), dict(rows_dropout=True, vd_dropout=True, atom_messages=True)):
        with pytest.raises(NotImplementedError, match="directed"):
            fused_block(_bond(), **kw)


@pytest.mark.parametrize("act", ["relu", "leakyrelu", "tanh", "elu"])
def test_fused_block_takes_an_undirected_block_on_request(act):
    from chemprop_amd.model import fused_block

    assert fused_block(_bond(activation=act), undirected=True)[0] == act
    # p = 0.2: its only dropout home is the row kernels — rows_dropout=True as well, whatever the activation
    mp = _bond(activation=act, dropout=0.2)
    with pytest.raises(NotImplementedError, match="rows_dropout"):
        fused_block(mp, undirected=True)
    assert fused_block(mp, undirected=True, rows_dropout=True)[0] == act
    # a directed block answers as before, with or without the keyword
    from chemprop_amd.nn import BondMessagePassing

    d = BondMessagePassing(d_h=64, activation=act)
    assert fused_block(d) == fused_block(d, undirected=True)


def test_fused_block_undirected_with_atom_descriptors():
    from chemprop_amd.model import fused_block

    assert fused_block(_bond(d_vd=5), undirected=True)[0] == "relu"          # (the stage behind the block: unchanged)
    mp = _bond(d_vd=5, dropout=0.2)
    with pytest.raises(NotImplementedError, match="W_d"):
        fused_block(mp, undirected=True, rows_dropout=True)
    with pytest.raises(NotImplementedError, match="rows_dropout"):
        fused_block(mp, undirected=True, vd_dropout=True)
    assert fused_block(mp, undirected=True, rows_dropout=True, vd_dropout=True)[0] == "relu"


def test_fused_block_still_refuses_with_every_keyword():
    from chemprop_amd import agg as cagg
    from chemprop_amd.model import FusedTrainer, MulticomponentMPNN, RegressionFFN, fused_block
    from chemprop_amd.nn import AtomMessagePassing, BondMessagePassing, MulticomponentMessagePassing

    with pytest.raises(NotImplementedError):
        fused_block(_bond(activation="prelu"), **ALL)
    odd = _bond(activation="tanh", dropout=0.2)
    odd.dropout = nn.AlphaDropout(0.2)
    with pytest.raises(NotImplementedError):
        fused_block(odd, **ALL)
    with pytest.raises(NotImplementedError):
        fused_block(AtomMessagePassing(d_h=64, undirected=True), **ALL)
    assert fused_block(AtomMessagePassing(d_h=64), **ALL)[0] == "relu"       # (the directed atom block: as before)
    # a multicomponent model with an undirected block: refused at construction, before any parameter is looked at
    blocks = [BondMessagePassing(d_h=64), _bond()]
    mcmp = MulticomponentMessagePassing(blocks, 2)
    model = MulticomponentMPNN(mcmp, cagg.MeanAggregation(), RegressionFFN(input_dim=mcmp.output_dim))
    with pytest.raises(NotImplementedError):
        FusedTrainer(model, ffn_dropout=True, **ALL)


# ---- dmpnn_forward on placeholder pointers --------------------------------------------------------------------------------------------
def test_forward_refuses_undirected_dropout_without_the_flag_as_before():
    rc, msg = _call(_args(flags=UND))
    assert rc == EINVAL and "dropout" in msg and "directed" in msg, (rc, msg)


REFUSED_WITH_THE_FLAG = [
    ("prelu", dict(act="prelu"), "PReLU"),
    ("W_d", dict(wd=4096), "W_d"),
    ("d_h>1024", dict(d_h=1028), "1024"),
    ("odd-d_h", dict(d_h=301, ldh=301), "update contraction"),
    ("odd-d_v", dict(d_v=73), "finalize contraction"),
    ("p=1", dict(p=1.0), "dropout_p"),
]


@pytest.mark.parametrize("name,kw,word", REFUSED_WITH_THE_FLAG, ids=[r[0] for r in REFUSED_WITH_THE_FLAG])
def test_forward_keeps_every_other_condition_of_the_row_kernels_with_the_flag(name, kw, word):
    rc, msg = _call(_args(flags=UND | MASK, **kw))
    assert rc == EINVAL and "dropout" in msg and word in msg, (name, rc, msg)


BAD_FLAGS = [
    ("no-undirected", ROWS | MASK),
    ("fused", UND | MASK | _lib.F_FUSED),
    ("mega", UND | MASK | _lib.F_MEGA),
    ("tile-plan", UND | MASK | _lib.F_TILE_PLAN),
    ("atom", UND | MASK | _lib.F_ATOM),
]


@pytest.mark.parametrize("name,flags", BAD_FLAGS, ids=[b[0] for b in BAD_FLAGS])
@pytest.mark.parametrize("p", [0.2, 0.0])
def test_forward_refuses_the_flag_outside_its_route(name, flags, p):
    rc, msg = _call(_args(flags=flags, p=p, d_h=300))
    assert rc == EINVAL and "DMPNN_F_UNDIRECTED_MASK" in msg, (name, rc, msg)


# ---- dmpnn_backward on placeholder pointers -------------------------------------------------------------------------------------------
def _bwd(flags, p=0.2, **kw):
    lib = _lib.load()
    b = _lib.BwdArgs()
    f = _args(flags=flags, p=p, **kw)
    for name in ("plan", "V", "E", "W_i", "W_h", "W_o", "b_o", "H0", "Hs", "Ms", "Mv", "out", "wsplit"):
        setattr(f, name, 4096)
    f.n_mslots = f.n_hslots = f.depth - 1
    f.wsplit_bytes = 1 << 40
    b.f = f
    b.gout, b.ldgout = 4096, f.d_h
    b.gW_i = b.gW_h = b.gW_o = b.gb_o = 4096
    b.ws, b.ws_bytes = 4096, 1 << 40
    rc = int(lib.dmpnn_backward(C.byref(b), None))
    return rc, lib.dmpnn_last_error_string().decode(errors="replace")


def test_backward_refuses_undirected_dropout_without_the_flag_as_before():
    rc, msg = _bwd(UND)
    assert rc == EINVAL and "dropout" in msg, (rc, msg)


@pytest.mark.parametrize("name,flags", BAD_FLAGS, ids=[b[0] for b in BAD_FLAGS])
@pytest.mark.parametrize("p", [0.2, 0.0])
def test_backward_refuses_the_flag_outside_its_route(name, flags, p):
    rc, msg = _bwd(flags, p=p, d_h=300)
    assert rc == EINVAL and "DMPNN_F_UNDIRECTED_MASK" in msg, (name, rc, msg)


def test_backward_with_the_flag_still_refuses_what_the_row_kernels_do_not_carry():
    rc, msg = _bwd(UND | MASK, d_h=1028)                                      # (beyond the hash key's 1024 columns)
    assert rc == EINVAL and "dropout" in msg, (rc, msg)


# ---- the host's statement of the conditions -------------------------------------------------------------------------------------------
def test_rows_dropout_refusal_with_and_without_the_keyword():
    r = engine.rows_dropout_refusal
    assert "undirected" in r(72, 14, 400, 3, "relu", False, True)
    assert "undirected" in r(72, 14, 400, 3, "relu", undirected=True, undirected_dropout=False)
    for act in ("none", "relu", "leakyrelu", "tanh", "elu"):
        assert r(72, 14, 400, 3, act, undirected=True, undirected_dropout=True) is None
    assert r(72, 14, 400, 3, "relu", undirected_dropout=True) is None         # (a directed block: the keyword changes nothing)
    # every other reason stands with the keyword
    assert "prelu" in r(72, 14, 400, 3, "prelu", undirected=True, undirected_dropout=True)
    assert "W_d" in r(72, 14, 400, 3, "relu", True, True, undirected_dropout=True)
    assert "1024" in r(72, 14, 1028, 3, "relu", undirected=True, undirected_dropout=True)
    assert "odd d_h" in r(72, 14, 301, 3, "relu", undirected=True, undirected_dropout=True)
    assert "odd d_v" in r(73, 14, 400, 3, "relu", undirected=True, undirected_dropout=True)
    assert "undirected" in r(72, 14, 400, 3, "relu", False, True, True, undirected_dropout=True)   # (an atom block is directed)


def test_the_flag_is_bit_12_in_the_header_too_and_the_abi_stays_15():
    assert _lib.F_UNDIRECTED_MASK == 1 << 12
    src = open(os.path.join(ROOT, "include", "dmpnn.h")).read()
    m = re.search(r"DMPNN_F_UNDIRECTED_MASK\s*=\s*1u\s*<<\s*(\d+)", src)
    assert m and int(m.group(1)) == 12
    bits = [int(b) for b in re.findall(r"DMPNN_F_[A-Z0-9_]+\s*=\s*1u\s*<<\s*(\d+)", src)]
    assert len(bits) == len(set(bits)), "two flags share a bit"
    assert _lib.ABI_VERSION == 15 and int(re.search(r"#define DMPNN_ABI_VERSION (\d+)", src).group(1)) == 15
    assert _lib.load().dmpnn_version() == 15
