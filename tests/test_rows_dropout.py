"""Block dropout in the row kernels of the per-step general route on the f16 pipe (``DMPNN_F_SPLIT16 | DMPNN_F_KEEP`` without
``DMPNN_F_FUSED``; include/dmpnn.h, ``dmpnn_fwd_args.dropout_p``: its third home): the host side that needs no GPU — the argument
checks of ``dmpnn_forward`` and ``dmpnn_linear16_dropout_fwd``, which run before anything reaches the device, the host's own
statement of the conditions, and the keyword that lets a block with a smooth activation into the one-call step."""
import ctypes as C

import pytest
from torch import nn

from chemprop_amd import _lib, engine

EINVAL = -1
ROWS = _lib.F_SPLIT16 | _lib.F_KEEP


def _args(flags=ROWS, act="relu", p=0.2, depth=3, d_h=400, d_v=72, d_e=14, nV=200, nE=420, wd=None, ldh=None):
    a = _lib.FwdArgs()
    a.n_atoms, a.n_edges, a.d_v, a.d_e, a.d_h, a.depth, a.flags = nV, nE, d_v, d_e, d_h, depth, flags
    a.ldv, a.lde, a.ldh, a.ldout = d_v, d_e, (d_h + 3) // 4 * 4 if ldh is None else ldh, d_h
    a.act, a.dropout_p, a.W_d = _lib.ACT[act], p, wd
    return a


def _call(a, **ptrs):
    """``dmpnn_forward`` on placeholders nothing dereferences: every case below is refused on the host."""
    lib = _lib.load()
    for f in ("plan", "V", "E", "W_i", "W_h", "W_o", "b_o", "H0", "Hs", "Ms", "Mv", "out", "msplit", "wsplit"):
        setattr(a, f, ptrs.get(f, 4096))
    if a.W_d:
        a.d_vd, a.V_d, a.b_d, a.Hv, a.ldvd, a.ldout = 4, 4096, 4096, 4096, 4, a.d_h + 4
    if a.act == _lib.ACT["prelu"]:
        a.act_slope_ptr = 4096
    a.n_mslots = a.n_hslots = 2
    a.wsplit_bytes = 1 << 40
    rc = int(lib.dmpnn_forward(C.byref(a), None))
    return rc, lib.dmpnn_last_error_string().decode(errors="replace")


REFUSED = [
    ("prelu", dict(act="prelu"), "PReLU"),
    ("W_d", dict(wd=4096), "W_d"),
    ("undirected", dict(flags=ROWS | _lib.F_UNDIRECTED), "directed"),
    ("d_h>1024", dict(d_h=1028), "1024"),
    ("odd-d_h-update", dict(d_h=301, ldh=301), "update contraction"),         # (K1 = d_h odd: the fp32-MFMA kernel would run it)
    ("odd-d_h-depth1", dict(d_h=301, ldh=301, depth=1), "finalize contraction"),
    ("odd-d_v-finalize", dict(d_v=73), "finalize contraction"),
    ("p>=1", dict(p=1.0), "dropout_p"),
    ("p<0", dict(p=-0.1), "dropout_p"),
]


@pytest.mark.parametrize("name,kw,word", REFUSED, ids=[r[0] for r in REFUSED])
def test_forward_refuses_rows_dropout_outside_its_conditions_before_any_device_work(name, kw, word):
    rc, msg = _call(_args(**kw))
    assert rc == EINVAL and "dropout" in msg and word in msg, (name, rc, msg)


def test_forward_refuses_a_misaligned_operand_of_a_masked_contraction():
    # the message slots 4-byte aligned: the update contraction would leave k_rows16
    rc, msg = _call(_args(), Ms=4100)
    assert rc == EINVAL and "dropout" in msg and "update contraction" in msg, (rc, msg)
    rc, msg = _call(_args(), Mv=4100)
    assert rc == EINVAL and "dropout" in msg and "finalize contraction" in msg, (rc, msg)


def test_the_other_routes_refuse_dropout_as_before():
    """What tests/test_lean_dropout.py pins, at this file's shapes: the fp32 general route, the fp32 fused route, the per-step fused
    route on the f16 pipe without ``keep_bits``, and the general route on the f16 pipe WITHOUT ``DMPNN_F_KEEP`` (inference)."""
    for flags in (_lib.F_KEEP, _lib.F_FUSED | _lib.F_KEEP, _lib.F_FUSED | _lib.F_SPLIT16, _lib.F_FUSED | _lib.F_SPLIT16 | _lib.F_KEEP,
                  _lib.F_SPLIT16, 0, _lib.F_MEGA | _lib.F_SPLIT16 | _lib.F_KEEP):
        rc, msg = _call(_args(flags=flags, d_h=300))
        assert rc == EINVAL and "dropout" in msg, (flags, rc, msg)


def test_linear16_dropout_fwd_is_exported_and_checks_its_arguments_on_the_host():
    assert "dmpnn_linear16_dropout_fwd" in _lib.EXPORTS
    lib = _lib.load()
    assert hasattr(lib, "dmpnn_linear16_dropout_fwd")

    def call(N=64, p=0.3, site=1, C_=4096, M=48, K1=32):
        g = _lib.GemmArgs()
        g.M, g.N, g.K1, g.K2 = M, N, K1, 0
        g.A1, g.lda1, g.W, g.ldw = 4096, K1, 4096, K1
        g.C, g.ldc, g.Zpre, g.ldz = C_, N, 4096, N
        rc = int(lib.dmpnn_linear16_dropout_fwd(C.byref(g), 4096, 1 << 40, 0, p, 5, site, None))
        return rc, lib.dmpnn_last_error_string().decode(errors="replace")

    for kw in (dict(N=1028), dict(p=0.0), dict(p=1.0), dict(p=-0.5), dict(site=-1), dict(C_=None)):
        rc, msg = call(**kw)
        assert rc == EINVAL and "dropout" in msg, (kw, rc, msg)
    rc, msg = call(K1=33)                                                     # (what dmpnn_linear16_fwd refuses, it refuses)
    assert rc == EINVAL and "linear16" in msg, (rc, msg)


def test_rows_dropout_refusal_names_the_failed_condition():
    r = engine.rows_dropout_refusal
    for act in ("none", "relu", "leakyrelu", "tanh", "elu"):
        assert r(72, 14, 400, 3, act) is None
    assert r(72, 14, 1024, 1, "tanh") is None and r(72, 14, 302, 4, "elu") is None and r(106, 28, 64, 2, "relu", False, False) is None
    assert "prelu" in r(72, 14, 400, 3, "prelu") and "custom" in r(72, 14, 400, 3, "custom")
    assert "W_d" in r(72, 14, 400, 3, "relu", True)
    assert "undirected" in r(72, 14, 400, 3, "relu", False, True)
    assert "1024" in r(72, 14, 1028, 3, "relu")
    assert "odd d_h" in r(72, 14, 301, 3, "relu")
    assert "odd d_v" in r(73, 14, 400, 3, "relu")
    assert "depth" in r(72, 14, 400, 0, "relu")
    # ... and agrees with the library's argument checks on the shape conditions
    for (dv, dh, depth, act, wd, und) in ((72, 400, 3, "relu", None, 0), (72, 1028, 3, "relu", None, 0), (72, 301, 3, "relu", None, 0),
                                          (73, 400, 3, "relu", None, 0), (72, 400, 3, "prelu", None, 0), (72, 400, 3, "tanh", 4096, 0),
                                          (72, 400, 3, "elu", None, _lib.F_UNDIRECTED)):
        if r(dv, 14, dh, depth, act, wd is not None, bool(und)) is None:
            continue                                                          # (a taken case would launch: not on this machine)
        rc, msg = _call(_args(flags=ROWS | und, act=act, depth=depth, d_h=dh, d_v=dv, wd=wd, ldh=dh if dh % 2 else None))
        assert rc == EINVAL and "dropout" in msg, (dv, dh, depth, act, rc, msg)


def test_fused_block_takes_a_smooth_activation_with_dropout_only_on_request():
    from chemprop_amd.model import fused_block
    from chemprop_amd.nn import BondMessagePassing

    for act in ("tanh", "elu"):
        mp = BondMessagePassing(d_h=64, activation=act, dropout=0.2)
        with pytest.raises(NotImplementedError, match="ReLU"):
            fused_block(mp)
        assert fused_block(mp, rows_dropout=True)[0] == act
    relu = BondMessagePassing(d_h=400, dropout=0.2)
    assert fused_block(relu)[0] == fused_block(relu, rows_dropout=True)[0] == "relu"
    # what stays refused with the keyword: PReLU, undirected, W_d + dropout, a dropout module that is not nn.Dropout
    for kw in (dict(activation="prelu"), dict(undirected=True), dict(d_vd=4)):
        with pytest.raises(NotImplementedError):
            fused_block(BondMessagePassing(d_h=64, dropout=0.2, **kw), rows_dropout=True)
    odd = BondMessagePassing(d_h=64, activation="tanh", dropout=0.2)
    odd.dropout = nn.AlphaDropout(0.2)
    with pytest.raises(NotImplementedError):
        fused_block(odd, rows_dropout=True)
