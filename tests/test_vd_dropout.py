"""Block dropout behind the atom-descriptor layer (the reference applies the block's ``nn.Dropout`` once more behind ``W_d``,
``message_passing/base.py:185-188``) as a mask site of the stage's own kernels: ``dmpnn_vd_args.dropout_p`` / ``dropout_seed``,
``DMPNN_DROP_SITE_VD`` and ``fused_block(..., vd_dropout=True)`` — everything that needs no GPU."""
import ctypes as C

import numpy as np
import pytest
import torch

from chemprop_amd import _lib
from oracle.dropout_hash import keep_mask
from test_atom_descriptors import _step, _vd

EINVAL, ENOSPC = -1, -3


def test_vd_args_end_in_the_dropout_fields():
    names = [n for n, _ in _lib.VdArgs._fields_]
    assert names[-2:] == ["dropout_p", "dropout_seed"]
    assert names[-4:-2] == ["ws", "ws_bytes"]   # (grown at its end: an older caller's block is a prefix)
    assert dict(_lib.VdArgs._fields_)["dropout_p"] is C.c_float and dict(_lib.VdArgs._fields_)["dropout_seed"] is C.c_uint64


def test_grown_vd_struct_matches_the_c_layout(tmp_path):
    """``dmpnn_vd_args`` with its two new fields at the offsets the C compiler gives them; ``dmpnn_step_args`` still ends in ``vd``;
    the header's site constant is the package's."""
    import os
    import shutil
    import subprocess

    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if cc is None:
        cc = "/opt/rocm/llvm/bin/clang"
    fields = [n for n, _ in _lib.VdArgs._fields_]
    assert "dropout_p" in fields and "dropout_seed" in fields
    fmt = " ".join(["%zu"] * (len(fields) + 4))
    offs = ",".join(f"offsetof(dmpnn_vd_args, {n})" for n in fields)
    src = tmp_path / "off.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "dmpnn.h"\nint main(void){printf("' + fmt + '\\n",' + offs +
                   ',sizeof(dmpnn_vd_args), offsetof(dmpnn_step_args, vd), sizeof(dmpnn_step_args), (size_t)DMPNN_DROP_SITE_VD);return 0;}\n')
    exe = tmp_path / "off"
    inc = os.path.join(os.path.dirname(_lib.__file__), "..", "include")
    subprocess.run([cc, "-I", inc, str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    want = [getattr(_lib.VdArgs, n).offset for n in fields] + [C.sizeof(_lib.VdArgs), _lib.StepArgs.vd.offset, C.sizeof(_lib.StepArgs),
                                                               _lib.DROP_SITE_VD]
    assert got == want
    assert _lib.StepArgs._fields_[-1][0] == "vd"
    assert _lib.ABI_VERSION == 15


def test_the_site_behind_the_layer_is_pinned():
    """``DROP_SITE_VD`` is 0x8000 — between the block's sites (``0 .. depth-1``) and the predictor's (from 0x10000) — and the library's
    host twin of the device hash agrees with the oracle there over the widest layer's columns."""
    lib = _lib.load()
    assert _lib.DROP_SITE_VD == 0x8000 < _lib.DROP_SITE_FFN
    site = _lib.DROP_SITE_VD
    for seed, p in ((0x1234_5678_9ABC, 0.1), (3, 0.5)):
        got = np.array([[lib.dmpnn_dropout_keep(C.c_uint64(seed), site, r, c, C.c_float(p)) for c in range(544)] for r in range(97)], dtype=bool)
        assert np.array_equal(got, keep_mask(seed, site, 97, 544, p)), (seed, p)


def _call(a, which):
    lib = _lib.load()
    fn = lib.dmpnn_vd_forward if which == "fwd" else lib.dmpnn_vd_backward
    return int(fn(C.byref(a), None)), lib.dmpnn_last_error_string().decode()


@pytest.mark.parametrize("which", ("fwd", "bwd"))
def test_stage_refuses_a_dropout_outside_the_unit_interval(which):
    """``0 <= p < 1`` or ``DMPNN_EINVAL`` naming dropout, on made-up addresses: before any device work."""
    for p in (-0.1, 1.0, 1.5):
        rc, msg = _call(_vd(dropout_p=p, dropout_seed=7), which)
        assert rc == EINVAL and "dropout" in msg, (which, p, rc, msg)


@pytest.mark.parametrize("which", ("fwd", "bwd"))
def test_a_valid_dropout_passes_the_checks_in_the_old_order(which):
    """``p = 0.3`` is past the new check: a block that is otherwise refused for a LATER reason (a leading dimension, the workspace) is
    refused for that reason; one refused for an EARLIER reason (the width) keeps that reason even with a bad ``p``."""
    rc, msg = _call(_vd(dropout_p=0.3, dropout_seed=7, ldhv=299), which)
    assert rc == EINVAL and "leading dimension" in msg and "dropout" not in msg, (rc, msg)
    good = _vd(dropout_p=0.3, dropout_seed=7)
    assert good.ws_bytes == _vd().ws_bytes   # (no workspace for the mask: it is regenerated)
    rc, msg = _call(_vd(dropout_p=0.3, dropout_seed=7, ws_bytes=good.ws_bytes - 1), which)
    assert rc == ENOSPC and "workspace too small" in msg, (rc, msg)
    rc, msg = _call(_vd(d_h=400, d_vd=200, ws_bytes=1 << 30, dropout_p=1.5), which)
    assert rc == EINVAL and "beyond" in msg, (rc, msg)
    assert _vd().dropout_p == 0.0 and _call(_vd(n=0, dropout_p=0.3), "fwd")[0] == 0


def test_step_requires_the_blocks_own_dropout_behind_the_layer():
    """One ``nn.Dropout`` module in the reference: ``vd.dropout_p > 0`` needs the block's ``p`` and seed."""
    lib = _lib.load()

    def call(s):
        return int(lib.dmpnn_train_step(C.byref(s), None)), lib.dmpnn_last_error_string().decode()

    p32 = C.c_float(0.2).value
    vd = _vd(dropout_p=0.2, dropout_seed=99)
    rc, msg = call(_step(vd))                                                          # the block without dropout
    assert rc == EINVAL and "atom-descriptor" in msg and "dropout" in msg, (rc, msg)
    rc, msg = call(_step(vd, **{"bwd.f.dropout_p": 0.2, "bwd.f.dropout_seed": 98}))      # equal p, another seed
    assert rc == EINVAL and "atom-descriptor" in msg and "dropout" in msg, (rc, msg)
    rc, msg = call(_step(vd, **{"bwd.f.dropout_p": 0.25, "bwd.f.dropout_seed": 99}))     # another p
    assert rc == EINVAL and "atom-descriptor" in msg and "dropout" in msg, (rc, msg)
    # the block's own p and seed: past this rule — the stage's own checks speak next (a workspace one byte short; still no launch)
    short = _vd(dropout_p=0.2, dropout_seed=99, ws_bytes=vd.ws_bytes - 1)
    rc, msg = call(_step(short, **{"bwd.f.dropout_p": p32, "bwd.f.dropout_seed": 99}))
    assert rc == ENOSPC and "workspace too small" in msg, (rc, msg)
    rc, msg = call(_step(short, **{"bwd.f.dropout_p": p32, "bwd.f.dropout_seed": 98}))
    assert rc == EINVAL and "dropout" in msg, (rc, msg)
    # a stage without dropout behind a block with it is not this rule's business
    rc, msg = call(_step(_vd(ws_bytes=vd.ws_bytes - 1), **{"bwd.f.dropout_p": p32, "bwd.f.dropout_seed": 99}))
    assert rc == ENOSPC and "workspace too small" in msg, (rc, msg)


def test_fused_block_takes_atom_descriptors_with_dropout_on_request():
    from chemprop_amd.model import fused_block
    from chemprop_amd.nn import BondMessagePassing

    blk = lambda **kw: BondMessagePassing(d_vd=5, dropout=0.2, **kw)
    # the defaults keep the refusals
    for kw in (dict(), dict(rows_dropout=True)):
        with pytest.raises(NotImplementedError, match="W_d"):
            fused_block(blk(), **kw)
    assert fused_block(blk(), vd_dropout=True) == fused_block(BondMessagePassing())
    assert fused_block(blk(), vd_dropout=True)[0] == "relu"
    with pytest.raises(NotImplementedError, match="ReLU"):
        fused_block(blk(activation="tanh"), vd_dropout=True)
    assert fused_block(blk(activation="tanh"), vd_dropout=True, rows_dropout=True)[0] == "tanh"
    for kw in (dict(activation="prelu"), dict(undirected=True)):
        with pytest.raises(NotImplementedError):
            fused_block(blk(**kw), vd_dropout=True, rows_dropout=True)
    alpha = blk()
    alpha.dropout = torch.nn.AlphaDropout(0.2)
    with pytest.raises(NotImplementedError, match="nn.Dropout"):
        fused_block(alpha, vd_dropout=True)
    with pytest.raises(NotImplementedError, match="beyond"):
        fused_block(BondMessagePassing(d_h=400, d_vd=200, dropout=0.2), vd_dropout=True)
    # without dropout the keyword changes nothing
    assert fused_block(BondMessagePassing(d_vd=5), vd_dropout=True) == fused_block(BondMessagePassing(d_vd=5))
