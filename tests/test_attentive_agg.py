"""AttentiveAggregation on its own kernels and on the one-call step — everything that needs no GPU: what ``HeadSpec`` takes and
refuses with ``attentive=True``, the order of ``params()``, the argument checks of ``dmpnn_molagg_attn_*`` and of ``dmpnn_head`` in
attentive mode (error codes, before any device work: every pointer here is a dummy), and the preconditions of the GPU tests' inputs."""
import ctypes as C

import pytest
import torch
from torch import nn

import attn_harness as ah
from chemprop_amd import _lib

EINVAL, ENOSPC = -1, -3
DUMMY = 4096   # a non-NULL, 16-byte aligned address no check may dereference


def _model(agg, d_h=16, d_in=None, **mp_kw):
    from chemprop_amd.model import MPNN, RegressionFFN
    from chemprop_amd.nn import BondMessagePassing

    mp = BondMessagePassing(d_h=d_h, **mp_kw)
    return MPNN(mp, agg, RegressionFFN(n_tasks=1, input_dim=int(mp.output_dim) if d_in is None else d_in, hidden_dim=8), batch_norm=True)


def test_headspec_refuses_by_default_and_takes_the_mirror_and_the_reference_class_by_name():
    from chemprop_amd import agg as cagg
    from chemprop_amd.model import HeadSpec

    m = _model(cagg.AttentiveAggregation(output_size=16))
    with pytest.raises(NotImplementedError):
        HeadSpec(m)
    with pytest.raises(NotImplementedError):
        HeadSpec(m, attentive=False)
    spec = HeadSpec(m, attentive=True)
    assert spec.agg_mode == _lib.MOLAGG_ATTENTIVE == 3 and spec.att is m.agg.W

    class AttentiveAggregation(nn.Module):   # (the reference's class is told by its name in the MRO)
        def __init__(self, output_size):
            super().__init__()
            self.W = nn.Linear(output_size, 1)

    class Mine(AttentiveAggregation):
        pass

    for cls in (AttentiveAggregation, Mine):
        assert HeadSpec(_model(cls(16)), attentive=True).att is not None
    # the other aggregations are untouched by the switch
    assert HeadSpec(_model(cagg.MeanAggregation()), attentive=True).agg_mode == 1


def test_headspec_attentive_refusals_name_their_reason():
    from chemprop_amd import agg as cagg
    from chemprop_amd.model import HeadSpec

    with pytest.raises(NotImplementedError, match=r"nn\.Linear\(16, 1\)"):
        HeadSpec(_model(cagg.AttentiveAggregation(output_size=12)), attentive=True)
    m = _model(cagg.AttentiveAggregation(output_size=16))
    m.agg.W = nn.Linear(16, 1, bias=False)
    with pytest.raises(NotImplementedError, match="bias"):
        HeadSpec(m, attentive=True)
    m.agg.W = nn.Linear(16, 2)
    with pytest.raises(NotImplementedError, match=r"nn\.Linear\(16, 1\)"):
        HeadSpec(m, attentive=True)

    class Multi(nn.Module):   # (what a multicomponent block looks like to HeadSpec)
        def __init__(self, mp):
            super().__init__()
            self.blocks, self.n_components, self.output_dim = nn.ModuleList([mp, mp]), 2, 2 * mp.output_dim

    m = _model(cagg.AttentiveAggregation(output_size=32), d_in=32)
    m.message_passing = Multi(m.message_passing)
    with pytest.raises(NotImplementedError, match="multicomponent"):
        HeadSpec(m, attentive=True)


def test_params_lists_the_attention_first_in_model_parameters_order():
    from chemprop_amd import agg as cagg
    from chemprop_amd.model import HeadSpec

    m = _model(cagg.AttentiveAggregation(output_size=16))
    ps = HeadSpec(m, attentive=True).params()
    assert ps[0] is m.agg.W.weight and ps[1] is m.agg.W.bias
    blk = {id(p) for p in m.message_passing.parameters()}
    rest = [p for p in m.parameters() if id(p) not in blk]
    assert [id(p) for p in ps] == [id(p) for p in rest]


def test_the_atom_descriptor_stage_widens_the_attention():
    from chemprop_amd import agg as cagg
    from chemprop_amd.model import HeadSpec

    m = _model(cagg.AttentiveAggregation(output_size=21), d_h=16, d_vd=5)
    assert int(m.message_passing.output_dim) == 21
    assert HeadSpec(m, attentive=True).att.in_features == 21
    with pytest.raises(NotImplementedError):
        HeadSpec(_model(cagg.AttentiveAggregation(output_size=16), d_h=16, d_vd=5), attentive=True)


def _attn_args(n_atoms=10, n_mols=3, d=8):
    a = _lib.MolAggAttnArgs()
    a.n_atoms, a.n_mols, a.d_h = n_atoms, n_mols, d
    a.ldh = a.ldo = a.ldgo = a.ldgh = d
    for f in ("H", "batch", "bounds", "W", "b", "out", "keep_s", "keep_Z", "gout", "gH", "gW", "gb", "ws"):
        setattr(a, f, DUMMY)
    a.ws_bytes = 1 << 30
    return a


def test_molagg_attn_argument_checks_are_codes_before_any_device_work():
    lib = _lib.load()
    fwd, bwd = lib.dmpnn_molagg_attn_fwd, lib.dmpnn_molagg_attn_bwd
    assert fwd(None, None) == EINVAL and bwd(None, None) == EINVAL
    for field in ("ldh", "ldo"):
        a = _attn_args()
        setattr(a, field, 7)
        assert fwd(C.byref(a), None) == EINVAL, field
        assert b"d_h" in lib.dmpnn_last_error_string()
    for field in ("ldh", "ldgo", "ldgh"):
        a = _attn_args()
        setattr(a, field, 7)
        assert bwd(C.byref(a), None) == EINVAL, field
    a = _attn_args(d=0)
    assert fwd(C.byref(a), None) == EINVAL and bwd(C.byref(a), None) == EINVAL
    a = _attn_args()
    a.keep_Z = None   # (keep_s without keep_Z)
    assert fwd(C.byref(a), None) == EINVAL
    for field in ("H", "W", "out"):
        a = _attn_args()
        setattr(a, field, None)
        assert fwd(C.byref(a), None) == EINVAL, field
    for field in ("H", "gout", "gH", "keep_s"):
        a = _attn_args()
        setattr(a, field, None)
        if field == "keep_s":
            a.keep_Z = None
        assert bwd(C.byref(a), None) == EINVAL, field
    # the workspace: the partial rows of gW | gb in the backward pass, the bounds table when none is handed over
    a = _attn_args()
    need = int(lib.dmpnn_molagg_attn_ws_bytes(C.byref(a)))
    assert need >= 3 * (8 + 4) * 4
    a.ws_bytes = need - 1
    assert bwd(C.byref(a), None) == ENOSPC
    assert b"workspace" in lib.dmpnn_last_error_string()
    a.ws = None
    assert bwd(C.byref(a), None) == ENOSPC
    a = _attn_args()
    a.bounds = None
    own = int(lib.dmpnn_molagg_attn_ws_bytes(C.byref(a)))
    assert own >= need + int(lib.dmpnn_molagg_ws_bytes(3))
    a.ws_bytes = 8
    assert fwd(C.byref(a), None) == ENOSPC
    a = _attn_args()
    a.ws = DUMMY + 4   # (not 16-byte aligned)
    assert bwd(C.byref(a), None) == EINVAL


def test_molagg_fwd_and_bwd_still_refuse_the_attentive_mode():
    lib = _lib.load()
    assert lib.dmpnn_molagg_fwd(DUMMY, 8, 10, 8, 3, DUMMY, _lib.MOLAGG_ATTENTIVE, C.c_float(1.0), DUMMY, 8, None) == EINVAL
    assert lib.dmpnn_molagg_bwd(DUMMY, 8, DUMMY, 10, 8, 3, DUMMY, _lib.MOLAGG_ATTENTIVE, C.c_float(1.0), DUMMY, 8, None) == EINVAL


def _head_args(mode=3, d=8, B=4, nV=9):
    h = _lib.HeadArgs()
    h.n_atoms, h.n_mols, h.d_h, h.batch = nV, B, d, DUMMY
    h.agg_mode, h.agg_norm = mode, 1.0
    h.n_layers, h.act = 2, _lib.ACT["tanh"]
    h.dims[0], h.dims[1], h.dims[2] = d, 16, 1
    for l in range(2):
        h.W[l], h.b[l], h.gW[l], h.gb[l] = DUMMY, DUMMY, DUMMY, DUMMY
    h.loss = _lib.LOSS["mse"]
    h.targets = h.preds = h.loss_out = h.gHv = DUMMY
    h.ldg = d
    h.att_W = h.att_b = h.g_att_W = h.g_att_b = DUMMY
    return h


def test_head_attentive_argument_checks_are_codes_before_any_device_work():
    lib = _lib.load()
    h = _head_args()
    sum_bytes = int(lib.dmpnn_head_ws_bytes(C.byref(_head_args(mode=0))))
    att_bytes = int(lib.dmpnn_head_ws_bytes(C.byref(h)))
    assert att_bytes > sum_bytes   # (the workspace grows in attentive mode only)
    for mode in (1, 2):
        assert int(lib.dmpnn_head_ws_bytes(C.byref(_head_args(mode=mode)))) == sum_bytes
    h.ws, h.ws_bytes = DUMMY, att_bytes
    for field in ("att_W", "att_b"):
        g = _head_args()
        g.ws, g.ws_bytes = DUMMY, att_bytes
        setattr(g, field, None)
        assert lib.dmpnn_head(C.byref(g), DUMMY, 8, None) == EINVAL, field
        assert b"att_W" in lib.dmpnn_last_error_string()
    g = _head_args()
    g.ws, g.ws_bytes, g.n_components = DUMMY, 1 << 30, 2
    assert lib.dmpnn_head(C.byref(g), DUMMY, 8, None) == EINVAL
    assert b"component" in lib.dmpnn_last_error_string()
    assert lib.dmpnn_head(C.byref(h), DUMMY, 7, None) == EINVAL          # ldhv < d_h
    g = _head_args()
    g.ws, g.ws_bytes, g.ldg = DUMMY, att_bytes, 7
    assert lib.dmpnn_head(C.byref(g), DUMMY, 8, None) == EINVAL          # ldg < d_h
    g = _head_args()
    g.ws, g.ws_bytes, g.act = DUMMY, att_bytes, _lib.ACT["prelu"]
    assert lib.dmpnn_head(C.byref(g), DUMMY, 8, None) == EINVAL          # (the head's own checks run in front of the attention's launch)
    g = _head_args()
    g.ws, g.ws_bytes = DUMMY, sum_bytes                                    # enough for sum / mean / norm, too small for this mode
    assert lib.dmpnn_head(C.byref(g), DUMMY, 8, None) == ENOSPC
    # (the size it names is this mode's own, never the inner head's — which this workspace would hold)
    assert f"({sum_bytes} < {att_bytes} bytes)" in lib.dmpnn_last_error_string().decode()
    g.ws = None
    assert lib.dmpnn_head(C.byref(g), DUMMY, 8, None) == ENOSPC
    # the order of the rules: a call that is wrong in an argument AND has no workspace reports the argument — in either mode, whether
    # the rule is the attention's own or the head's behind it
    for mode, spoil, names in ((3, dict(act=_lib.ACT["prelu"]), "activation"), (3, dict(ldg=7), "ldg"), (3, dict(att_b=None), "att_W"),
                               (0, dict(act=_lib.ACT["prelu"]), "activation"), (0, dict(preds=None), "preds"), (0, dict(n_layers=0), "predictor layers")):
        g = _head_args(mode=mode)
        for k, v in spoil.items():
            setattr(g, k, v)
        assert g.ws is None and g.ws_bytes == 0
        assert lib.dmpnn_head(C.byref(g), DUMMY, 8, None) == EINVAL, (mode, spoil)
        assert names in lib.dmpnn_last_error_string().decode(), (mode, spoil, lib.dmpnn_last_error_string())
        g = _head_args(mode=mode)   # (the same call, unspoiled: what stops it is the workspace)
        assert lib.dmpnn_head(C.byref(g), DUMMY, 8, None) == ENOSPC and b"workspace" in lib.dmpnn_last_error_string(), mode


def test_abi_mirror_of_the_new_struct_matches_a_c_compiler(tmp_path):
    import os
    import shutil
    import subprocess

    gcc = shutil.which("gcc")
    assert gcc, "gcc is needed for the layout check"
    inc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "dmpnn.h"', "int main(void) {",
             'printf("size %zu\\n", sizeof(dmpnn_molagg_attn_args));']
    for f in _lib.MolAggAttnArgs._fields_:
        lines.append(f'printf("{f[0]} %zu\\n", offsetof(dmpnn_molagg_attn_args, {f[0]}));')
    lines.append('printf("mode %d\\n", (int)DMPNN_MOLAGG_ATTENTIVE); return 0; }')
    (tmp_path / "l.c").write_text("\n".join(lines))
    subprocess.run([gcc, "-I", inc, str(tmp_path / "l.c"), "-o", str(tmp_path / "l")], check=True)
    out = dict(l.split() for l in subprocess.run([str(tmp_path / "l")], capture_output=True, text=True, check=True).stdout.splitlines())
    assert int(out["size"]) == C.sizeof(_lib.MolAggAttnArgs) and int(out["mode"]) == _lib.MOLAGG_ATTENTIVE
    for f in _lib.MolAggAttnArgs._fields_:
        assert int(out[f[0]]) == getattr(_lib.MolAggAttnArgs, f[0]).offset, f[0]
    for n in ("dmpnn_molagg_attn_ws_bytes", "dmpnn_molagg_attn_fwd", "dmpnn_molagg_attn_bwd"):
        assert n in _lib.EXPORTS and hasattr(_lib.load(), n)
    assert _lib.load().dmpnn_version() == 15


@pytest.mark.parametrize("case", ah.agg_cases(), ids=lambda c: c.id)
def test_kernel_case_inputs_meet_their_preconditions(case):
    inp = ah.build(case)   # (asserts max|logit| <= 30)
    assert inp["H"].shape == (sum(case.sizes), case.d) and inp["gout"].shape == (case.n_mols, case.d)
    assert bool((inp["batch"][1:] >= inp["batch"][:-1]).all()) and int(inp["batch"].max()) < case.n_mols
    if case.scale > 1:
        assert inp["max_logit"] > ah.build(ah.AggCase("x1", case.sizes, case.d))["max_logit"]


def test_the_case_list_covers_every_path_of_the_kernels():
    cs = ah.agg_cases()
    widths = {c.d for c in cs if c.sizes == ah.BASE_SIZES and not c.pad and not c.offset and c.scale == 1.0 and not c.extra_mols}
    assert {1, 4, 6, 301, 44, 256, 300, 1024, 2400} <= widths
    assert 0 in ah.BASE_SIZES and 1 in ah.BASE_SIZES and 64 in ah.BASE_SIZES and 65 in ah.BASE_SIZES
    assert max(ah.BEYOND_STAGE) == ah.STAGE_ATOMS + 1
    beyond = [c for c in cs if c.sizes == ah.BEYOND_STAGE]
    assert any(c.vector and c.d > ah.NARROW_VEC for c in beyond) and any(not c.vector and c.d > ah.NARROW_SCALAR for c in beyond)
    assert any(c.offset % 4 for c in cs) and any(c.pad % 4 == 0 and c.pad for c in cs) and any(c.pad % 4 for c in cs)
    assert any(c.extra_mols for c in cs) and any(len(c.sizes) == 1 for c in cs) and any(c.scale == 4.0 for c in cs)


@pytest.mark.parametrize("case", ah.head_cases(), ids=lambda c: c.id)
def test_head_case_inputs_meet_their_preconditions(case):
    inp = ah.head_inputs(case)
    counts = torch.bincount(inp["batch"], minlength=case.B)
    assert int(counts.min()) >= 1 and int(counts.max()) <= 3 and inp["Hv"].shape == (int(counts.sum()), case.d_h)
    ref = ah.head_reference(case, inp)
    for k in ah.head_output_names(case):
        assert bool(torch.isfinite(ref[k]).all()), k
