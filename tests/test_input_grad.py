"""Gradients with respect to the block's inputs (``dmpnn_backward_inputs`` / ``dmpnn_src_sum``, ``engine.backward(inputs=)``,
``autograd.mp_forward``'s routing) — everything that needs no GPU: the struct layout, the exports, the argument checks (on made-up
addresses: every refusal comes before any device work) and the routing decision as a pure function."""
import ctypes as C
import os
import shutil
import subprocess

import pytest
import torch

from chemprop_amd import _lib

EINVAL, ENOSPC = -1, -3
FAKE = 0x7000_0000_0000   # (a made-up device address, 16-byte aligned: nothing may ever read it)


def test_struct_matches_the_c_layout(tmp_path):
    """``dmpnn_bwd_inputs_args`` at the offsets the C compiler gives it; ``dmpnn_bwd_args`` is its unchanged first member."""
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang") or "/opt/rocm/llvm/bin/clang"
    fields = [n for n, _ in _lib.BwdInputsArgs._fields_]
    assert fields == ["b", "gV", "ldgv", "gE", "ldge", "gV_d", "ldgvd"]
    fmt = " ".join(["%zu"] * (len(fields) + 2))
    offs = ",".join(f"offsetof(dmpnn_bwd_inputs_args, {n})" for n in fields)
    src = tmp_path / "off.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "dmpnn.h"\nint main(void){printf("' + fmt + '\\n",' + offs +
                   ',sizeof(dmpnn_bwd_inputs_args), sizeof(dmpnn_bwd_args));return 0;}\n')
    exe = tmp_path / "off"
    inc = os.path.join(os.path.dirname(_lib.__file__), "..", "include")
    subprocess.run([cc, "-I", inc, str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    want = [getattr(_lib.BwdInputsArgs, n).offset for n in fields] + [C.sizeof(_lib.BwdInputsArgs), C.sizeof(_lib.BwdArgs)]
    assert got == want
    assert _lib.BwdInputsArgs.b.offset == 0


def test_entries_are_exported_and_the_version_stays():
    lib = _lib.load()
    for name in ("dmpnn_backward_inputs", "dmpnn_src_sum", "dmpnn_backward_inputs_ws_bytes"):
        assert name in _lib.EXPORTS
        assert getattr(lib, name) is not None
    assert "dmpnn_inputgrad.hip" in _lib.SOURCES
    assert _lib.ABI_VERSION == 15 and int(lib.dmpnn_version()) == 15


def _args(**over):
    """A well-formed block on made-up addresses (per-step general route, relu, depth 2, no W_d); ``over``: fields to change, a
    dotted name for the nested blocks (``b.f.flags``)."""
    a = _lib.BwdInputsArgs()
    f = a.b.f
    f.plan, f.n_atoms, f.n_edges = FAKE, 10, 20
    f.d_v, f.d_e, f.d_h, f.d_vd, f.depth, f.flags, f.act = 8, 4, 16, 0, 2, _lib.F_KEEP, _lib.ACT["relu"]
    f.V, f.ldv, f.E, f.lde = FAKE, 8, FAKE, 4
    f.W_i = f.W_h = f.W_o = f.b_o = FAKE
    f.ldh, f.H0, f.Hs, f.n_hslots, f.Ms, f.n_mslots, f.Mv = 16, FAKE, FAKE, 1, FAKE, 1, FAKE
    f.out, f.ldout = FAKE, 16
    a.b.gout, a.b.ldgout = FAKE, 16
    a.gV, a.ldgv, a.gE, a.ldge = FAKE, 8, FAKE, 4
    for k, v in over.items():
        if k in ("ws", "ws_bytes"):
            continue
        obj, parts = a, k.split(".")
        for p in parts[:-1]:
            obj = getattr(obj, p)
        setattr(obj, parts[-1], v)
    a.b.ws = FAKE
    a.b.ws_bytes = over.get("ws_bytes", int(_lib.load().dmpnn_backward_inputs_ws_bytes(C.byref(a.b.f))))
    return a


def _call(a):
    lib = _lib.load()
    n0 = int(lib.dmpnn_last_launch_count())
    rc = int(lib.dmpnn_backward_inputs(C.byref(a) if a is not None else None, None))
    return rc, lib.dmpnn_last_error_string().decode(errors="replace"), int(lib.dmpnn_last_launch_count()) - n0


@pytest.mark.parametrize("name,over,word", [
    ("mega", {"b.f.flags": _lib.F_KEEP | _lib.F_FUSED | _lib.F_MEGA | _lib.F_SPLIT16}, "general route"),
    ("tile plan", {"b.f.flags": _lib.F_KEEP | _lib.F_TILE_PLAN}, "general route"),
    ("fused", {"b.f.flags": _lib.F_KEEP | _lib.F_FUSED}, "general route"),
    ("atom", {"b.f.flags": _lib.F_KEEP | _lib.F_ATOM}, "general route"),
    ("prelu", {"b.f.act": _lib.ACT["prelu"]}, "PReLU"),
    ("gV_d without W_d", {"gV_d": FAKE, "ldgvd": 5}, "W_d"),
    ("ldgv", {"ldgv": 7}, "leading dimension"),
    ("ldge", {"ldge": 3}, "leading dimension"),
    ("ldgvd", {"b.f.W_d": FAKE, "b.f.b_d": FAKE, "b.f.V_d": FAKE, "b.f.ldvd": 5, "b.f.d_vd": 5, "b.f.Hv": FAKE, "b.f.ldout": 21, "b.ldgout": 21,
               "gV_d": FAKE, "ldgvd": 4}, "leading dimension"),
])
def test_refusals_come_before_any_device_work(name, over, word):
    rc, msg, launches = _call(_args(**over))
    assert rc == EINVAL and word in msg and launches == 0, (name, rc, msg, launches)


def test_null_struct_and_short_workspace():
    rc, msg, launches = _call(None)
    assert rc == EINVAL and "null" in msg and launches == 0
    good = _args()
    rc, msg, launches = _call(_args(ws_bytes=good.b.ws_bytes - 1))
    assert rc == ENOSPC and "workspace too small" in msg and launches == 0
    lib = _lib.load()
    # the existing entry's answer is unchanged by the new one, which asks for more (the transposed weight slices)
    assert int(lib.dmpnn_backward_inputs_ws_bytes(C.byref(good.b.f))) > int(lib.dmpnn_backward_ws_bytes(C.byref(good.b.f))) > 0


def test_no_atoms_is_ok_and_does_nothing():
    """``n_atoms == 0``: ``DMPNN_OK`` with no parameter gradient asked for, nothing launched (the made-up addresses are never used)."""
    rc, msg, launches = _call(_args(**{"b.f.n_atoms": 0, "b.f.n_edges": 0}))
    assert rc == 0 and launches == 0, (rc, msg, launches)


def test_src_sum_refuses_bad_arguments():
    lib = _lib.load()
    for args in ((None, 4, 6, 8, FAKE, 8, FAKE, 8), (FAKE, 4, 6, 0, FAKE, 8, FAKE, 8), (FAKE, 4, 6, 8, FAKE, 7, FAKE, 8),
                 (FAKE, 4, 6, 8, FAKE, 8, FAKE, 7), (FAKE, 4, 6, 8, None, 8, FAKE, 8), (FAKE, 4, 6, 8, FAKE, 8, None, 8), (FAKE, -1, 6, 8, FAKE, 8, FAKE, 8)):
        n0 = int(lib.dmpnn_last_launch_count())
        assert int(lib.dmpnn_src_sum(*args, None)) == EINVAL, args
        assert int(lib.dmpnn_last_launch_count()) == n0


def test_routing_decision_is_a_full_plan_at_level_zero():
    """An input that requires grad: a full plan (no light plan, no tile plan) and the route cap 0 — whatever the caller had; nothing
    upstream requires grad: exactly what the caller had."""
    from chemprop_amd.autograd import input_grad_plan, input_grad_wanted

    for light in (False, True, "tiles"):
        for level in (0, 1, 2):
            assert input_grad_plan(True, light, level) == (False, 0)
            assert input_grad_plan(False, light, level) == (light, level)
    x, g = torch.zeros(2, 3), torch.zeros(2, 3, requires_grad=True)
    assert not input_grad_wanted(x, x, None)
    assert input_grad_wanted(g, x, None) and input_grad_wanted(x, g, None) and input_grad_wanted(x, x, g)
    with torch.no_grad():
        assert not input_grad_wanted(g, g, g)


def test_engine_backward_refuses_unknown_input_names_and_keeps_its_default():
    """A name outside ``{"V", "E", "V_d"}`` is a ``ValueError`` before anything is allocated or enqueued (the state is never looked
    at: ``None`` stands in for it); ``inputs`` defaults to ``None`` and ``linear_fn``'s ``plan`` to ``None``."""
    import inspect

    from chemprop_amd import backward, engine

    with pytest.raises(ValueError, match="drawn from"):
        engine.backward(None, None, {}, inputs={"X"})
    with pytest.raises(ValueError, match="drawn from"):
        engine.backward(None, None, {}, inputs={"V", "H"})
    sig = inspect.signature(engine.backward)
    assert sig.parameters["inputs"].default is None
    assert "plan" in inspect.signature(backward.linear_fn).parameters and inspect.signature(backward.linear_fn).parameters["plan"].default is None
    assert callable(engine.src_sum)


def test_linear_fn_refuses_a_plan_beside_another_gather():
    """``plan=`` says "the gather is ``plan.src32``": any other gather beside it is refused before the kernel runs."""
    from chemprop_amd import backward

    class _Plan:
        src32 = torch.zeros(4, dtype=torch.int32)

    x, w = torch.zeros(3, 2), torch.zeros(5, 2)
    with pytest.raises(ValueError, match="plan.src32"):
        backward.linear_fn(x, w, None, gather=torch.zeros(4, dtype=torch.int32), n_rows=4, plan=_Plan())
    with pytest.raises(ValueError, match="plan.src32"):
        backward.linear_fn(x, w, None, plan=_Plan())


def test_the_restated_kernel_constants_are_the_kernels_own():
    """``tests/test_input_grad_gpu.py`` places its shapes by the constants of ``k_input_grad_v`` and of the row kernels' tile,
    restated in ``tests/input_grad_shapes.py``: they are read back from the sources here, so that a kernel whose tile moves fails this test
    instead of quietly leaving the seams."""
    import re

    import input_grad_shapes as sh

    csrc = os.path.join(os.path.dirname(_lib.__file__), "csrc")
    src = open(os.path.join(csrc, "dmpnn_inputgrad.hip")).read()
    const = lambda name, text=src: int(re.search(r"constexpr int " + name + r" = (\d+);", text).group(1))
    assert (const("kIgTA"), const("kIgKC"), const("kIgCT")) == (sh.FUSED_TILE, sh.FUSED_KCHUNK, sh.FUSED_MAX_DV // 64)
    assert "constexpr int kIgMaxDv = 4 * kIgCT * 16;" in src
    rows = open(os.path.join(csrc, "dmpnn_rows16_impl.hpp")).read()
    assert "constexpr int RT = 3, BM = 16 * RT;" in rows and sh.ROW_TILE == 16 * 3
