"""Block dropout on the lean per-step route (``k_step16`` / ``k_bstep16``; include/dmpnn.h, ``dmpnn_fwd_args.dropout_p``): the host
side that needs no GPU — the size rule, the route rules (unchanged: they never pick the lean form for p > 0) and the argument checks
of ``dmpnn_forward``, which run before anything reaches the device."""
import ctypes as C

from chemprop_amd import _lib, engine

EINVAL = -1
LEAN = _lib.F_FUSED | _lib.F_SPLIT16 | _lib.F_KEEP


def _args(flags=LEAN, act="relu", p=0.0, depth=3, d_h=300, d_v=72, d_e=14, nV=20500, nE=43800, wd=None):
    a = _lib.FwdArgs()
    a.n_atoms, a.n_edges, a.d_v, a.d_e, a.d_h, a.depth, a.flags = nV, nE, d_v, d_e, d_h, depth, flags
    a.ldv, a.lde, a.ldh, a.ldout = d_v, d_e, (d_h + 3) // 4 * 4, d_h
    a.act, a.dropout_p, a.W_d = _lib.ACT[act], p, wd
    return a


def test_keep_bits_bytes_of_the_lean_form_does_not_depend_on_dropout():
    lib = _lib.load()
    size = lambda a: int(lib.dmpnn_forward_keep_bits_bytes(C.byref(a)))
    n0 = size(_args())
    assert n0 == 3 * 43800 * (320 // 8)                     # depth sites x rows x block_cols(300) / 8 bytes
    assert size(_args(p=0.2)) == n0 > 0
    assert size(_args(p=0.2, act="leakyrelu")) == n0
    # the lean form's own conditions still hold under dropout (and "none" is no ReLU-class activation for the mask's purposes)
    for a in (_args(p=0.2, act="tanh"), _args(p=0.2, act="elu"), _args(p=0.2, wd=4096), _args(p=0.2, depth=1), _args(p=0.2, d_h=512),
              _args(p=0.2, depth=9), _args(p=0.2, d_v=73), _args(p=0.2, d_e=13), _args(p=0.2, d_h=302), _args(p=0.2, act="none"),
              _args(p=1.0), _args(p=1.5), _args(p=-0.1)):
        assert size(a) == 0
    assert size(_args(act="none")) == n0                    # (without dropout the identity keeps its lean form)


def test_the_route_rules_never_pick_the_lean_form_for_dropout():
    """``lean`` implies p == 0 (tests/test_host.py pins the rule's table): the lean route with dropout is taken on demand only."""
    lib = _lib.load()
    for (nV, nE, n_mols) in ((166000, 355702, 4096), (20500, 43800, 512)):
        for p in (0.0, 0.2):
            a = _args(flags=0, p=p, nV=nV, nE=nE)
            info = _lib.TrainRouteInfo()
            assert lib.dmpnn_train_route(C.byref(a), n_mols, 0, -1, 2, 0, -1, C.byref(info)) == 0
            assert _lib.ROUTES[info.route] == ("general16" if p else "fused16"), (nE, p, _lib.ROUTES[info.route])
            assert info.lean == (0 if p else 1) and info.keep_bits == (0 if p else 1)
            assert _lib.ROUTES[lib.dmpnn_forward_route(C.byref(a), 1, 2, 0, 0)] == ("general16" if p else "fused16")
    assert engine.train_route(166000, 355702, 72, 14, 300, 3, "relu", 4096, dropout_p=0.2).lean == 0


def test_forward_refuses_dropout_outside_its_two_homes_before_any_device_work():
    """``dmpnn_forward`` validates ``dropout_p`` on the host (no GPU here; every pointer below is a placeholder nothing dereferences)."""
    lib = _lib.load()

    def call(a):
        for f in ("plan", "V", "E", "W_i", "W_h", "W_o", "b_o", "H0", "Hs", "Ms", "Mv", "out", "msplit", "wsplit"):
            setattr(a, f, 4096)
        a.n_mslots = a.n_hslots = 2
        rc = int(lib.dmpnn_forward(C.byref(a), None))
        return rc, lib.dmpnn_last_error_string().decode(errors="replace")

    a = _args(p=1.5)
    a.keep_bits, a.keep_bits_bytes = 4096, 1 << 40
    rc, msg = call(a)
    assert rc == EINVAL and "dropout_p" in msg, (rc, msg)
    # the lean flags without keep_bits: the fp32-keeping fused16 forward has no dropout
    rc, msg = call(_args(p=0.2))
    assert rc == EINVAL and "dropout" in msg, (rc, msg)
    # ... and with keep_bits where the lean form's own conditions fail
    for kw in (dict(act="tanh"), dict(d_h=512), dict(depth=1), dict(d_v=73)):
        a = _args(p=0.2, **kw)
        a.keep_bits, a.keep_bits_bytes = 4096, 1 << 40
        rc, msg = call(a)
        assert rc == EINVAL and "dropout" in msg, (kw, rc, msg)
    # the per-step general route, the per-step fused route on fp32, inference on the step kernels
    for flags in (_lib.F_KEEP, _lib.F_FUSED | _lib.F_KEEP, _lib.F_FUSED | _lib.F_SPLIT16):
        rc, msg = call(_args(flags=flags, p=0.2))
        assert rc == EINVAL and "dropout" in msg, (flags, rc, msg)


def test_lean_dropout_refusal_names_the_failed_condition():
    r = engine.lean_dropout_refusal
    assert r(72, 14, 300, 3, "relu") is None and r(106, 28, 100, 2, "leakyrelu") is None
    assert "depth 1" in r(72, 14, 300, 1, "relu")
    assert "320" in r(72, 14, 400, 3, "relu")
    assert "odd" in r(73, 14, 300, 3, "relu") and "odd" in r(72, 13, 300, 3, "relu")
    assert "> 8" in r(72, 14, 300, 9, "relu")
    assert "tanh" in r(72, 14, 300, 3, "tanh")
    assert "W_d" in r(72, 14, 300, 3, "relu", True)
    # ... and agrees with the library's size rule on every case above
    lib = _lib.load()
    for (dv, de, dh, depth, act) in ((72, 14, 300, 3, "relu"), (72, 14, 300, 1, "relu"), (72, 14, 400, 3, "relu"), (73, 14, 300, 3, "relu"),
                                     (72, 14, 300, 9, "relu"), (72, 14, 300, 3, "tanh"), (72, 14, 302, 3, "relu"), (250, 14, 300, 3, "relu")):
        n = int(lib.dmpnn_forward_keep_bits_bytes(C.byref(_args(p=0.2, act=act, depth=depth, d_h=dh, d_v=dv, d_e=de))))
        assert (n > 0) == (r(dv, de, dh, depth, act) is None), (dv, de, dh, depth, act)
