"""An atom block on the per-step general route of the C ABI: ``engine.forward(route="general", atom=True, keep=True)`` (``DMPNN_F_ATOM``
without ``DMPNN_F_FUSED``, fp32 and ``DMPNN_F_SPLIT16``) and ``engine.backward`` on what it kept.

One batch shape: a single-atom molecule, six QM9-shaped ones and one 40-atom molecule (beyond the tile), at the case's ``d_v`` /
``d_e``.  The grid crosses ``d_h`` in {64, 300, 324} (324: above the tile kernels' width), depth in {1, 2, 3} and both arithmetics;
biases, the activation (relu | tanh) and ``d_e`` in {2, 14, 16} are dealt over it as a Latin square; ``d_e = 13`` with ``d_v = 71``
puts every contraction on the fp32 kernel under either arithmetic; three cases run with ``dropout = (0.2, seed)``.

The bar (``tests/atom_harness.py``, the project's: ``tests/head_harness.py``): ``out`` and every wanted gradient against the float64
restatement on the CPU, ``err = max|got - ref| / max|ref|`` within ``min(MARGIN max(e32, 2**-23), cap)`` — ``e32`` the same
restatement in float32, caps 1e-5 (``out``) and 2e-5 (gradients).  ``gW_h`` is compared as a whole AND per column block (the hidden
block ``[:, :d_h]``, the bond-feature block ``[:, d_h:]``), so a zero block cannot hide in the norm.  ReLU cases are compared under
fixed decisions: the reference gets the 0 / 1 factors the device run kept (the sign of the kept ``H0`` / ``H^(t)`` / ``out``; under a
dropped entry the reference's own), and those may differ from the free float64 run's in at most 1e-3 of the elements.  With dropout
the reference is given the masks of ``oracle.dropout_hash.keep_mask`` at sites ``t - 1`` / ``depth - 1``.

MARGIN: the worst ``err / max(e32, 2**-23)`` over this module's cases on the MI355X is 2.32 (``h324-d3-de14-relu-bias-f32``; 2.31
``h300-d3-de14-relu-bias-p0.2``, 2.25 ``h300-d2-de16-relu-bias-f32`` follow — neither arithmetic stands out); doubled and rounded up
to a power of two: 8.  No ReLU decision of any case differed from the free float64 run's.
"""
import ctypes as C
import dataclasses
import functools
import itertools

import pytest
import torch

import atom_harness as ah
import rows_harness as rh
from chemprop_amd import _lib

MARGIN = 8.0
gpu = pytest.mark.gpu
SEED = 0x0123_4567_89AB_CDEF
FLIP_SHARE = 1e-3


@dataclasses.dataclass(frozen=True)
class B:
    id: str
    d_h: int
    depth: int
    bias: bool
    act: str
    d_e: int = 14
    d_v: int = 72
    mfma: str = "split16"
    p: float = 0.0
    skip: tuple = ()          # gradients that are not wanted (NULL)
    seed: int = 0


def _cases():
    cs = []
    for j, (a, b) in enumerate(itertools.product(range(3), range(3))):
        d_h, depth, d_e = (64, 300, 324)[a], (1, 2, 3)[b], (2, 14, 16)[(a + b) % 3]
        act = ("relu", "tanh")[j % 2]
        for k, mfma in enumerate(("split16", "f32")):
            bias = bool((j + k) % 2)
            cs.append(B(f"h{d_h}-d{depth}-de{d_e}-{act}-{'bias' if bias else 'nobias'}-{mfma}", d_h, depth, bias, act, d_e, mfma=mfma, seed=j))
    cs += [B("h64-d3-de13-dv71-tanh-bias-f32", 64, 3, True, "tanh", 13, 71, "f32", seed=11),
           B("h64-d3-de13-dv71-relu-nobias-split16", 64, 3, False, "relu", 13, 71, seed=12),
           B("h300-d3-de14-relu-bias-null-gW_i-gb_h", 300, 3, True, "relu", skip=("W_i", "b_h"), seed=13),
           B("h300-d3-de14-relu-bias-p0.2", 300, 3, True, "relu", p=0.2, seed=14),
           B("h324-d2-de16-tanh-nobias-p0.2", 324, 2, False, "tanh", 16, p=0.2, seed=15),
           B("h64-d1-de2-tanh-bias-p0.2", 64, 1, True, "tanh", 2, p=0.2, seed=16)]
    assert len({c.id for c in cs}) == len(cs)
    return cs


CASES = _cases()


@functools.lru_cache(maxsize=None)
def _inputs(c: B):
    """Batch (CPU), parameters, the gradient input, the dropout keep masks and the FREE float64 run — computed once, never written to."""
    from oracle import dropout_hash as dh

    bmg = ah.mixed_batch(c.d_v, c.d_e, seed=c.seed)
    w = ah.block_weights(c.d_v, c.d_e, c.d_h, c.bias, seed=c.seed)
    nV, nE = int(bmg.V.shape[0]), int(bmg.E.shape[0])
    G = torch.randn(nV, c.d_h, generator=torch.Generator().manual_seed(5 + c.seed))
    keeps = None
    if c.p > 0:
        keeps = [torch.from_numpy(dh.keep_mask(SEED, t, nE, c.d_h, c.p)) for t in range(c.depth - 1)]
        keeps.append(torch.from_numpy(dh.keep_mask(SEED, c.depth - 1, nV, c.d_h, c.p)))
    _, _, pre, made = ah.block_ref(bmg, w, c.depth, c.act, keeps=keeps, p=c.p)
    return bmg, w, G, keeps, pre, made


def _references(c: B, decisions):
    """float64 and float32 restatements under the same decisions and masks -> (named float64 tensors, e32)."""
    bmg, w, G, keeps, _, _ = _inputs(c)
    res = []
    for dtype in (torch.float64, torch.float32):
        out, L, _, _ = ah.block_ref(bmg, w, c.depth, c.act, dtype, decisions=decisions, keeps=keeps, p=c.p)
        res.append(ah.named(out, ah.block_grads(out, L, G), c.d_h))
    return res[0], ah.yardstick(res[0], res[1])


def _share(a, b):
    return sum(int((x != y).sum()) for x, y in zip(a, b)) / max(1, sum(x.numel() for x in a))


def test_atom_block_references_on_cpu():
    """Every case: the restatement is ``oracle.dmpnn_torch.atom_forward`` (float64, no dropout); the batch mixes a single-atom molecule
    with a 40-atom one; float32 itself meets the caps under the float64 run's decisions; the float32 run's own ReLU decisions stay
    within the share the GPU tests allow; no reference tensor but depth 1's ``gW_h`` / ``gb_h`` is identically zero."""
    from oracle import dmpnn_torch as ot

    assert {c.d_h for c in CASES} == {64, 300, 324} and {c.depth for c in CASES} == {1, 2, 3} and {c.d_e for c in CASES} == {2, 13, 14, 16}
    for c in CASES:
        bmg, w, G, keeps, pre, made = _inputs(c)
        sizes = torch.bincount(bmg.batch)
        assert int(sizes.min()) == 1 and int(sizes.max()) == 40 and len(sizes) == 8 and int(bmg.E.shape[1]) == c.d_e
        if c.p == 0:
            mw = ot.MPWeights(*(None if w[k] is None else w[k].double() for k in ("W_i", "W_h", "W_o", "b_o", "b_i", "b_h")))
            o = ot.atom_forward(bmg.V.double(), bmg.E.double(), bmg.edge_index, bmg.rev_edge_index, mw, depth=c.depth, activation=c.act)
            mine = ah.block_ref(bmg, w, c.depth, c.act)[0]
            assert torch.allclose(mine, o, rtol=1e-12, atol=1e-14), c.id
        ref, e32 = _references(c, made if c.act == "relu" else None)
        for k, e in e32.items():
            assert e < rh.CAP["fwd" if k == "out" else "grad"], (c.id, k, e)
            if c.depth > 1 or not k.startswith(("gW_h", "gb_h")):
                assert float(ref[k].abs().max()) > 0, (c.id, k)
            else:
                assert not bool(ref[k].any()), (c.id, k)
        if c.act == "relu":
            made32 = ah.block_ref(bmg, w, c.depth, c.act, torch.float32, keeps=keeps, p=c.p)[3]
            assert _share(made32, made) <= FLIP_SHARE, (c.id, _share(made32, made))


def _forward(c: B, dev, **kw):
    from chemprop_amd import engine

    cpu, w, G, keeps, _, _ = _inputs(c)
    bmg = ah.on_device(cpu, dev)
    plan = engine.GraphPlan.from_bmg(bmg)
    d = {k: (None if v is None else v.to(dev)) for k, v in w.items()}
    args = dict(depth=c.depth, act=c.act, keep=True, route="general", mfma=c.mfma, atom=True, dropout=(c.p, SEED) if c.p > 0 else None)
    args.update(kw)
    out, st = engine.forward(plan, bmg.V, bmg.E, d["W_i"], d["W_h"], d["W_o"], d["b_o"], d["b_i"], d["b_h"], **args)
    return out, st, bmg, d


@gpu
@pytest.mark.parametrize("c", CASES, ids=lambda c: c.id)
def test_atom_block_on_the_general_route(c, gpu_device):
    from chemprop_amd import engine

    dev = gpu_device
    cpu, w, G, keeps, pre, made = _inputs(c)
    out, st, bmg, _ = _forward(c, dev)
    assert st.route == ("general16" if c.mfma == "split16" else "general"), st.route
    assert st.args.flags & _lib.F_ATOM and not st.args.flags & _lib.F_FUSED
    assert int(st.args.msplit_bytes) == cpu.E.shape[0] * 64 and abs(float(st.args.dropout_p) - c.p) < 1e-7
    need = {k: k not in c.skip for k in ah.PARAMS}
    grads = engine.backward(st, G.to(dev), need)
    torch.cuda.synchronize()
    for k in ah.PARAMS:
        if k in c.skip or w[k] is None:
            assert grads[k] is None, f"{k}: not wanted (or not there), so not among the outputs"
    got = dict(out=out.cpu())
    for k in ah.PARAMS:
        if grads[k] is not None:
            got["g" + k] = grads[k].cpu()
    assert tuple(got["gW_h"].shape) == (c.d_h, c.d_h + c.d_e) and ("gW_i" in c.skip or "W_i" in c.skip or tuple(got["gW_i"].shape) == (c.d_h, c.d_v))
    got["gW_h[:, :d_h]"], got["gW_h[:, d_h:]"] = got["gW_h"][:, :c.d_h], got["gW_h"][:, c.d_h:]
    # the kept bond-feature half of the messages: zero-padded [n_edges][16] rows in the caller's edge order
    ME = st.refs[15][0].cpu()
    me64 = ah.atom_message_ref(cpu, cpu.E)
    assert torch.equal(ME[:, :c.d_e].double(), me64) and not bool(ME[:, c.d_e:].any()), "ME: small integers, exact; zero padding"
    decisions = None
    if c.act == "relu":
        H0 = st.H0[:, :c.d_h].cpu()
        Hs = [st.Hs[t][:, :c.d_h].cpu() for t in range(c.depth - 1)]
        o = got["out"]
        if keeps is None:
            decisions = [H0 > 0] + [h > 0 for h in Hs] + [o > 0]
        else:   # (under a dropped entry the kept value says nothing: the reference's own decision, times 0)
            decisions = [H0 > 0] + [torch.where(keeps[t], Hs[t] > 0, pre[t + 1] > 0) for t in range(c.depth - 1)] + [torch.where(keeps[-1], o > 0, pre[c.depth] > 0)]
        share = _share(decisions, made)
        print(f"ATOMBAR {c.id} relu decisions that differ from the free float64 run: {share:.3e} of the elements")
        assert share <= FLIP_SHARE, share
    if keeps is not None:
        assert bool((got["out"][~keeps[-1]] == 0).all())
        for t in range(c.depth - 1):
            assert bool((st.Hs[t][:, :c.d_h].cpu()[~keeps[t]] == 0).all()), f"update site {t}"
    ref, e32 = _references(c, decisions)
    fails, worst = ah.compare(c.id, got, {k: ref[k] for k in got}, e32, MARGIN)
    print(f"ATOMBAR {c.id} worst-ratio={worst:.2f}")
    assert not fails, f"{c.id}: " + "; ".join(fails)


@gpu
def test_atom_block_inference_on_the_general_route(gpu_device):
    """Without ``keep`` the same ``msplit`` buffer is scratch: the output is the training forward's, bit for bit."""
    for c in (CASES[4], CASES[5]):   # (depth 3, both arithmetics)
        assert c.depth == 3
        a, st_a, _, _ = _forward(c, gpu_device)
        b, st_b, _, _ = _forward(c, gpu_device, keep=False)
        assert st_b.route == st_a.route and st_b.args.msplit and not st_b.args.flags & _lib.F_KEEP
        assert torch.equal(a, b)


@gpu
def test_atom_general_route_refusals(gpu_device):
    """What the route does not take is refused loudly: ``RouteUnavailable`` from the host, ``DMPNN_EINVAL`` with a message from the
    library — ``d_e = 17``, ``W_d``, undirected, ``msplit`` short by one row, a fused route, and the default rule on a batch beyond
    the tile."""
    from chemprop_amd import engine

    dev = gpu_device
    lib = _lib.load()
    c = CASES[4]
    cpu, w, _, _, _, _ = _inputs(c)
    bmg = ah.on_device(cpu, dev)
    plan = engine.GraphPlan.from_bmg(bmg)
    d = {k: (None if v is None else v.to(dev)) for k, v in w.items()}
    fwd = lambda **kw: engine.forward(plan, bmg.V, kw.pop("E", bmg.E), d["W_i"], kw.pop("W_h", d["W_h"]), d["W_o"], d["b_o"], d["b_i"], d["b_h"],
                                      depth=c.depth, act=c.act, keep=True, atom=True, **kw)
    gen = torch.Generator().manual_seed(1)
    E17 = torch.randn(plan.n_edges, 17, generator=gen).to(dev)
    with pytest.raises(engine.RouteUnavailable):
        fwd(route="general", E=E17, W_h=torch.randn(c.d_h, c.d_h + 17, generator=gen).to(dev))
    with pytest.raises(engine.RouteUnavailable):
        fwd(route="general", undirected=True)
    with pytest.raises(engine.RouteUnavailable):
        D = c.d_h + 3
        fwd(route="general", W_d=torch.randn(D, D, generator=gen).to(dev), b_d=torch.randn(D, generator=gen).to(dev),
            V_d=torch.randn(plan.n_atoms, 3, generator=gen).to(dev))
    with pytest.raises(engine.RouteUnavailable):   # (the default rule, capped as for a batch with a molecule beyond the tile)
        fwd(max_level=1)
    with pytest.raises(engine.RouteUnavailable):
        fwd(route="fused16")

    def call(st):
        with engine._OnDevice(dev):
            rc = int(lib.dmpnn_forward(C.byref(st.args), engine._stream_ptr(dev)))
        torch.cuda.synchronize()
        return rc, lib.dmpnn_last_error_string().decode(errors="replace")

    for mfma in ("split16", "f32"):
        out, st = fwd(route="general", mfma=mfma, launch=False)
        out.fill_(float("nan"))
        st.args.msplit_bytes -= 64
        rc, msg = call(st)
        assert rc == rh.EINVAL and "msplit" in msg, (rc, msg)
        st.args.msplit_bytes += 64
        st.args.msplit = None
        rc, msg = call(st)
        assert rc == rh.EINVAL and "msplit" in msg, (rc, msg)
        st.args.msplit = st.refs[15].data_ptr()
        for extra in (_lib.F_FUSED | _lib.F_SPLIT16, _lib.F_UNDIRECTED):
            flags = st.args.flags
            st.args.flags = flags | extra
            rc, msg = call(st)
            assert rc == rh.EINVAL and "DMPNN_F_ATOM" in msg, (extra, rc, msg)
            st.args.flags = flags
        assert bool(torch.isnan(out).all()), "a refused call writes nothing"
        rc, msg = call(st)
        assert rc == 0, msg
        assert bool(torch.isfinite(out).all())
    # d_e = 17 and W_d at the library itself
    out, st = fwd(route="general", launch=False)
    st.args.d_e = 17
    rc, msg = call(st)
    assert rc == rh.EINVAL and msg, (rc, msg)
