"""The staged ``FusedTrainer.step`` and the shared builder of a head call (``HeadSpec.call_args``): the module path's head node against
the hand-built call of ``head_harness.run_head`` bit for bit, and the order of a step's stages — every refusal before anything is
counted or drawn, the block's dropout seed before the head's, Adam's step count after the call."""
import copy

import pytest
import torch

import head_harness as hh

# (a): the column kernels' layout (norm, batch norm); (b): descriptors without batch norm — the aggregate lands in the fingerprint's rows
HEAD_CASES = {
    "a": dict(atoms=(1, 4, 2, 3, 1), d_h=8, d_xd=0, hidden=8, tasks=2, agg="norm", bn=True, bounded=False),
    "b": dict(atoms=(2, 1, 3), d_h=12, d_xd=3, hidden=8, tasks=1, agg="mean", bn=False, bounded=True),
}


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(HEAD_CASES))
def test_module_path_head_node_equals_a_hand_built_head_call_bit_for_bit(name, gpu_device):
    """``head_loss(...).backward()`` (``_HeadLoss`` on ``HeadSpec.call_args``) and ``head_harness.run_head`` (``HeadSpec.fill`` and the
    rest by hand) on deep copies of one model and the same inputs: the loss, ``gH_v`` and every head parameter's gradient are equal
    bit for bit — after two runs of ``run_head`` alone have shown the head deterministic on the case."""
    from chemprop_amd.model import HeadSpec, head_loss

    c = HEAD_CASES[name]
    n_mols, dev = len(c["atoms"]), gpu_device
    torch.manual_seed(11)
    model = hh.make_model(c["d_h"], c["d_xd"], c["hidden"], c["tasks"], bn=c["bn"], agg=c["agg"], kind="mse").to(dev).train()
    gen = torch.Generator().manual_seed(12)
    batch = torch.repeat_interleave(torch.arange(n_mols), torch.tensor(c["atoms"])).to(dev)
    Hv0 = torch.randn(int(batch.numel()), c["d_h"], generator=gen).to(dev)
    T = torch.randn(n_mols, c["tasks"], generator=gen).to(dev)
    X = hh.descriptors(n_mols, c["d_xd"], 13).to(dev) if c["d_xd"] else None
    w = lt = gt = None
    if c["bounded"]:
        w = (0.5 + torch.rand(n_mols, generator=gen)).to(dev)
        lt = (torch.rand(n_mols, c["tasks"], generator=gen) < 0.5).to(dev)
        gt = (torch.rand(n_mols, c["tasks"], generator=gen) < 0.5).to(dev)

    def by_hand():
        m = copy.deepcopy(model)
        loss, _, grads, gH = hh.run_head(m, Hv0, batch, n_mols, T, w, lt, gt, X)
        return loss, [grads[id(p)] for p in HeadSpec(m).params()], gH

    ref, again = by_hand(), by_hand()
    assert ref[0] == again[0] and torch.equal(ref[2], again[2]) and all(torch.equal(a, b) for a, b in zip(ref[1], again[1])), \
        "run_head alone is not deterministic on this case"
    m = copy.deepcopy(model)
    Hv = Hv0.clone().requires_grad_()
    loss = head_loss(m, Hv, batch, n_mols, T, w, lt, gt, X_d=X)
    assert loss is not None, "the head kernels must take this model"
    loss.backward()
    torch.cuda.synchronize()
    print(f"case {name}: loss {float(loss.detach()):.9g} (by hand {ref[0]:.9g}), max |gH_v - by hand| {float((Hv.grad.cpu() - ref[2]).abs().max()):.3g}")
    assert float(loss.detach()) == ref[0]
    assert torch.equal(Hv.grad.cpu(), ref[2])
    params = HeadSpec(m).params()
    assert len(params) == len(ref[1]) == (2 if c["bn"] else 0) + 4
    for p, g in zip(params, ref[1]):
        assert torch.equal(p.grad.cpu(), g), tuple(p.shape)


@pytest.mark.gpu
def test_a_refused_step_leaves_no_trace_and_a_taken_step_draws_its_seeds_in_order(gpu_device):
    """Every refusal of ``FusedTrainer.step`` is raised before a seed is drawn, a batch is counted or Adam's step count moves: the
    CPU generator, ``opt.steps``, the batch norm's buffers and every parameter are unchanged.  The step that is then taken draws
    the block's dropout seed first, the head's second, and advances ``opt.steps`` to 1."""
    from chemprop_amd import agg as cagg, synth
    from chemprop_amd.model import MPNN, FusedTrainer, RegressionFFN
    from chemprop_amd.nn import BondMessagePassing

    dev = gpu_device
    torch.manual_seed(3)
    model = MPNN(BondMessagePassing(d_h=32, dropout=0.1), cagg.MeanAggregation(), RegressionFFN(n_tasks=2, input_dim=32, hidden_dim=16, dropout=0.1),
                 batch_norm=True).to(dev).train()
    tr = FusedTrainer(model, lr=1e-3, ffn_dropout=True)
    bmg = synth.random_batch(8, "qm9", seed=4)
    bmg.to(dev)
    y = torch.randn(8, 2).to(dev)
    good, nV = bmg.batch, int(bmg.V.shape[0])

    def snapshot():
        bn = model.bn
        return (torch.get_rng_state(), tr.opt.steps, bn.running_mean.clone(), bn.running_var.clone(), bn.num_batches_tracked.clone(),
                [p.detach().clone() for p in model.parameters()])

    def unchanged(a, b):
        return (torch.equal(a[0], b[0]) and a[1] == b[1] and all(torch.equal(x, z) for x, z in zip(a[2:5], b[2:5]))
                and all(torch.equal(x, z) for x, z in zip(a[5], b[5])))

    before = snapshot()
    refusals = [
        ("targets", ValueError, "targets must be", lambda: tr.step(bmg, torch.randn(8, 3, generator=torch.Generator().manual_seed(5)).to(dev))),
        ("batch", ValueError, "bmg.batch", lambda: tr.step(bmg, y)),
        ("weights", ValueError, "weights", lambda: tr.step(bmg, y, weights=torch.ones(7, device=dev))),
        ("lt_mask", ValueError, "lt_mask", lambda: tr.step(bmg, y, lt_mask=torch.zeros(8, 1, dtype=torch.bool, device=dev))),
        ("X_d", ValueError, "X_d given", lambda: tr.step(bmg, y, X_d=torch.zeros(8, 3, device=dev))),
        ("V_d", ValueError, "V_d given", lambda: tr.step(bmg, y, V_d=torch.zeros(nV, 2, device=dev))),
        ("eval", RuntimeError, "eval mode", lambda: tr.step(bmg, y)),
    ]
    for what, exc, match, call in refusals:
        if what == "batch":
            bmg.batch = good.int()
        if what == "eval":
            model.eval()
        try:
            with pytest.raises(exc, match=match):
                call()
        finally:
            bmg.batch = good
            model.train()
        assert unchanged(before, snapshot()), what

    tr.step(bmg, y)
    torch.cuda.synchronize()
    torch.set_rng_state(before[0])
    first, second = (int(torch.randint(0, 2 ** 62, (1,), dtype=torch.int64).item()) for _ in range(2))
    assert tr.last_dropout_seed == first
    assert tr.last_head_dropout_seed == second
    assert tr.opt.steps == 1
