"""GPU: a run of ImageGPT blocks as one autograd node (ops.gpt_blocks, ops/gpt_block.py). Without sinks against the same blocks
as a chain of one-block runs, where autograd carries the activations and gradients from block to block and no boundary kernel
runs: the boundary kernels are built from the device functions of the single ones (csrc/gpt_block.hip), so every bit must
agree. With sinks and a chain, where the backward parks, queues, leaves head launches to the tail below and flushes: the launches
it makes, and its results against the same run with the backward boundaries on two launches."""

import pytest
import torch

import _util

pytestmark = pytest.mark.gpu

BWD_LAUNCHES = ("pg_gpt_block_head_tail_bwd_partial", "pg_gpt_block_head_bwd_partial", "pg_gpt_block_tail_bwd_partial",
                "pg_gpt_block_head_bwd", "pg_gpt_block_tail_bwd", "pg_gpt_model_reduce")


@pytest.fixture(scope="module")
def case():
    """3 blocks, 8x8 images = four 16-pixel tiles per image, batch 2, 4 heads; input and output gradient. Left unchanged."""
    from pytorch_generative_amd.models.autoregressive.image_gpt import TransformerBlock

    assert torch.cuda.is_available(), "gpu tests need the MI355X"
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    blocks = [TransformerBlock(16, 4).to(dev) for _ in range(3)]
    with torch.no_grad():
        for p in (p for b in blocks for p in b.parameters()):
            p.add_(torch.randn(p.shape, generator=torch.Generator().manual_seed(p.numel())).to(dev) * 0.1)
    x0 = torch.randn(2, 16, 8, 8, generator=torch.Generator().manual_seed(1)).to(dev)
    dy = torch.randn(2, 16, 8, 8, generator=torch.Generator().manual_seed(2)).to(dev)
    assert all(b._fused_ok(x0) for b in blocks)
    return blocks, x0, dy


def _named(blocks):
    return [(f"{i}.{k}", p) for i, b in enumerate(blocks) for k, p in b.named_parameters()]


def _run(case, forward, sinks=False):
    """One forward and backward; gradients from plain .grad, or from sinks (as FlatAdam hands them out) when sinks is set."""
    blocks, x0, dy = case
    for _, p in _named(blocks):
        p.grad = None
        if sinks:
            p._pg_grad = torch.zeros_like(p)
    try:
        x = x0.clone().requires_grad_(True)
        y = forward(x)
        y.backward(dy)
        torch.cuda.synchronize()
        grads = {k: (p._pg_grad if sinks else p.grad).clone() for k, p in _named(blocks)}
        assert not sinks or all(p.grad is None for _, p in _named(blocks))
    finally:
        for _, p in _named(blocks):
            p.__dict__.pop("_pg_grad", None)
    return y.detach(), x.grad.clone(), grads


def test_a_run_of_three_blocks_equals_three_runs_of_one_bitwise(case):
    """Gradients into plain .grad (every kernel reduces its own rows), attention backward in its fixed-order form."""
    from pytorch_generative_amd import ops

    blocks = case[0]

    def one_by_one(x):
        for b in blocks:
            x = ops.gpt_blocks(x, [b])
        return x

    was = ops.set_deterministic(True)
    try:
        y, dx, grads = _run(case, lambda x: ops.gpt_blocks(x, blocks))
        y1, dx1, grads1 = _run(case, one_by_one)
    finally:
        ops.set_deterministic(was)
    assert bool(torch.isfinite(y).all()) and bool(torch.isfinite(dx).all()) and float(dx.abs().max()) > 0
    assert torch.equal(y, y1), "outputs differ"
    assert torch.equal(dx, dx1), "input gradients differ"
    assert grads.keys() == grads1.keys() and len(grads) == 3 * 14
    for k, g in grads.items():
        assert float(g.abs().max()) > 0, k
        assert torch.equal(g, grads1[k]), f"gradient of {k} differs"


def test_a_flushing_run_with_sinks_launches_as_planned_and_matches_two_launch_boundaries(case, lib, monkeypatch):
    """Every parameter with a sink, a chain that this run flushes. Switch on: the last tail parks, both boundaries run fused, block
    0's head on its own, one reduction of three jobs; off: three parked tails and heads, the same reduction. The fused kernel's
    d_o and gx are the two launches' bits (tests/test_gpu_gpt_boundary_bwd.py), so output and input gradient are compared
    bitwise; its partial rows sum the same tiles over other waves, so the parameter gradients pass the gradient gate of
    _util.GradReport, against each other and against the run without sinks."""
    from pytorch_generative_amd import ops

    blocks = case[0]
    calls = []
    for name in BWD_LAUNCHES:
        real = getattr(lib, name)
        monkeypatch.setattr(lib, name, lambda *a, _n=name, _r=real: (calls.append(_n), _r(*a))[1], raising=False)

    def flushing_run(x):
        return ops.gpt_blocks(x, blocks, ops.new_block_chain(), flush=True)

    got, launched = {}, {}
    was = ops.set_deterministic(True)
    try:
        for on in (True, False):
            monkeypatch.setattr(ops.gpt_block, "FUSE_BOUNDARY_BWD", on)
            del calls[:]
            got[on] = _run(case, flushing_run, sinks=True)
            ops.assert_no_pending_block_reductions()
            launched[on] = [c.replace("pg_gpt_block_", "").replace("pg_gpt_", "") for c in calls]
        plain = _run(case, lambda x: ops.gpt_blocks(x, blocks))
    finally:
        ops.set_deterministic(was)
    assert launched[True] == ["tail_bwd_partial", "head_tail_bwd_partial", "head_tail_bwd_partial", "head_bwd_partial",
                              "model_reduce"], launched[True]
    assert launched[False] == ["tail_bwd_partial", "head_bwd_partial"] * 3 + ["model_reduce"], launched[False]
    for other, what in ((got[False], "two-launch boundaries"), (plain, "no sinks")):
        assert torch.equal(got[True][0], other[0]), f"output differs from {what}"
        assert torch.equal(got[True][1], other[1]), f"input gradient differs from {what}"
        rep = _util.GradReport(f"gpt_blocks[sinks, fused boundaries vs {what}]")
        for k, g in got[True][2].items():
            rep.add(k, g, other[2][k])
        assert len(rep.rows) == 3 * 14
        rep.finish()
