"""GPU: the d_k = d_v = 4 matrix-core attention (csrc/attention_mfma.hip) with the front-loaded query partition
of its forward and dQ kernels: a sequence whose 16-query groups do not fill whole 64-query blocks puts the short
block FIRST (queries [0, 16 F)), every later block holds four groups. Output and the three input gradients against
float64 `oracle.ops.causal_attention_core`, with the fused backward and with the two-kernel backward
(`ops.set_deterministic`, whose dQ kernel is partitioned the same way); both read the forward's lse.

Shapes: every way the groups can fall (one group, F = 0..3, L % 16 != 0, odd L with scalar stores, one block per
wave, the 13-block plan of the bench) at the smallest size that has it. The boosted cases scale q so that the
scores step up at key-tile boundaries by enough for exp2(score) to grow far more than 2^8-fold from one tile to the
next, so that the lazy running-max rescale of the forward fires inside blocks whose groups are not the ones the
64-aligned partition put together; N(0, 1) inputs never reach it.
Tolerances are the suite's own: 1e-4 max-norm for the output, `_util.GradReport` for the gradients."""

import functools

import pytest
import torch

import _util
from oracle import ops as oops

pytestmark = pytest.mark.gpu

TOL = 1e-4
N = 2

SHAPES = [
    (1, 16),   # L = 16: one group
    (4, 12),   # L = 48: one short block
    (8, 8),    # L = 64: F = 0, one whole block
    (5, 16),   # L = 80: F = 1, the bench's remainder at the smallest size
    (10, 10),  # L = 100: F = 3, L % 16 != 0
    (9, 13),   # L = 117: odd L, scalar stores
    (7, 32),   # L = 224: F = 2, one block per wave
    (28, 28),  # L = 784: 13 blocks, the plan the bench runs
]
# key positions (multiples of 16) at which the boosted cases' scores step up
BOOST_STEPS = {80: (32, 48), 784: (64, 400, 656)}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need the MI355X"
    from pytorch_generative_amd import _lib

    _lib.load()  # fail loudly if the extension is missing
    return torch.device("cuda:0")


def _rand(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


@functools.lru_cache(maxsize=None)
def _case(h, w, heads, strict, boost):
    """Inputs and the float64 reference (output, dq, dk, dv) of one case: made once, shared by both backward paths."""
    e = v = heads * 4
    q, kv, d_o = _rand(N, e, h, w, seed=1), _rand(N, e + v, h, w, seed=2), _rand(N, v, h, w, seed=3)
    if boost:
        # channel 0 of every head: q = 128 * (1 +- 5 / 32), k = 0.25 * (steps passed). At every step all later scores
        # rise by at least 0.72 * 108 * 0.25 = 19 log2 units (0.72 = log2(e) / sqrt(d_k)): exp2(score - running max)
        # jumps to 2^19, far past the 2^8 at which the kernel moves its running max. The size is put into q, and k
        # stays within the unit scale of its other channels, for the sake of the reference, not of the kernel: a row
        # of dS sums to zero, so a constant offset c in k adds c * eps * sum|dS| of rounding to dq that nothing in the
        # exact result balances, and the gradient gate's floor is set for unit-scale operands. Likewise the scores stay
        # below 2^7, where fp32 resolves them to 1e-5; steps of 2^8 log2 units themselves would put them past 2^9,
        # where the spacing of fp32 numbers alone (6e-5) is the size of the tolerance.
        pos = torch.arange(h * w).reshape(1, 1, h, w)
        q[:, 0:e:4] = 128.0 * (1.0 + q[:, 0:e:4].clamp(-5.0, 5.0) / 32)
        kv[:, 0:e:4] = sum((pos >= s).float() for s in BOOST_STEPS[h * w]) * 0.25
    qo, kvo = q.double().requires_grad_(True), kv.double().requires_grad_(True)
    oo = oops.causal_attention_core(qo, kvo[:, :e], kvo[:, e:], heads, strict)
    oo.backward(d_o.double())
    return q, kv, d_o, oo.detach(), qo.grad, kvo.grad[:, :e], kvo.grad[:, e:]


def _check(dev, h, w, heads, strict, deterministic, boost):
    from pytorch_generative_amd import ops

    e = v = heads * 4
    L = h * w
    q, kv, d_o, o_ref, dq_ref, dk_ref, dv_ref = _case(h, w, heads, strict, boost)
    was = ops.set_deterministic(deterministic)
    try:
        qg, kvg = q.to(dev).requires_grad_(True), kv.to(dev).requires_grad_(True)
        og = ops.causal_attention(qg, kvg, heads, e, v, strict)
        og.backward(d_o.to(dev))
        torch.cuda.synchronize()
    finally:
        ops.set_deterministic(was)
    what = f"L={L} heads={heads} strict={strict} deterministic={deterministic} boost={boost}"
    got, want = og.detach().cpu().reshape(N, v, L), o_ref.reshape(N, v, L)
    print(f"[partition] {what}: output max-norm err {_util.rel_err(got, want):.3e}")
    assert bool(torch.isfinite(got).all()), what
    _util.assert_close(got, want, TOL, what + " output")  # every row
    first = 16 * (-(-L // 16) % 4)  # 16 F: the rows block 0 computes along with its own but must leave to block 1
    if 0 < first < L:
        _util.assert_close(got[:, :, first:], want[:, :, first:], TOL, what + f" output rows >= {first}")
    if strict:  # the row with no allowed key is exactly zero
        assert torch.equal(got[:, :, 0], torch.zeros(N, v))
    rep = _util.GradReport(what)
    rep.add("dq", qg.grad, dq_ref)
    rep.add("dk", kvg.grad[:, :e], dk_ref)
    rep.add("dv", kvg.grad[:, e:], dv_ref)
    rep.finish()


@pytest.mark.parametrize("deterministic", [False, True], ids=["fused-bwd", "two-kernel-bwd"])
@pytest.mark.parametrize("strict", [False, True], ids=["mask-b", "mask-center"])
@pytest.mark.parametrize("heads", [2, 4])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"L{s[0] * s[1]}")
def test_front_loaded_partition_against_float64(dev, shape, heads, strict, deterministic):
    _check(dev, shape[0], shape[1], heads, strict, deterministic, boost=False)


@pytest.mark.parametrize("deterministic", [False, True], ids=["fused-bwd", "two-kernel-bwd"])
@pytest.mark.parametrize("shape", [(5, 16), (28, 28)], ids=["L80", "L784"])
def test_running_max_rescale_in_regrouped_blocks(dev, shape, deterministic):
    _check(dev, shape[0], shape[1], 2, False, deterministic, boost=True)
