"""GPU: the forward block boundary of ImageGPT in one launch (csrc/gpt_block.hip, tail_head_fwd_kernel: the tail of block i and
LN1 + the q/kv projection of block i+1 on the x_new register tile) against the two launches it replaces, bit for bit — the two
forms run the same device functions, so anything but equality is a difference in how the compiler contracted them. Kernel
level through the C-ABI at the tile counts where the walk changes (one tile, a walk that crosses images, the bench's 49 tiles
per image, three tiles per wave under the launch's own grid rule), then the model: loss and gradients with the switch on and
off, and replays of the captured step against eager steps."""

import pytest
import torch

pytestmark = pytest.mark.gpu

EPS = 1e-5
PG_ESHAPE = -2
# (N, L). The fused launch has min(ceil(tiles / 4), 1536) workgroups of four waves (grid_blocks, which = 4): at 384 x 49 = 18 816
# tiles each of its 6144 waves walks three tiles and the first 384 a fourth — prologue, steady iterations and the last
# iteration's re-read of its own tile in one wave
SHAPES = {"one_tile": (1, 16), "crosses_images": (3, 48), "bench_row_count": (2, 784), "three_tiles_per_wave": (384, 784)}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need the MI355X"
    return torch.device("cuda:0")


def _rand(*shape, seed, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


@pytest.fixture(scope="module")
def params(dev):
    """tail of block i: wp, bp, ln2 w/b, w1, b1, w2, b2; head of block i+1: ln1 w/b, wq, bq, wkv, bkv"""
    tail = [_rand(16, 16, seed=10, scale=.2), _rand(16, seed=11), 1 + _rand(16, seed=12, scale=.1), _rand(16, seed=13, scale=.1),
            _rand(64, 16, seed=14, scale=.2), _rand(64, seed=15), _rand(16, 64, seed=16, scale=.1), _rand(16, seed=17)]
    head = [1 + _rand(16, seed=20, scale=.1), _rand(16, seed=21, scale=.1), _rand(16, 16, seed=22, scale=.2), _rand(16, seed=23),
            _rand(32, 16, seed=24, scale=.2), _rand(32, seed=25)]
    return [t.to(dev) for t in tail], [t.to(dev) for t in head]


def _ptrs(ts):
    return [t.data_ptr() for t in ts]


@pytest.mark.parametrize("case", list(SHAPES))
def test_fused_boundary_equals_tail_then_head_bitwise(dev, lib, params, case):
    n, L = SHAPES[case]
    tail, head = params
    x, o = _rand(n, 16, L, seed=1).to(dev), _rand(n, 16, L, seed=2).to(dev)
    nan = lambda c: torch.full((n, c, L), float("nan"), device=dev)  # noqa: E731
    xnew_a, qkv_a, xnew_b, qkv_b = nan(16), nan(48), nan(16), nan(48)
    st = torch.cuda.current_stream().cuda_stream
    assert lib.pg_gpt_block_tail_fwd(o.data_ptr(), x.data_ptr(), *_ptrs(tail), xnew_a.data_ptr(), n, 16, 64, L, EPS, st) == 0
    assert lib.pg_gpt_block_head_fwd(xnew_a.data_ptr(), *_ptrs(head), qkv_a.data_ptr(), n, 16, L, EPS, st) == 0
    assert lib.pg_gpt_block_tail_head_fwd(o.data_ptr(), x.data_ptr(), *_ptrs(tail), xnew_b.data_ptr(), *_ptrs(head),
                                          qkv_b.data_ptr(), n, 16, 64, L, EPS, st) == 0
    torch.cuda.synchronize()
    assert bool(torch.isfinite(xnew_a).all()) and bool(torch.isfinite(qkv_a).all())
    assert torch.equal(xnew_b, xnew_a), f"{case}: x_new of the fused launch differs from pg_gpt_block_tail_fwd"
    assert torch.equal(qkv_b, qkv_a), f"{case}: qkv of the fused launch differs from pg_gpt_block_head_fwd"


def test_unqualifying_channel_count_is_refused_and_writes_nothing(dev, lib, params):
    n, c, L = 2, 32, 48
    tail, head = params
    x, o = _rand(n, c, L, seed=1).to(dev), _rand(n, c, L, seed=2).to(dev)
    xnew, qkv = torch.full((n, c, L), float("nan"), device=dev), torch.full((n, 3 * c, L), float("nan"), device=dev)
    st = torch.cuda.current_stream().cuda_stream
    rc = lib.pg_gpt_block_tail_head_fwd(o.data_ptr(), x.data_ptr(), *_ptrs(tail), xnew.data_ptr(), *_ptrs(head), qkv.data_ptr(),
                                        n, c, 64, L, EPS, st)
    torch.cuda.synchronize()
    assert rc == PG_ESHAPE
    assert bool(torch.isnan(xnew).all()) and bool(torch.isnan(qkv).all())


# ------------------------------------------------------------------------------------------------ model level
def _model(dev):
    import pytorch_generative_amd as pg

    torch.manual_seed(0)
    m = pg.models.ImageGPT(1, 1, in_size=28, n_transformer_blocks=2, n_attention_heads=4, n_embedding_channels=16)
    with torch.no_grad():
        m._pos.normal_(0, 0.1)
    return m.to(dev)


def _batches(dev, k):
    g = torch.Generator().manual_seed(11)
    return [torch.bernoulli(torch.full((2, 1, 28, 28), 0.1307), generator=g).to(dev) for _ in range(k)]


def _count(monkeypatch, lib, name, calls):
    real = getattr(lib, name)
    monkeypatch.setattr(lib, name, lambda *a: (calls.append(name), real(*a))[1], raising=False)


def test_loss_and_gradients_equal_with_the_switch_on_and_off(dev, lib, monkeypatch):
    """One step of a 2-block ImageGPT either way: the fused launch runs once (one boundary) and replaces one tail_fwd and one
    head_fwd launch; the logits and every parameter gradient are the same bits, and so is the loss summed from the logits in a
    fixed order. The scalar that ops.bce_with_logits_sum_mean returns is NOT compared bit for bit: bce_fwd_kernel adds its up to
    512 workgroup sums with atomicAdd in completion order, and two runs with the SAME switch setting differ in its last bit
    (measured: 419.0448 against 419.04477, one ulp, with logits and gradients equal). It is held to the reordering bound of that
    sum instead, (512 - 1) * 2^-24 * loss; its gradient does not depend on its value."""
    import torch.nn.functional as F

    from pytorch_generative_amd import ops, optim

    calls = []
    for name in ("pg_gpt_block_tail_head_fwd", "pg_gpt_block_tail_fwd", "pg_gpt_block_head_fwd"):
        _count(monkeypatch, lib, name, calls)
    x = _batches(dev, 1)[0]
    was = ops.set_deterministic(True)
    try:
        got = {}
        for on in (True, False):
            monkeypatch.setattr(ops.gpt_block, "FUSE_BOUNDARY", on)
            del calls[:]
            m = _model(dev)
            opt = optim.FlatAdam(m.parameters(), lr=1e-3)
            opt.zero_grad()
            logits = m(x)
            loss = ops.bce_with_logits_sum_mean(logits, x)
            loss.backward()
            torch.cuda.synchronize()
            n = {k: calls.count(k) for k in set(calls)}
            want = ({"pg_gpt_block_tail_head_fwd": 1, "pg_gpt_block_tail_fwd": 1, "pg_gpt_block_head_fwd": 1} if on else
                    {"pg_gpt_block_tail_fwd": 2, "pg_gpt_block_head_fwd": 2})
            assert n == want, f"FUSE_BOUNDARY={on}: forward launches {n}"
            ordered = F.binary_cross_entropy_with_logits(logits.detach().cpu().double(), x.cpu().double(), reduction="sum") / x.shape[0]
            got[on] = (logits.detach().clone(), ordered, float(loss), {k: p.grad.detach().clone() for k, p in m.named_parameters()})
    finally:
        ops.set_deterministic(was)
    assert torch.equal(got[True][0], got[False][0]), "logits differ"
    assert torch.equal(got[True][1], got[False][1]), "loss (fixed summation order) differs"
    assert abs(got[True][2] - got[False][2]) <= 511 * 2.0 ** -24 * abs(got[False][2]), "loss differs by more than a reordered sum can"
    assert len(got[True][3]) == len(got[False][3]) > 0
    for k, g in got[True][3].items():
        assert torch.equal(g, got[False][3][k]), f"gradient of {k} differs"


def test_graph_replays_of_the_fused_step_equal_eager_steps(dev):
    """Three replays of the captured step equal three eager steps bit for bit under ops.set_deterministic(True); the fused
    boundary is selected whatever the switch's default."""
    from pytorch_generative_amd import graph, ops, optim

    xs = _batches(dev, 3)
    loss_fn = lambda x, preds: ops.bce_with_logits_sum_mean(preds, x)  # noqa: E731
    was, sw = ops.set_deterministic(True), ops.gpt_block.FUSE_BOUNDARY
    ops.gpt_block.FUSE_BOUNDARY = True
    try:
        m1, m2 = _model(dev), _model(dev)
        o1, o2 = optim.FlatAdam(m1.parameters(), lr=1e-3), optim.FlatAdam(m2.parameters(), lr=1e-3)
        for x in xs:
            o1.zero_grad()
            loss_fn(x, m1(x)).backward()
            o1.step()
        step = graph.GraphedTrainStep(m2, o2, loss_fn, xs[0], preserve_state=True)
        for x in xs:
            step(x)
        torch.cuda.synchronize()
        assert torch.equal(o1.flat_param, o2.flat_param), "graph replays differ from eager steps"
        assert torch.equal(o1.exp_avg, o2.exp_avg) and torch.equal(o1.exp_avg_sq, o2.exp_avg_sq)
    finally:
        ops.gpt_block.FUSE_BOUNDARY = sw
        ops.set_deterministic(was)
