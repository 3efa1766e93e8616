"""GPU: the categorical pixel likelihood (csrc/categorical.hip) — the loss, lse, per-sample sums and the logits gradient
against the float64 restatement of tests/_categorical_ref.py: the issue's nine shapes (the planner gives them 1, 4 or
8 lanes per sub-pixel) and six more that reach the split over 2 lanes and K up to the limit of 4096, on the scalar and the
4-wide path (tests/test_categorical_ref_cpu.py checks that the cases reach every split the planner gives: 1, 2, 4, 8),
classes that no split divides, logits
that overflow without the max subtraction, the residual plane of lse, bit reproducibility; the per-position draw
against the float64 pick on strided views; and the public surface on a small PixelCNN (graph replay == eager, the
recipe, sample() on both samplers) and ImageGPT."""

import copy
import functools
import glob
import os

import pytest
import torch

import _categorical_ref as ref
import _util

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)

# (N, C, K, H, W)
SHAPES = [
    (1, 1, 2, 1, 1),       # smallest problem
    (2, 1, 3, 1, 5),       # HW odd, scalar path
    (3, 3, 7, 2, 3),       # several channels
    (2, 1, 256, 4, 4),     # K = 256
    (1, 1, 257, 2, 2),     # K not divisible by any lane split
    (5, 1, 512, 3, 4),     # K = 512
    (2, 3, 64, 5, 7),      # three channels, odd HW
    (70, 1, 16, 8, 8),     # more samples than one wave
    (64, 1, 256, 28, 28),  # the recipe's shape (plain logits only)
]
RECIPE = SHAPES[-1]
# The planner splits a sub-pixel's classes over S = K / 64 (rounded down to a power of two, at most 8) lanes whatever N, C
# and HW are: the shapes above reach S = 1, 4 and 8 (the last on the 4-wide path only). These add S = 2, S = 8 on the scalar
# path and the largest K, small.
SPLIT_SHAPES = [
    (1, 1, 130, 1, 5),     # S = 2, scalar path, K not a multiple of the split
    (2, 1, 128, 2, 2),     # S = 2, 4-wide
    (1, 1, 1024, 2, 2),    # S = 8, 128 classes per lane
    (1, 1, 2048, 1, 3),    # S = 8, scalar path
    (1, 1, 4096, 2, 2),    # the largest K
    (3, 1, 4096, 1, 3),    # the largest K, odd HW, units of several images
]
VARIANTS = [(s, "plain") for s in SHAPES + SPLIT_SHAPES] + [(s, "wide") for s in SHAPES[:-1] + SPLIT_SHAPES]


@functools.lru_cache(maxsize=None)
def _case(shape, variant):
    """Inputs and the float64 reference of one case, computed once: (logits, images, loss, per_sample, lse, grad)."""
    n, c, k, h, w = shape
    g = torch.Generator().manual_seed(1000 * n + 100 * c + k + 7 * h * w + (variant != "plain"))
    logits = torch.randn(n, k * c, h, w, generator=g) * 3
    if variant == "wide":  # exp() of these overflows fp32 unless the maximum is subtracted
        sign = torch.randint(0, 2, (n, 1, c, h, w), generator=g).float() * 2 - 1
        logits = (logits.view(n, k, c, h, w) * 30 + 80 * sign).reshape(n, k * c, h, w)
    elif variant == "equal":  # some sub-pixels whose K logits are all the same
        flat = logits.view(n, k, c * h * w)
        flat[:, :, ::2] = 5.0
    t = torch.randint(0, k, (n, c, h, w), generator=g)
    t.view(-1)[0] = 0
    t.view(-1)[-1] = k - 1  # both end classes (a single sub-pixel keeps the last one)
    images = ref.to_level(t, k)
    assert torch.equal(ref.classes(images, k), t)
    loss, grad = ref.loss_and_grad(logits, images, k)
    return logits, images, loss, ref.nll_per_sample(logits, images, k), ref.lse(logits, k), grad


def _run(logits, images, k, grad_output=None):
    from pytorch_generative_amd import ops

    z = logits.to(DEV).requires_grad_(True)
    x = images.to(DEV)
    loss = ops.categorical_nll_sum_mean(z, x, k)
    lse = loss.grad_fn.saved_tensors[2]  # (2, N, C, H, W): lse and the rounding residual of its last addition
    (loss if grad_output is None else loss * grad_output).backward()
    torch.cuda.synchronize()
    return loss.detach(), lse, z.grad


@pytest.mark.parametrize("shape,variant", VARIANTS + [(SHAPES[2], "equal"), (SHAPES[3], "equal")],
                         ids=lambda v: v if isinstance(v, str) else "x".join(map(str, v)))
def test_op_parity_float64(shape, variant):
    from pytorch_generative_amd import ops

    n, c, k, h, w = shape
    logits, images, want_loss, want_ps, want_lse, want_grad = _case(shape, variant)
    loss, planes, grad = _run(logits, images, k)
    lse = planes[0]
    per_sample = ops.categorical_nll_per_sample(logits.to(DEV), images.to(DEV), k)
    what = f"{shape} {variant}"
    print(f"[categorical] {what}: loss {_util.rel_err(loss, want_loss):.2e} per-sample {_util.rel_err(per_sample, want_ps):.2e} "
          f"lse {_util.rel_err(lse, want_lse):.2e}")
    assert lse.shape == images.shape and per_sample.shape == (n,) and grad.shape == logits.shape
    assert not per_sample.requires_grad
    _util.assert_close(loss, want_loss, 1e-5, f"{what} loss")
    _util.assert_close(per_sample, want_ps, 1e-5, f"{what} per-sample loss")
    _util.assert_close(lse, want_lse, 1e-5, f"{what} lse")
    # lse + residual is the normaliser the backward uses. Its error is that of log(sum) alone, whatever the size of the
    # logits: the sum's terms near the maximum carry the 2 ulp of the hardware exp (2.4e-7), the accumulation over a lane's
    # classes and the merges less than that again, logf 1e-7: 4e-6 leaves a factor of several, and is a quarter of the
    # 1.5e-5 that rounding lse itself to fp32 costs at the wide logits' size of 400.
    two = planes[0].double().cpu() + planes[1].double().cpu()
    err = float((two - want_lse).abs().max())
    print(f"[categorical] {what}: |lse + residual - float64| {err:.2e}")
    assert err <= 4e-6, f"{what}: lse + residual off by {err:.2e}"
    rep = _util.GradReport(f"categorical {what}")
    rep.add("dlogits", grad, want_grad)
    rep.finish()


@pytest.mark.parametrize("shape", [SHAPES[1], SHAPES[4], SHAPES[7], RECIPE, SPLIT_SHAPES[0], SPLIT_SHAPES[4]],
                         ids=lambda s: "x".join(map(str, s)))
def test_gradient_is_bit_reproducible_and_scales_exactly(shape):
    k = shape[2]
    logits, images = _case(shape, "plain")[:2]
    _, lse1, grad1 = _run(logits, images, k)
    _, lse2, grad2 = _run(logits, images, k)
    assert torch.equal(lse1, lse2) and torch.equal(grad1, grad2)
    _, _, half = _run(logits, images, k, grad_output=0.5)
    assert torch.equal(half, grad1 * 0.5)


def test_images_gradient_is_none_and_shapes_are_checked():
    from pytorch_generative_amd import ops

    logits, images = _case(SHAPES[2], "plain")[:2]
    z, x = logits.to(DEV).requires_grad_(True), images.to(DEV).requires_grad_(True)
    ops.categorical_nll_sum_mean(z, x, 7).backward()
    assert x.grad is None and z.grad is not None
    with pytest.raises(ValueError):
        ops.categorical_nll_sum_mean(z, x, 8)
    with pytest.raises(ValueError):
        ops.categorical_nll_per_sample(z.detach()[:, :, :1], x.detach(), 7)
    with pytest.raises(ValueError):
        ops.categorical_sample(torch.zeros(2, 14, device=DEV), torch.zeros(2, 3, device=DEV), 7)


# ---- the draw ---------------------------------------------------------------------------------------------------------

def _interior_uniforms(logits2d, k, temperature, g):
    """Per draw a class of probability >= 1e-3 and the midpoint of its CDF interval: at least 5e-4 from a boundary, far
    above the fp32 error of a 257-term running sum."""
    run, total = ref.cdf(logits2d, k, temperature)
    cdf = run / total.unsqueeze(2)
    lower = torch.cat([torch.zeros_like(cdf[:, :, :1]), cdf[:, :, :-1]], dim=2)
    prob = cdf - lower
    score = torch.rand(prob.shape, generator=g, dtype=torch.float64) * (prob >= 1e-3)
    cls = score.argmax(dim=2)
    assert bool((prob.gather(2, cls.unsqueeze(2)) >= 1e-3).all())
    u = (0.5 * (lower + cdf)).gather(2, cls.unsqueeze(2)).squeeze(2).float()
    return u, cls


@pytest.mark.parametrize("temperature", [1.0, 0.5])
@pytest.mark.parametrize("c", [1, 3])
@pytest.mark.parametrize("n", [1, 70])
@pytest.mark.parametrize("k", [2, 7, 256, 257])
def test_sampler_matches_float64_pick(k, n, c, temperature):
    from pytorch_generative_amd import ops

    g = torch.Generator().manual_seed(k * 1000 + n * 10 + c + int(temperature * 4))
    w, col = 3, 1
    row = torch.randn(n, k * c, 1, w, generator=g) * 3
    u, cls = _interior_uniforms(row[:, :, 0, col], k, temperature, g)
    assert torch.equal(ref.pick(row[:, :, 0, col], u, k, temperature), cls)
    view = row.to(DEV)[:, :, 0, col]
    assert not view.is_contiguous() or n * k * c == 1
    got = ops.categorical_sample(view, u.to(DEV), k, temperature)
    torch.cuda.synchronize()
    assert got.shape == (n, c) and got.dtype == torch.float32
    assert torch.equal(got.cpu(), ref.to_level(cls, k))
    # the (n, c) layout ImageGPT's decoder hands over: contiguous
    again = ops.categorical_sample(view.contiguous(), u.to(DEV), k, temperature)
    assert torch.equal(again, got)


@pytest.mark.parametrize("k", [2, 7, 257])
def test_sampler_edge_cases(k):
    from pytorch_generative_amd import ops

    # u = 0, no mass on class 0: the comparison is strict, so class 1
    z = torch.zeros(1, k)
    z[0, 0] = -200.0
    got = ops.categorical_sample(z.to(DEV), torch.zeros(1, 1, device=DEV), k)
    assert torch.equal(got.cpu(), ref.to_level(torch.tensor([[1]]), k))
    # the largest u below 1: the last class with mass, whichever lane holds it
    u1 = torch.nextafter(torch.tensor([[1.0]]), torch.tensor([[0.0]]))
    for last in sorted({0, (k - 1) // 2, k - 2, k - 1}):
        z = torch.full((1, k), -2000.0)
        z[0, :last + 1] = torch.linspace(0.0, 1.0, last + 1)
        got = ops.categorical_sample(z.to(DEV), u1.to(DEV), k)
        assert torch.equal(got.cpu(), ref.to_level(torch.tensor([[last]]), k)), last
        assert ref.pick(z, u1, k).item() == last
    # every level comes out as the fp32 quotient class / (K - 1)
    z = torch.full((k, k), -2000.0)
    z.fill_diagonal_(0.0)
    got = ops.categorical_sample(z.to(DEV), torch.full((k, 1), 0.5, device=DEV), k)
    assert torch.equal(got.cpu().view(-1), ref.levels(k))


# ---- models -----------------------------------------------------------------------------------------------------------

K_MODEL = 8


def _pixel_cnn(sample_fn=None, seed=0):
    import pytorch_generative_amd as pg

    torch.manual_seed(seed)
    return pg.models.PixelCNN(in_channels=1, out_channels=K_MODEL, n_residual=2, residual_channels=4, head_channels=8,
                              sample_fn=sample_fn).to(DEV)


def _grey_batches(n_batches, n=16, seed=5):
    g = torch.Generator().manual_seed(seed)
    return [ref.to_level(torch.randint(0, K_MODEL, (n, 1, 8, 8), generator=g), K_MODEL) for _ in range(n_batches)]


def test_graphed_steps_equal_eager_bitwise():
    from pytorch_generative_amd import graph, ops, optim, recipes

    was = ops.set_deterministic(True)
    try:
        loss3 = recipes.categorical_loss(K_MODEL)
        loss_fn = lambda x, preds: loss3(x, None, preds)  # noqa: E731
        xs = [x.to(DEV) for x in _grey_batches(3)]
        m1 = _pixel_cnn()
        m2 = copy.deepcopy(m1)
        o1, o2 = optim.FlatAdam(m1.parameters(), lr=1e-3), optim.FlatAdam(m2.parameters(), lr=1e-3)
        for x in xs:
            o1.zero_grad()
            loss_fn(x, m1(x)).backward()
            o1.step()
        step = graph.GraphedTrainStep(m2, o2, loss_fn, xs[0], preserve_state=True)
        for x in xs:
            step(x)
        torch.cuda.synchronize()
        before = _pixel_cnn()
        changed = False
        for (k, p1), (_, p2), (_, p0) in zip(m1.named_parameters(), m2.named_parameters(), before.named_parameters()):
            assert torch.equal(p1, p2), f"{k}: graph replay differs from eager steps"
            changed = changed or not torch.equal(p1, p0)
        assert changed, "three steps left every parameter as it was"
    finally:
        ops.set_deterministic(was)


def test_recipe_trains_one_epoch_and_checkpoints(tmp_path):
    from pytorch_generative_amd import recipes

    loader = [(x, torch.zeros(x.shape[0])) for x in _grey_batches(2)]
    t = recipes.run(lambda: _pixel_cnn(), loaders=recipes.grey_mnist, loss_fn=recipes.categorical_loss(K_MODEL), lr=1e-3,
                    n_epochs=1, batch_size=16, log_dir=str(tmp_path), n_gpus=1, device_id=0, debug_loader=loader)
    assert t._epoch == 1 and t._step == 2
    assert all(bool(torch.isfinite(p).all()) for p in t.model.parameters())
    assert glob.glob(os.path.join(str(tmp_path), "trainer_state_1.ckpt")), os.listdir(str(tmp_path))
    assert all(v == v and abs(v) != float("inf") for v in t.last_eval_metrics.values()) and t.last_eval_metrics


def test_grey_mnist_serves_the_levels_the_loss_decodes():
    from pytorch_generative_amd import recipes

    with pytest.warns(UserWarning):
        train, _ = recipes.grey_mnist(4)
    x = next(iter(train))[0].cpu()
    assert tuple(x.shape) == (4, 1, 28, 28) and x.dtype == torch.float32
    assert torch.equal(ref.to_level(ref.classes(x, 256), 256), x), "grey MNIST batches are not at the levels j / 255"


def _recording_sampler(seed):
    from pytorch_generative_amd import nn as pg_nn

    class Recording(pg_nn.CategoricalSampler):
        def __init__(self):
            super().__init__(K_MODEL, generator=torch.Generator(device=DEV).manual_seed(seed))
            self.records = []

        def __call__(self, logits):
            u = torch.rand((logits.shape[0], logits.shape[1] // self.n_classes), device=logits.device,
                           generator=self.generator)
            out = self.draw(logits, u)
            self.records.append((logits.detach().clone(), u, out))
            return out

    return Recording()


@pytest.mark.parametrize("incremental", [True, False])
def test_pixel_cnn_sample(incremental):
    from pytorch_generative_amd import nn as pg_nn

    g = torch.Generator().manual_seed(11)
    cond = torch.full((2, 1, 8, 8), -1.0)
    given = torch.rand(2, 1, 8, 8, generator=g) < 0.3
    cond[given] = ref.to_level(torch.randint(0, K_MODEL, (int(given.sum()),), generator=g), K_MODEL)
    levels = ref.levels(K_MODEL)

    canvases = []
    for _ in range(2):
        sampler = pg_nn.CategoricalSampler(K_MODEL, generator=torch.Generator(device=DEV).manual_seed(77))
        model = _pixel_cnn(sample_fn=sampler).eval()
        canvases.append(model.sample(conditioned_on=cond.to(DEV), incremental=incremental).cpu())
    canvas = canvases[0]
    assert torch.equal(canvases[0], canvases[1]), "the same generator seed must give the same canvas"
    assert canvas.shape == cond.shape
    assert torch.equal(canvas[given], cond[given]), "given entries must be kept"
    assert bool(torch.isin(canvas, levels).all()), "every entry is a level j / 7"

    rec = _recording_sampler(77)
    model = _pixel_cnn(sample_fn=rec).eval()
    assert torch.equal(model.sample(conditioned_on=cond.to(DEV), incremental=incremental).cpu(), canvas)
    torch.cuda.synchronize()
    assert len(rec.records) == 64
    excepted = draws = 0
    for logits, u, out in rec.records:
        logits, u, out = logits.cpu(), u.cpu(), out.cpu()
        assert logits.shape == (2, K_MODEL) and u.shape == out.shape == (2, 1)
        run, total = ref.cdf(logits, K_MODEL)
        near = ((run / total.unsqueeze(2) - u.double().unsqueeze(2)).abs() < 1e-4).any(dim=2)
        agree = out == ref.to_level(ref.pick(logits, u, K_MODEL), K_MODEL)
        assert bool((agree | near).all()), "a draw away from every CDF boundary differs from the float64 pick"
        assert bool(torch.isin(out, levels).all())
        excepted += int(near.sum())
        draws += near.numel()
    print(f"[categorical] sample incremental={incremental}: {excepted} of {draws} draws within 1e-4 of a CDF boundary")
    assert draws == 128 and excepted <= 2


def test_image_gpt_sample():
    import pytorch_generative_amd as pg
    from pytorch_generative_amd import nn as pg_nn

    torch.manual_seed(3)
    sampler = pg_nn.CategoricalSampler(4, generator=torch.Generator(device=DEV).manual_seed(5))
    model = pg.models.ImageGPT(in_channels=1, out_channels=4, in_size=8, n_transformer_blocks=1, n_attention_heads=2,
                               n_embedding_channels=4, sample_fn=sampler).to(DEV).eval()
    cond = torch.full((3, 1, 8, 8), -1.0)
    cond[:, :, :2, :] = ref.to_level(torch.randint(0, 4, (3, 1, 2, 8), generator=torch.Generator().manual_seed(1)), 4)
    got = model.sample(conditioned_on=cond.to(DEV)).cpu()
    assert got.shape == (3, 1, 8, 8)
    assert torch.equal(got[:, :, :2, :], cond[:, :, :2, :]), "given entries must be kept"
    assert bool(torch.isin(got, ref.levels(4)).all()), "every entry is a level j / 3"
