"""GPU: the model's last 1x1 convolution fused into the categorical likelihood (csrc/linear_categorical.hip, ops.DeferredLogits,
defer_head) against the float64 restatement of tests/_linear_categorical_ref.py, with the gates of
tests/test_gpu_categorical.py: 1e-5 on loss / lse / per-sample sums, lse + residual within 4e-6 absolute (the bound that file
derives: the normaliser's error is that of log(sum) alone), _util.GradReport defaults on dh, dW, db, dln_w, dln_b. Then bit
reproducibility, the fused route next to .dense() + the dense kernels, the four models with defer_head on and off (loss,
gradients, graph replay == eager, the recipe, sample()), an unsupported head, and the memory the op takes."""

import copy
import functools
import glob
import os

import pytest
import torch

import _categorical_ref as cref
import _linear_categorical_ref as ref
import _util

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)

# (N, Cin, K, C, H, W)
SHAPES = [
    (1, 4, 2, 1, 1, 1),        # smallest problem
    (2, 4, 3, 1, 1, 5),        # K below one class tile, HW odd
    (3, 20, 7, 3, 2, 3),       # several channels, Cin not a multiple of 16
    (70, 4, 257, 1, 1, 5),     # tiles span images, K no multiple of anything
    (2, 16, 256, 1, 4, 4),     # several class tiles
    (5, 64, 512, 1, 3, 4),     # K = 512
    (2, 64, 64, 3, 5, 7),      # three channels
    (1, 256, 16, 1, 8, 8),     # widest Cin
    (1, 8, 4096, 1, 2, 2),     # largest K
]
RECIPE = (64, 16, 256, 1, 28, 28)  # the recipe's shape, LN only
VARIANT_SHAPES = [SHAPES[2], SHAPES[3], SHAPES[4], SHAPES[6]]
CASES = ([(s, t, "plain", True) for s in SHAPES for t in ref.TRANSFORMS] + [(RECIPE, "ln", "plain", True)]
         + [(s, t, "wide", True) for s in VARIANT_SHAPES for t in ref.TRANSFORMS]
         + [(s, t, "plain", False) for s in VARIANT_SHAPES for t in ref.TRANSFORMS]
         + [(s, t, "equal", True) for s in (SHAPES[2], SHAPES[4]) for t in ref.TRANSFORMS])
GRADS = ("dh", "dW", "db", "dln_w", "dln_b")


def _id(v):
    if isinstance(v, tuple):
        return "x".join(map(str, v))
    return {True: "bias", False: "nobias"}.get(v, v)


@functools.lru_cache(maxsize=None)
def _case(shape, transform, variant, bias):
    """The fp32 inputs and their float64 reference, computed once and shared."""
    case = ref.make_case(shape, transform, variant, bias)
    return case, ref.reference(case)


def _head(case):
    """The head as the models hold it: a 1x1 Conv2d (and the LayerNorm in front of it) carrying the case's parameters."""
    from pytorch_generative_amd import nn as pg_nn

    kc, cin = case["w"].shape
    conv = pg_nn.Conv2d(in_channels=cin, out_channels=kc, kernel_size=1, bias=case["b"] is not None).to(DEV)
    ln = None
    with torch.no_grad():
        conv.weight.copy_(case["w"].view(kc, cin, 1, 1))
        if case["b"] is not None:
            conv.bias.copy_(case["b"])
        if case["transform"] == "ln":
            ln = pg_nn.NCHWLayerNorm(cin, eps=case["eps"]).to(DEV)
            ln.weight.copy_(case["ln_w"])
            ln.bias.copy_(case["ln_b"])
    return conv, ln


def _run(case, grad_output=None, dense=False):
    """loss, the lse planes and the gradients of one forward + backward on the fused route (dense=True: .dense() + the dense
    kernels)."""
    from pytorch_generative_amd import ops

    conv, ln = _head(case)
    h = case["h"].to(DEV).requires_grad_(True)
    x = case["images"].to(DEV)
    deferred = ops.DeferredLogits(h, conv, in_act="relu" if case["transform"] == "relu" else None, pre_ln=ln)
    assert ops.linear_categorical_supported(h, conv, deferred.in_act, ln)
    loss = ops.categorical_nll_sum_mean(deferred.dense() if dense else deferred, x, case["k"])
    fused = type(loss.grad_fn).__name__.startswith("_LinearCategoricalNLL")
    assert fused != dense, f"took the {'fused' if fused else 'dense'} route"
    planes = loss.grad_fn.saved_tensors[2]
    (loss if grad_output is None else loss * grad_output).backward()
    torch.cuda.synchronize()
    grads = {"dh": h.grad, "dW": conv.weight.grad.view(conv.weight.shape[0], -1)}
    if conv.bias is not None:
        grads["db"] = conv.bias.grad
    if ln is not None:
        grads["dln_w"], grads["dln_b"] = ln.weight.grad, ln.bias.grad
    return loss.detach(), planes, grads, deferred


def _check(what, loss, planes, grads, want):
    lse = planes[0]
    print(f"[linear_categorical] {what}: loss {_util.rel_err(loss, want['loss']):.2e} lse {_util.rel_err(lse, want['lse']):.2e}")
    assert lse.shape == want["lse"].shape
    _util.assert_close(loss, want["loss"], 1e-5, f"{what} loss")
    _util.assert_close(lse, want["lse"], 1e-5, f"{what} lse")
    assert set(grads) == {g for g in GRADS if g in want}
    rep = _util.GradReport(f"linear_categorical {what}")
    for name, got in grads.items():
        assert got.shape == want[name].shape, name
        rep.add(name, got, want[name])
    rep.finish()


@pytest.mark.parametrize("shape,transform,variant,bias", CASES, ids=_id)
def test_op_parity_float64(shape, transform, variant, bias):
    from pytorch_generative_amd import ops

    case, want = _case(shape, transform, variant, bias)
    what = f"{shape} {transform} {variant} bias={bias}"
    loss, planes, grads, deferred = _run(case)
    assert planes.shape == (2,) + tuple(case["images"].shape)
    _check(what, loss, planes, grads, want)
    per_sample = ops.categorical_nll_per_sample(deferred, case["images"].to(DEV), case["k"])
    torch.cuda.synchronize()
    assert per_sample.shape == (shape[0],) and not per_sample.requires_grad
    print(f"[linear_categorical] {what}: per-sample {_util.rel_err(per_sample, want['per_sample']):.2e}")
    _util.assert_close(per_sample, want["per_sample"], 1e-5, f"{what} per-sample loss")


@pytest.mark.parametrize("shape,transform,variant,bias", CASES, ids=_id)
def test_lse_plus_residual(shape, transform, variant, bias):
    """lse + residual, the normaliser the backward uses, within 4e-6 absolute of the float64 lse: the bound
    tests/test_gpu_categorical.py derives for the dense kernels, whose logits are given.

    Here the logits are computed, and the float64 reference computes them exactly: their own rounding is part of the
    difference. For the plain and equal cases (|z| below 16) the fp32 rounding is a fraction of the bound. For the "wide" cases
    max|z| is 90-190, where one ulp of a logit is 7.6e-6 (64 <= |z| < 128) or 1.5e-5 (above): fp32 logits alone miss the
    bound there (6.4e-6 to 4.7e-5 measured), which is why the kernels evaluate the classes that carry the mass of such a
    sub-pixel once more in float64 (lc_z64 in csrc/linear_categorical.hip). With that, on an MI355X: wide cases at most
    2.1e-6, all other cases at most 2.6e-6."""
    case, want = _case(shape, transform, variant, bias)
    _, planes, _, _ = _run(case)
    err = float((planes[0].double().cpu() + planes[1].double().cpu() - want["lse"]).abs().max())
    print(f"[linear_categorical] {shape} {transform} {variant} bias={bias}: |lse + residual - float64| {err:.2e}")
    assert err <= 4e-6, f"lse + residual off by {err:.2e}"


@pytest.mark.parametrize("shape,transform", [(SHAPES[1], "none"), (SHAPES[2], "ln"), (SHAPES[3], "relu"), (SHAPES[5], "ln"),
                                             (SHAPES[8], "none"), (RECIPE, "ln")], ids=_id)
def test_bit_reproducible_and_scales_exactly(shape, transform):
    case, _ = _case(shape, transform, "plain", True)
    _, planes1, grads1, _ = _run(case)
    _, planes2, grads2, _ = _run(case)
    assert torch.equal(planes1, planes2)
    for name in grads1:
        assert torch.equal(grads1[name], grads2[name]), name
    _, _, half, _ = _run(case, grad_output=0.5)
    for name in grads1:
        assert torch.equal(half[name], grads1[name] * 0.5), name


@pytest.mark.parametrize("shape,transform", [(SHAPES[2], "relu"), (SHAPES[4], "ln"), (SHAPES[6], "none"), (SHAPES[4], "relu")],
                         ids=_id)
def test_fused_route_next_to_the_dense_route(shape, transform):
    case, want = _case(shape, transform, "plain", True)
    for dense in (False, True):
        loss, planes, grads, _ = _run(case, dense=dense)
        _check(f"{shape} {transform} {'dense' if dense else 'fused'} route", loss, planes, grads, want)


def test_memory_stays_below_half_the_logits():
    """One forward + backward at the recipe's shape: what it allocates on top stays below half the bytes of the logits tensor
    it replaces (64 * 256 * 784 * 4 = 51.4 MB) — the features' gradient (3.2 MB), the lse planes (0.4 MB) and the
    partial-row workspace, which the planner caps at a quarter of the logits (12.8 MB). A consequence of the design."""
    from pytorch_generative_amd import ops

    case, _ = _case(RECIPE, "ln", "plain", True)
    conv, ln = _head(case)
    h = case["h"].to(DEV).requires_grad_(True)
    x = case["images"].to(DEV)
    ops.categorical_nll_sum_mean(ops.DeferredLogits(h, conv, pre_ln=ln), x, 256).backward()  # parameters' .grad exist now
    torch.cuda.synchronize()
    h.grad = None
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    ops.categorical_nll_sum_mean(ops.DeferredLogits(h, conv, pre_ln=ln), x, 256).backward()
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - before
    logits_bytes = 64 * 256 * 784 * 4
    print(f"[linear_categorical] memory: peak rise {rise / 1e6:.1f} MB, logits {logits_bytes / 1e6:.1f} MB")
    assert rise < logits_bytes // 2


# ---- models -----------------------------------------------------------------------------------------------------------

K_MODEL = 8


def _build(name, sample_fn=None, seed=0):
    import pytorch_generative_amd as pg

    m = pg.models
    torch.manual_seed(seed)
    k = K_MODEL
    if name == "ImageGPT":
        model = m.ImageGPT(in_channels=1, out_channels=k, in_size=8, n_transformer_blocks=1, n_attention_heads=2,
                           n_embedding_channels=4, sample_fn=sample_fn)
    elif name == "ImageGPT16":  # the shape the fused block kernels take
        model = m.ImageGPT(in_channels=1, out_channels=k, in_size=8, n_transformer_blocks=2, n_attention_heads=4,
                           n_embedding_channels=16, sample_fn=sample_fn)
    elif name == "PixelCNN":
        model = m.PixelCNN(in_channels=1, out_channels=k, n_residual=1, residual_channels=4, head_channels=8, sample_fn=sample_fn)
    elif name == "GatedPixelCNN":
        model = m.GatedPixelCNN(in_channels=1, out_channels=k, n_gated=1, gated_channels=4, head_channels=8, sample_fn=sample_fn)
    else:
        model = m.PixelSNAIL(in_channels=1, out_channels=k, n_channels=8, n_pixel_snail_blocks=1, n_residual_blocks=1,
                             attention_key_channels=2, attention_value_channels=4, sample_fn=sample_fn)
    if name.startswith("ImageGPT"):
        with torch.no_grad():
            model._pos.normal_(0, 0.1)
    return model.to(DEV)


MODELS = ["ImageGPT", "ImageGPT16", "PixelCNN", "GatedPixelCNN", "PixelSNAIL"]


def _grey_batches(n_batches, n=16, seed=5):
    g = torch.Generator().manual_seed(seed)
    return [cref.to_level(torch.randint(0, K_MODEL, (n, 1, 8, 8), generator=g), K_MODEL) for _ in range(n_batches)]


def _loss_and_grads(model, x, defer):
    from pytorch_generative_amd import ops

    model.defer_head = defer
    model.zero_grad(set_to_none=True)
    preds = model(x)
    assert isinstance(preds, ops.DeferredLogits) == defer
    assert tuple(preds.shape) == (x.shape[0], K_MODEL, 8, 8)
    loss = ops.categorical_nll_sum_mean(preds, x, K_MODEL)
    if defer:
        assert type(loss.grad_fn).__name__.startswith("_LinearCategoricalNLL"), "the model's head did not take the fused route"
    loss.backward()
    torch.cuda.synchronize()
    # (a parameter no path reaches, such as the last layer's vertical stack, has no gradient on either route)
    return loss.detach(), {k: None if p.grad is None else p.grad.clone() for k, p in model.named_parameters()}


@pytest.mark.parametrize("name", MODELS)
def test_model_with_deferred_head_matches_dense(name):
    model = _build(name)
    x = _grey_batches(1)[0].to(DEV)
    want_loss, want = _loss_and_grads(model, x, False)
    loss, got = _loss_and_grads(model, x, True)
    _util.assert_close(loss, want_loss, 1e-5, f"{name} loss")
    rep = _util.GradReport(f"{name} defer_head")
    for k in want:
        assert (got[k] is None) == (want[k] is None), k
        if want[k] is not None:
            rep.add(k, got[k], want[k])
    rep.finish()
    # the dense tensor a DeferredLogits stands for is the model's own output
    model.defer_head = True
    with torch.no_grad():
        deferred = model(x)
        model.defer_head = False
        assert torch.equal(deferred.dense(), model(x))


@pytest.mark.parametrize("name", ["ImageGPT16", "PixelCNN"])
def test_graphed_steps_equal_eager_bitwise(name):
    from pytorch_generative_amd import graph, ops, optim, recipes

    was = ops.set_deterministic(True)
    try:
        loss3 = recipes.categorical_loss(K_MODEL)
        loss_fn = lambda x, preds: loss3(x, None, preds)  # noqa: E731
        xs = [x.to(DEV) for x in _grey_batches(3)]
        m1 = _build(name)
        m1.defer_head = True
        m2 = copy.deepcopy(m1)
        assert m2.defer_head is True
        o1, o2 = optim.FlatAdam(m1.parameters(), lr=1e-3), optim.FlatAdam(m2.parameters(), lr=1e-3)
        for x in xs:
            o1.zero_grad()
            preds = m1(x)
            assert isinstance(preds, ops.DeferredLogits)
            loss = loss_fn(x, preds)
            assert type(loss.grad_fn).__name__.startswith("_LinearCategoricalNLL")
            loss.backward()
            o1.step()
        step = graph.GraphedTrainStep(m2, o2, loss_fn, xs[0], preserve_state=True)
        for x in xs:
            step(x)
        torch.cuda.synchronize()
        before = _build(name)
        changed = False
        for (k, p1), (_, p2), (_, p0) in zip(m1.named_parameters(), m2.named_parameters(), before.named_parameters()):
            assert torch.equal(p1, p2), f"{k}: graph replay differs from eager steps"
            changed = changed or not torch.equal(p1, p0)
        assert changed, "three steps left every parameter as it was"
    finally:
        ops.set_deterministic(was)


def test_recipe_trains_one_epoch_with_deferred_head(tmp_path):
    from pytorch_generative_amd import recipes

    loader = [(x, torch.zeros(x.shape[0])) for x in _grey_batches(2)]
    t = recipes.run(lambda: _build("PixelCNN"), loaders=recipes.grey_mnist, loss_fn=recipes.categorical_loss(K_MODEL), lr=1e-3,
                    n_epochs=1, batch_size=16, log_dir=str(tmp_path), n_gpus=1, device_id=0, debug_loader=loader,
                    defer_head=True)
    assert t.model.defer_head is True
    assert t._epoch == 1 and t._step == 2
    assert all(bool(torch.isfinite(p).all()) for p in t.model.parameters())
    assert glob.glob(os.path.join(str(tmp_path), "trainer_state_1.ckpt")), os.listdir(str(tmp_path))
    assert all(v == v and abs(v) != float("inf") for v in t.last_eval_metrics.values()) and t.last_eval_metrics


@pytest.mark.parametrize("name", ["ImageGPT", "PixelCNN"])
def test_sample_sees_dense_logits(name):
    from pytorch_generative_amd import nn as pg_nn

    cond = torch.full((2, 1, 8, 8), -1.0)
    cond[:, :, :3, :] = cref.to_level(torch.randint(0, K_MODEL, (2, 1, 3, 8), generator=torch.Generator().manual_seed(1)), K_MODEL)
    canvases = []
    for defer in (False, True):
        sampler = pg_nn.CategoricalSampler(K_MODEL, generator=torch.Generator(device=DEV).manual_seed(77))
        model = _build(name, sample_fn=sampler).eval()
        model.defer_head = defer
        canvases.append(model.sample(conditioned_on=cond.to(DEV)).cpu())
        assert model.defer_head is defer, "sample() must leave the switch as it found it"
    assert torch.equal(canvases[0], canvases[1])
    assert bool(torch.isin(canvases[1], cref.levels(K_MODEL)).all())


def test_unsupported_head_takes_the_dense_route():
    """Cin = 6 is outside the kernels' domain: the same call runs .dense() and the dense loss kernels."""
    from pytorch_generative_amd import nn as pg_nn
    from pytorch_generative_amd import ops

    torch.manual_seed(3)
    conv = pg_nn.Conv2d(in_channels=6, out_channels=K_MODEL, kernel_size=1).to(DEV)
    h = torch.randn(4, 6, 8, 8, device=DEV, requires_grad=True)
    x = _grey_batches(1, n=4)[0].to(DEV)
    assert not ops.linear_categorical_supported(h, conv, "relu", None)
    deferred = ops.DeferredLogits(h, conv, in_act="relu")
    loss = ops.categorical_nll_sum_mean(deferred, x, K_MODEL)
    assert type(loss.grad_fn).__name__.startswith("_CategoricalNLLSumMean")
    want = ops.categorical_nll_sum_mean(conv(h, in_act="relu"), x, K_MODEL)
    assert torch.equal(loss, want)
    loss.backward()
    assert h.grad is not None and conv.weight.grad is not None
    per_sample = ops.categorical_nll_per_sample(deferred, x, K_MODEL)
    assert torch.equal(per_sample, ops.categorical_nll_per_sample(conv(h, in_act="relu").detach(), x, K_MODEL))
