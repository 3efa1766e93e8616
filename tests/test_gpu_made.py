"""GPU: MaskedLinear / MADE on the masked-GEMM kernels (csrc/masked_linear.hip) — op parity against a float64 restatement
(forward, data gradient, the unmasked weight / bias gradients) over ragged shapes, N = 1 .. 1100 and the recipe's
784 -> 8000 -> 784; the model against the reference fixture (tests/golden/made/cases.pt) over 3 steps with mask rotation,
with FlatAdam and with torch.optim.Adam; graph replay; bit reproducibility; sample(); reproduce()."""

import copy
import os

import pytest
import torch

import _util

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
CASES = os.path.join(_util.GOLDEN_DIR, "made", "cases.pt")
LR = 1e-3


def load_cases():
    return torch.load(CASES, map_location="cpu", weights_only=False)["cases"]


def made_mod():
    from pytorch_generative_amd.models.autoregressive import made

    return made


def _degrees(in_f, out_f, g):
    deg_in = torch.randint(0, 7, (in_f,), generator=g, dtype=torch.int32)
    deg_out = torch.randint(0, 7, (out_f,), generator=g, dtype=torch.int32)
    return deg_in, deg_out


def _mask(deg_in, deg_out, strict):
    return ((deg_in[None, :] < deg_out[:, None]) if strict else (deg_in[None, :] <= deg_out[:, None])).float()


# (N, in, out, masked, strict, bias)
OP_SHAPES = [
    (1, 1, 1, True, False, True), (1, 3, 17, True, True, True), (3, 17, 33, True, False, True),
    (17, 33, 255, True, True, False), (64, 255, 3, True, False, True), (64, 784, 8000, True, False, True),
    (64, 8000, 784, True, True, True), (1024, 33, 17, True, False, True), (1100, 255, 33, False, False, True),
    (65, 100, 129, True, True, False),
]


@pytest.mark.parametrize("n,in_f,out_f,masked,strict,bias", OP_SHAPES)
def test_op_parity_float64(n, in_f, out_f, masked, strict, bias):
    from pytorch_generative_amd import ops

    g = torch.Generator().manual_seed(n * 7919 + in_f * 31 + out_f)
    x = torch.randn(n, in_f, generator=g)
    w = torch.randn(out_f, in_f, generator=g) / in_f ** 0.5
    b = torch.randn(out_f, generator=g) if bias else None
    dy = torch.randn(n, out_f, generator=g)
    deg_in, deg_out = _degrees(in_f, out_f, g) if masked else (None, None)
    m = _mask(deg_in, deg_out, strict) if masked else torch.ones(out_f, in_f)

    xg = x.to(DEV).requires_grad_(True)
    wg = w.to(DEV).requires_grad_(True)
    bg = b.to(DEV).requires_grad_(True) if bias else None
    y = ops.masked_linear(xg, wg, bg, None if deg_in is None else deg_in.to(DEV),
                          None if deg_out is None else deg_out.to(DEV), strict)
    y.backward(dy.to(DEV))
    torch.cuda.synchronize()

    wm = w.double() * m.double()
    want_y = x.double() @ wm.t() + (b.double() if bias else 0)
    _util.assert_close(y, want_y, 1e-5, f"forward {n}x{in_f}->{out_f}")
    rep = _util.GradReport(f"masked_linear {n}x{in_f}->{out_f}")
    rep.add("dx", xg.grad, dy.double() @ wm)
    rep.add("dw (unmasked)", wg.grad, dy.double().t() @ x.double())
    if bias:
        rep.add("db", bg.grad, dy.double().sum(0))
    rep.finish()
    # the in-place masking: weight == W o M bit for bit (W * 1 = W, W * 0 = +-0 as torch's `weight.data *= mask`)
    assert torch.equal(wg.detach().cpu(), w * m)
    if masked and bool((m == 0).any()):
        assert float(wg.grad.cpu()[m == 0].abs().max()) > 0, "the weight gradient must not be masked"


def test_relu_chain_float64():
    """Three layers with the ReLU fused into the epilogues and its derivative into the next data gradient."""
    from pytorch_generative_amd import ops

    g = torch.Generator().manual_seed(3)
    dims = [37, 70, 19, 37]
    x = torch.randn(50, dims[0], generator=g)
    ws = [torch.randn(dims[i + 1], dims[i], generator=g) / dims[i] ** 0.5 for i in range(3)]
    bs = [torch.randn(dims[i + 1], generator=g) * 0.1 for i in range(3)]
    degs = [torch.randint(0, 9, (d,), generator=g, dtype=torch.int32) for d in dims]
    dy = torch.randn(50, dims[-1], generator=g)
    xg = x.to(DEV).requires_grad_(True)
    wg = [w.to(DEV).requires_grad_(True) for w in ws]
    bg = [b.to(DEV).requires_grad_(True) for b in bs]
    dd = [d.to(DEV) for d in degs]
    y = ops.masked_mlp(xg, [(wg[i], bg[i], dd[i], dd[i + 1], i == 2) for i in range(3)])
    y.backward(dy.to(DEV))

    xr = x.double().requires_grad_(True)
    wr = [w.double().requires_grad_(True) for w in ws]
    br = [b.double().requires_grad_(True) for b in bs]
    h = xr
    for i in range(3):
        h = h @ (wr[i] * _mask(degs[i], degs[i + 1], i == 2).double()).t() + br[i]
        if i < 2:
            h = torch.relu(h)
    h.backward(dy.double())
    _util.assert_close(y, h.detach(), 1e-5, "relu chain forward")
    # the masks act outside autograd, so the reference's (unmasked) weight gradient is dY_i^T X_i: rebuild it from the float64 activations
    acts, h = [x.double()], x.double()
    for i in range(3):
        z = h @ (ws[i].double() * _mask(degs[i], degs[i + 1], i == 2).double()).t() + bs[i].double()
        h = torch.relu(z) if i < 2 else z
        acts.append(h)
    gz = dy.double()
    rep = _util.GradReport("relu chain (unmasked wgrad)")
    for i in reversed(range(3)):
        rep.add(f"dw{i}", wg[i].grad, gz.t() @ acts[i])
        rep.add(f"db{i}", bg[i].grad, gz.sum(0))
        gz = (gz @ (ws[i].double() * _mask(degs[i], degs[i + 1], i == 2).double())) * (acts[i] > 0)
    rep.add("dx", xg.grad, xr.grad)
    rep.finish()


def _model_from_case(case, sample_fn=None):
    made = made_mod()
    model = made.MADE(sample_fn=sample_fn, **case["kwargs"])
    model.load_state_dict(case["state"], strict=True)
    return model.to(DEV)


def _post_adam_ok(name, got, want, grad_ref):
    """post-Adam parameters 1e-4 relative above the gradient noise floor; below it Adam's first steps
    are +-lr * sign(round-off) in the reference too, so the difference is only bounded by the steps taken."""
    got, want, gref = got.detach().double().cpu(), want.double(), grad_ref.double()
    above = gref.abs() > 1e-5 * float(gref.abs().max())
    d = (got - want).abs()
    if bool(above.any()):
        assert float(d[above].max()) <= 1e-4 * float(want.abs().max()) + 1e-7, name
    assert float(d.max()) <= 2 * 3 * LR + 1e-6, name


@pytest.mark.parametrize("optimizer", ["flat_adam", "torch_adam"])
@pytest.mark.parametrize("name", sorted(load_cases()))
def test_model_parity_with_fixture(name, optimizer):
    from pytorch_generative_amd import ops, optim

    case = load_cases()[name]
    model = _model_from_case(case)
    opt = optim.FlatAdam(model.parameters(), lr=LR) if optimizer == "flat_adam" else \
        torch.optim.Adam(model.parameters(), lr=LR)
    x = case["x"].to(DEV)
    layers = [m for m in model._net if isinstance(m, made_mod().MaskedLinear)]
    for i, step in enumerate(case["steps"]):
        before = {k: p.detach().clone() for k, p in model.named_parameters()}
        opt.zero_grad()
        logits = model(x)
        loss = ops.bce_with_logits_sum_mean(logits, x)
        loss.backward()
        torch.cuda.synchronize()
        what = f"{name} step {i}"
        assert logits.shape == x.shape
        _util.assert_close(logits, step["logits"], 1e-4, f"{what} logits")
        _util.assert_close(loss, step["loss"], 1e-4, f"{what} loss")
        for layer, m in zip(layers, step["masks"]):
            assert torch.equal(layer.mask.cpu(), m.float()), f"{what}: mask buffer"
        rep = _util.GradReport(what)
        named = dict(model.named_parameters())
        for k, want in step["grads"].items():
            rep.add(k, named[k].grad, want)
        rep.finish()
        for k, want in step["masked_weights"].items():
            m = step["masks"][int(k.split(".")[1]) // 2].float()
            # the forward's in-place masking, bit for bit, of this model's own weights
            assert torch.equal(named[k].detach().cpu(), before[k].cpu() * m), f"{what}: {k} != W o M"
            _util.assert_close(named[k], want, 1e-4, f"{what} {k} masked weight")
            if bool((m == 0).any()):
                assert float(named[k].grad.cpu()[m == 0].abs().max()) > 0, f"{what}: {k} grad is masked"
        opt.step()
        torch.cuda.synchronize()
        for k, want in step["params_after_adam"].items():
            _post_adam_ok(f"{what} {k} after Adam", named[k], want, step["grads"][k])
    assert model._mask_seed == len(case["steps"])


def _recipe_like(n_masks=1, seed=0, d=64, hidden=(96,)):
    torch.manual_seed(seed)
    return made_mod().MADE(d, list(hidden), n_masks=n_masks).to(DEV)


def test_graphed_steps_equal_eager_bitwise():
    from pytorch_generative_amd import graph, ops, optim

    loss_fn = lambda x, preds: ops.bce_with_logits_sum_mean(preds, x)  # noqa: E731
    g = torch.Generator().manual_seed(5)
    xs = [torch.bernoulli(torch.full((64, 1, 8, 8), 0.3), generator=g).to(DEV) for _ in range(4)]
    m1 = _recipe_like()
    m2 = copy.deepcopy(m1)
    o1, o2 = optim.FlatAdam(m1.parameters(), lr=LR), optim.FlatAdam(m2.parameters(), lr=LR)
    for x in xs:
        o1.zero_grad()
        loss_fn(x, m1(x)).backward()
        o1.step()
    step = graph.GraphedTrainStep(m2, o2, loss_fn, xs[0], preserve_state=True)
    for x in xs:
        step(x)
    torch.cuda.synchronize()
    for (k, p1), (_, p2) in zip(m1.named_parameters(), m2.named_parameters()):
        assert torch.equal(p1, p2), f"{k}: graph replay differs from eager steps"
    for (k, b1), (_, b2) in zip(m1.named_buffers(), m2.named_buffers()):
        assert torch.equal(b1, b2), k


def test_n_masks_above_one_refuses_capture_and_trains_eagerly(tmp_path):
    from pytorch_generative_amd import graph, ops, optim, trainer

    loss_fn = lambda x, _, preds: ops.bce_with_logits_sum_mean(preds, x)  # noqa: E731
    model = _recipe_like(n_masks=3)
    opt = optim.FlatAdam(model.parameters(), lr=LR)
    x = torch.bernoulli(torch.full((16, 1, 8, 8), 0.3)).to(DEV)
    seed0 = model._mask_seed
    with pytest.raises(RuntimeError, match="n_masks"):
        graph.GraphedTrainStep(model, opt, lambda xx, preds: loss_fn(xx, None, preds), x, warmup_iters=0)
    torch.cuda.synchronize()
    assert model._mask_seed == seed0, "a refused capture must not advance the mask"

    torch.manual_seed(1)
    ref = _recipe_like(n_masks=3, seed=2)
    model = copy.deepcopy(ref)
    loader = [(torch.bernoulli(torch.full((16, 1, 8, 8), 0.3)), torch.zeros(16)) for _ in range(3)]
    opt = optim.FlatAdam(model.parameters(), lr=LR)
    t = trainer.Trainer(model=model, loss_fn=loss_fn, optimizer=opt, train_loader=loader, eval_loader=loader[:1],
                        log_dir=str(tmp_path))
    with pytest.warns(UserWarning, match="n_masks=3"):
        t._train_epoch()  # the training steps only (evaluation and sampling mask the weights with further masks)
    assert not t._use_graph and t._step == 3
    # the same steps by hand: one mask per forward, the reference's rotation
    ro = optim.FlatAdam(ref.parameters(), lr=LR)
    for xb, _ in loader:
        ro.zero_grad()
        xb = xb.to(DEV)
        ops.bce_with_logits_sum_mean(ref(xb), xb).backward()
        ro.step()
    for (k, p1), (_, p2) in zip(ref.named_parameters(), model.named_parameters()):
        assert torch.equal(p1, p2), k
    assert model._mask_seed == ref._mask_seed == 3


def test_step_is_bit_reproducible():
    from pytorch_generative_amd import ops

    x = torch.bernoulli(torch.full((1024, 64), 0.3)).to(DEV)
    grads = []
    for _ in range(2):
        model = _recipe_like(hidden=(300, 77))
        ops.bce_with_logits_sum_mean(model(x), x).backward()
        torch.cuda.synchronize()
        grads.append([p.grad.clone() for p in model.parameters()] + [model(x).detach()])
    for a, b in zip(*grads):
        assert torch.equal(a, b)


@pytest.mark.parametrize("name", sorted(load_cases()))
def test_sample_matches_fixture(name):
    case = load_cases()[name]
    model = made_mod().MADE(sample_fn=lambda l: (l > 0).float(), **case["kwargs"])
    model.load_state_dict(case["sample_state"], strict=True)
    model = model.to(DEV)
    model._mask_seed = case["sample_mask_seed"]
    cond = case["conditioned_on"].to(DEV)
    got = model.sample(conditioned_on=cond)
    assert torch.equal(got.cpu(), case["sample"])
    given = case["conditioned_on"] >= 0
    assert torch.equal(got.cpu()[given], case["conditioned_on"][given])
    assert torch.equal(cond.cpu(), case["conditioned_on"]), "conditioned_on must not be modified"
    assert model._mask_seed == case["sample_mask_seed"] + 1


def test_reproduce_debug_loader(tmp_path):
    from pytorch_generative_amd.models.autoregressive import made

    class _Loader:
        def __iter__(self):
            g = torch.Generator().manual_seed(0)
            return iter([(torch.bernoulli(torch.full((8, 1, 28, 28), 0.2), generator=g), torch.zeros(8))
                         for _ in range(2)])

    t = made.reproduce(n_epochs=1, log_dir=str(tmp_path), debug_loader=_Loader())
    assert t._epoch == 1 and t._step == 2 and t._use_graph
    assert all(torch.isfinite(p).all() for p in t.model.parameters())
    assert isinstance(t.model, made.MADE) and t.model._dims == [784, 8000, 784]
