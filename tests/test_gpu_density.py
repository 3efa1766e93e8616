"""GPU: KDE and the Gaussian / Bernoulli mixture models on the streaming log-density kernels (csrc/density.hip) — op
parity against a float64 restatement from explicit differences (ragged shapes, N = 1 .. 1100, K = 1 .. 300, F = 1 .. 784,
the split-K KDE), the models against the reference fixture (tests/golden/density/cases.pt: the reference's mixtures run in float64,
see make_density_golden.py for why) over 3 Adam steps with FlatAdam and torch.optim.Adam, edge behaviour, graph replay, bit reproducibility, sample() and the memory bound."""

import copy
import math
import os

import numpy as np
import pytest
import torch

import _util

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
CASES = os.path.join(_util.GOLDEN_DIR, "density", "cases.pt")
LR = 1e-3  # torch.optim.Adam's default, what the fixture used


def load_cases():
    return torch.load(CASES, map_location="cpu", weights_only=False)


def mods():
    from pytorch_generative_amd.models import kde, mixture_models

    return kde, mixture_models


# ---- float64 restatements (chunked: never more than ~16 M elements of (rows, K, F) at once) -------------------------------

def _row_chunks(n, k, f):
    step = max(1, min(n, (1 << 24) // max(1, k * f)))
    return [(i, min(n, i + step)) for i in range(0, n, step)]


def mixture_truth(kind, x, g, logits, *params):
    """(lse, [d logits, d params...]) of sum_n g[n] lse[n] in float64, the reference's formulas on explicit (n, K, F)
    broadcasts."""
    x, g = x.double(), g.double()
    leaves = [p.double().clone().requires_grad_(True) for p in (logits, *params)]
    out = []
    for a, b in _row_chunks(x.shape[0], params[0].shape[0], x.shape[1]):
        xc = x[a:b, None, :]
        if kind == "gaussian":
            mean, log_std = leaves[1], leaves[2]
            comp = (-log_std - 0.5 * math.log(2 * math.pi) - 0.5 * ((xc - mean) / log_std.exp()) ** 2).sum(-1)
        else:
            lg = leaves[1]
            comp = (xc * lg - torch.nn.functional.softplus(lg)).sum(-1)
        lse = torch.logsumexp(torch.log_softmax(leaves[0], -1) + comp, dim=-1)
        (lse * g[a:b]).sum().backward()
        out.append(lse.detach())
    return torch.cat(out), [p.grad for p in leaves]


def kde_gaussian_truth(test, train, h):
    test, train = test.double(), train.double()
    n, d = train.shape
    z = 0.5 * d * math.log(2 * math.pi) + d * math.log(h) + math.log(n)
    out = []
    for a, b in _row_chunks(test.shape[0], n, d):
        diffs = (test[a:b, None, :] - train[None, :, :]) / h
        out.append(torch.logsumexp(-0.5 * (diffs ** 2).sum(-1) - z, dim=-1))
    return torch.cat(out)


def _mixture_inputs(kind, n, k, f, mode, seed):
    g = torch.Generator().manual_seed(seed)
    if mode == "init":  # the reference's initialisers: every component nearly the same, responsibilities all mixed
        logits = torch.ones(k)
        params = (torch.randn(k, f, generator=g) * 0.01, torch.zeros(k, f)) if kind == "gaussian" else \
            (torch.rand(k, f, generator=g),)
        x = torch.randn(n, f, generator=g) if kind == "gaussian" else torch.bernoulli(torch.full((n, f), 0.4), generator=g)
    elif mode == "clustered":  # data around well separated centres far from 0: the expanded quadratic cancels
        logits = torch.randn(k, generator=g)
        centres = 3 * torch.randn(k, f, generator=g)
        x = centres[torch.randint(0, k, (n,), generator=g)] + 0.5 * torch.randn(n, f, generator=g)
        params = (centres + 0.1 * torch.randn(k, f, generator=g), math.log(0.5) + 0.1 * torch.randn(k, f, generator=g))
    else:  # "spread"
        logits = torch.randn(k, generator=g)
        if kind == "gaussian":
            params = (0.5 * torch.randn(k, f, generator=g), 0.3 * torch.randn(k, f, generator=g))
            x = torch.randn(n, f, generator=g)
        else:
            params = (torch.randn(k, f, generator=g),)
            x = torch.bernoulli(torch.full((n, f), 0.4), generator=g) if seed % 2 else torch.rand(n, f, generator=g)
    gup = torch.randn(n, generator=g)
    return x, gup, logits, params


# (kind, N, K, F, mode)
MIXTURE_SHAPES = [
    ("gaussian", 1, 1, 1, "spread"), ("bernoulli", 1, 1, 1, "spread"),
    ("gaussian", 3, 2, 5, "spread"), ("bernoulli", 3, 2, 5, "spread"),
    ("gaussian", 17, 3, 33, "spread"), ("bernoulli", 17, 3, 33, "spread"),
    ("gaussian", 65, 33, 100, "spread"), ("bernoulli", 65, 33, 100, "spread"),
    ("gaussian", 1100, 5, 64, "spread"), ("bernoulli", 1100, 5, 64, "spread"),
    ("gaussian", 200, 300, 50, "spread"), ("bernoulli", 200, 300, 50, "spread"),       # K > 128: ten column tiles
    ("gaussian", 130, 129, 784, "spread"), ("bernoulli", 130, 129, 784, "spread"),
    ("gaussian", 64, 7, 784, "init"), ("bernoulli", 64, 7, 784, "init"),
    ("gaussian", 1024, 10, 784, "init"), ("bernoulli", 1024, 10, 784, "init"),
    ("gaussian", 257, 3, 5, "clustered"), ("gaussian", 300, 40, 64, "clustered"),
]


@pytest.mark.parametrize("kind,n,k,f,mode", MIXTURE_SHAPES)
def test_mixture_op_parity_float64(kind, n, k, f, mode):
    from pytorch_generative_amd import ops

    x, gup, logits, params = _mixture_inputs(kind, n, k, f, mode, seed=n * 7919 + k * 31 + f)
    leaves = [p.to(DEV).requires_grad_(True) for p in (logits, *params)]
    lse = ops.mixture_log_prob(kind, x.to(DEV), *leaves)
    lse.backward(gup.to(DEV))
    torch.cuda.synchronize()
    want, want_grads = mixture_truth(kind, x, gup, logits, *params)
    what = f"{kind} {mode} {n}x{k}x{f}"
    assert lse.shape == (n,)
    print(f"[density] {what}: forward rel err {_util.rel_err(lse, want):.3e}")
    _util.assert_close(lse, want, 1e-4, f"{what} lse")
    rep = _util.GradReport(what)
    names = ("mixture_logits", "mean", "log_std") if kind == "gaussian" else ("mixture_logits", "logits")
    for name, leaf, wg in zip(names, leaves, want_grads):
        rep.add(name, leaf.grad, wg)
    rep.finish()


# (M test, N train, d, bandwidth, data)
KDE_SHAPES = [
    (1, 1, 1, 0.5, "uniform"), (7, 40, 3, 0.1, "uniform"), (33, 129, 17, 0.3, "uniform"),
    (1100, 300, 64, 0.1, "uniform"), (65, 1000, 784, 0.2, "sparse"),
    (48, 20000, 784, 0.2, "sparse"),  # few row tiles, 625 column tiles: the split-K merge
    (5, 4097, 2, 1.0, "uniform"),
]


def _kde_inputs(m, n, d, data, seed):
    g = torch.Generator().manual_seed(seed)
    if data == "sparse":  # MNIST-like: most entries 0, the rest in [0, 1]
        draw = lambda r: torch.rand(r, d, generator=g) * (torch.rand(r, d, generator=g) < 0.2)  # noqa: E731
    else:
        draw = lambda r: torch.rand(r, d, generator=g)  # noqa: E731
    return draw(m), draw(n)


@pytest.mark.parametrize("m,n,d,h,data", KDE_SHAPES)
def test_kde_gaussian_parity_float64(lib, m, n, d, h, data):
    from pytorch_generative_amd import ops

    test, train = _kde_inputs(m, n, d, data, seed=m * 131 + n * 7 + d)
    if n == 20000:
        assert lib.pg_kde_workspace_floats(m, n, d) > n + 4, "this shape must exercise the split-K merge"
    got = ops.kde_gaussian(test.to(DEV), train.to(DEV), h)
    torch.cuda.synchronize()
    want = kde_gaussian_truth(test, train, h)
    print(f"[density] kde {m}x{n}x{d} h={h}: rel err {_util.rel_err(got, want):.3e}")
    assert got.shape == (m,)
    _util.assert_close(got, want, 1e-4, f"kde_gaussian {m}x{n}x{d}")


# ---- the models against the reference fixture --------------------------------------------------------------------------

def _post_adam_ok(name, got, want, grad_ref):
    """DESIGN.md §2, as tests/test_gpu_made.py: post-Adam parameters 1e-4 relative above the gradient noise floor; below
    it Adam's first steps are +-lr * sign(round-off) in the reference too, so the difference is only bounded by the
    steps taken."""
    got, want, gref = got.detach().double().cpu(), want.double(), grad_ref.double()
    above = gref.abs() > 1e-5 * float(gref.abs().max())
    d = (got - want).abs()
    if bool(above.any()):
        assert float(d[above].max()) <= 1e-4 * float(want.abs().max()) + 1e-7, name
    assert float(d.max()) <= 2 * 3 * LR + 1e-6, name


@pytest.mark.parametrize("optimizer", ["flat_adam", "torch_adam"])
@pytest.mark.parametrize("name", sorted(load_cases()["mixtures"]))
def test_model_parity_with_fixture(name, optimizer):
    from pytorch_generative_amd import optim

    _, mm = mods()
    case = load_cases()["mixtures"][name]
    model = getattr(mm, case["cls"])(**case["kwargs"])
    model.load_state_dict(case["state"], strict=True)
    model = model.to(DEV)
    opt = optim.FlatAdam(model.parameters(), lr=LR) if optimizer == "flat_adam" else \
        torch.optim.Adam(model.parameters(), lr=LR)
    x = case["x"].to(DEV)
    n = x.shape[0]
    for i, step in enumerate(case["steps"]):
        opt.zero_grad()
        out = model(x)
        loss = -out.mean()
        loss.backward()
        torch.cuda.synchronize()
        what = f"{name} step {i}"
        assert out.shape == ((n, 1) if case["cls"] == "GaussianMixtureModel" else (n,)) == step["out"].shape
        assert model._original_shape == x.shape
        _util.assert_close(out, step["out"], 1e-4, f"{what} output")
        _util.assert_close(loss, step["loss"], 1e-4, f"{what} loss")
        named = dict(model.named_parameters())
        rep = _util.GradReport(what)
        for k, want in step["grads"].items():
            rep.add(k, named[k].grad, want)
        rep.finish()
        opt.step()
        torch.cuda.synchronize()
        for k, want in step["params_after_adam"].items():
            _post_adam_ok(f"{what} {k} after Adam", named[k], want, step["grads"][k])


@pytest.mark.parametrize("d", sorted(load_cases()["kde"]))
def test_kde_matches_fixture(d):
    kde, _ = mods()
    cases = load_cases()
    case = cases["kde"][d]
    train, test = case["train"].to(DEV), case["test"].to(DEV)
    saw_minus_inf = False
    for h in cases["bandwidths"]:
        got = kde.KernelDensityEstimator(train, kde.GaussianKernel(bandwidth=h))(test)
        assert got.shape == (test.shape[0],)
        _util.assert_close(got, case["gaussian"][h], 1e-4, f"gaussian kde d={d} h={h}")
        got = kde.KernelDensityEstimator(train, kde.ParzenWindowKernel(bandwidth=h))(test).cpu()
        want = case["parzen"][h]
        print(f"[density] parzen d={d} h={h}: got {got.tolist()}")
        nan, inf = torch.isnan(want), torch.isinf(want)
        assert torch.equal(torch.isnan(got), nan), f"parzen d={d} h={h}: NaN where the reference has NaN only"
        assert torch.equal(got[inf], want[inf]), f"parzen d={d} h={h}: -inf where the reference has -inf"
        fin = ~(nan | inf)
        assert bool(((got[fin] - want[fin]).abs() <= 1e-6 * want[fin].abs()).all()), f"parzen d={d} h={h}"
        saw_minus_inf |= bool((want == -math.inf).any())
    assert saw_minus_inf, "the fixture must hold a test row that no window contains"


# ---- edge behaviour ----------------------------------------------------------------------------------------------------

def test_all_minus_inf_rows_give_minus_inf():
    from pytorch_generative_amd import ops

    g = torch.Generator().manual_seed(1)
    for k in (3, 300):  # 300: the column tiles are split across workgroups and merged
        x = torch.bernoulli(torch.full((5, 20), 0.5), generator=g).to(DEV)
        logits = torch.randn(k, 20, generator=g).to(DEV)
        mix = torch.full((k,), -math.inf, device=DEV)
        out = ops.mixture_log_prob("bernoulli", x, mix, logits)
        assert bool((out == -math.inf).all()), out
        # some components switched off (whole column tiles of them at k = 300): as if they were not there
        mix = torch.randn(k, generator=g)
        mix[: (2 * k) // 3] = -math.inf
        out = ops.mixture_log_prob("bernoulli", x, mix.to(DEV), logits)
        keep = (2 * k) // 3
        want, _ = mixture_truth("bernoulli", x.cpu(), torch.zeros(5), mix[keep:], logits.cpu()[keep:])
        _util.assert_close(out, want, 1e-4, f"partly -inf mixture_logits, K = {k}")


def test_parzen_count_zero_gives_minus_inf():
    from pytorch_generative_amd import ops

    train = torch.zeros(300, 4, device=DEV)
    test = torch.tensor([[0.1, 0.1, 0.1, 0.1], [0.1, 0.1, 0.1, 0.6], [9.0, 0.0, 0.0, 0.0]], device=DEV)
    got = ops.kde_parzen(test, train, 1.0).cpu()
    assert got[0] == 0.0 and got[1] == -math.inf and got[2] == -math.inf
    # coef = 1 / h**d overflows fp32: the reference's NaN (and +inf when every window contains the row); no crash
    train = torch.zeros(10, 784, device=DEV)
    test = torch.zeros(2, 784, device=DEV)
    test[1, 5] = 1.0
    got = ops.kde_parzen(test, train, 0.1).cpu()
    assert got[0] == math.inf and math.isnan(float(got[1]))


def test_input_gradient_raises():
    from pytorch_generative_amd import ops

    _, mm = mods()
    x = torch.zeros(4, 6, device=DEV, requires_grad=True)
    with pytest.raises(RuntimeError, match="gradient with respect to x"):
        mm.GaussianMixtureModel(2, 6).to(DEV)(x)
    with pytest.raises(RuntimeError, match="gradient with respect to x"):
        ops.mixture_log_prob("bernoulli", x, torch.zeros(2, device=DEV), torch.zeros(2, 6, device=DEV))
    with pytest.raises(RuntimeError, match="no gradient"):
        ops.kde_gaussian(x, torch.zeros(3, 6, device=DEV), 1.0)


@pytest.mark.parametrize("kind", ["gaussian", "bernoulli"])
def test_single_component(kind):
    """K = 1: lse is the component's log-probability and the mixture_logits gradient is 0 within the floor."""
    from pytorch_generative_amd import ops

    x, gup, _, params = _mixture_inputs(kind, 70, 1, 40, "spread", seed=11)
    mix = torch.tensor([0.7], device=DEV, requires_grad=True)
    leaves = [p.to(DEV).requires_grad_(True) for p in params]
    out = ops.mixture_log_prob(kind, x.to(DEV), mix, *leaves)
    out.backward(gup.to(DEV))
    x64 = x.double()
    if kind == "gaussian":
        mean, log_std = (p.double() for p in params)
        want = (-log_std - 0.5 * math.log(2 * math.pi) - 0.5 * ((x64 - mean) / log_std.exp()) ** 2).sum(-1)
    else:
        lg = params[0].double()
        want = (x64 * lg - torch.nn.functional.softplus(lg)).sum(-1)
    _util.assert_close(out, want, 1e-4, f"{kind} K = 1")
    scale = max(float(p.grad.abs().max()) for p in leaves)
    assert float(mix.grad.abs().max()) <= _util.GRAD_FLOOR * scale, mix.grad


# ---- graph replay, reproducibility -------------------------------------------------------------------------------------

def _train_model(kind, seed=0, k=5, f=64):
    _, mm = mods()
    torch.manual_seed(seed)
    cls = mm.GaussianMixtureModel if kind == "gaussian" else mm.BernoulliMixtureModel
    return cls(k, f).to(DEV)


def _batches(kind, count, n=96, shape=(1, 8, 8)):
    g = torch.Generator().manual_seed(5)
    if kind == "gaussian":
        return [torch.randn((n,) + shape, generator=g).to(DEV) for _ in range(count)]
    return [torch.bernoulli(torch.full((n,) + shape, 0.3), generator=g).to(DEV) for _ in range(count)]


@pytest.mark.parametrize("kind", ["gaussian", "bernoulli"])
def test_graphed_steps_equal_eager(kind):
    from pytorch_generative_amd import graph, optim

    loss_fn = lambda x, preds: -preds.mean()  # noqa: E731
    xs = _batches(kind, 4)
    m1 = _train_model(kind)
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
        assert not torch.equal(p1.cpu(), dict(_train_model(kind).named_parameters())[k].cpu()), f"{k} did not train"
        _util.assert_close(p2, p1, 1e-5, f"{kind} {k}: 4 replays vs 4 eager steps")


@pytest.mark.parametrize("kind", ["gaussian", "bernoulli"])
def test_forward_backward_bit_reproducible(kind):
    """No atomics in the forward, the split-K merge or the backward's row-range sums: two runs agree bit for bit."""
    from pytorch_generative_amd import ops

    x, gup, logits, params = _mixture_inputs(kind, 1100, 140, 300, "spread", seed=3)
    runs = []
    for _ in range(2):
        leaves = [p.to(DEV).requires_grad_(True) for p in (logits, *params)]
        out = ops.mixture_log_prob(kind, x.to(DEV), *leaves)
        out.backward(gup.to(DEV))
        torch.cuda.synchronize()
        runs.append([out.detach().clone()] + [p.grad.clone() for p in leaves])
    for a, b in zip(*runs):
        assert torch.equal(a, b)
    test, train = _kde_inputs(50, 5000, 32, "uniform", seed=4)
    a = ops.kde_gaussian(test.to(DEV), train.to(DEV), 0.3)
    b = ops.kde_gaussian(test.to(DEV), train.to(DEV), 0.3)
    assert torch.equal(a, b)


# ---- sample() ----------------------------------------------------------------------------------------------------------

def test_mixture_sample_shapes():
    _, mm = mods()
    for cls, shape in ((mm.GaussianMixtureModel, (4, 3, 8, 8)), (mm.BernoulliMixtureModel, (4, 3, 8, 8)),
                       (mm.GaussianMixtureModel, (4, 192)), (mm.BernoulliMixtureModel, (4, 192))):
        model = cls(n_components=5, n_features=192).to(DEV)
        model(torch.rand(shape, device=DEV))
        s = model.sample(7)
        assert s.shape == (7,) + shape[1:] and s.is_cuda and bool(torch.isfinite(s).all())
        if cls is mm.BernoulliMixtureModel:
            assert bool(((s == 0) | (s == 1)).all())


def test_kde_sample_shapes():
    kde, _ = mods()
    train = torch.rand(30, 6, device=DEV)
    for kernel in (kde.GaussianKernel(bandwidth=0.2), kde.ParzenWindowKernel(bandwidth=0.2), None):
        s = kde.KernelDensityEstimator(train, kernel).sample(9)
        assert s.shape == (9, 6) and s.is_cuda
    # Parzen noise stays inside the window of the row it was drawn around
    s = kde.KernelDensityEstimator(train[:1], kde.ParzenWindowKernel(bandwidth=0.2)).sample(50)
    assert float((s - train[:1]).abs().max()) <= 0.1 + 1e-6


def test_gaussian_kde_integrates_to_one():
    """The reference's own KDE test: 100 training points, a 2-D grid over [-8, 8) at 0.1 spacing."""
    kde, _ = mods()
    torch.manual_seed(0)
    train = torch.randn(100, 2).to(DEV)
    model = kde.KernelDensityEstimator(train)
    ticks = torch.arange(-8, 8, 0.1)
    xs, ys = torch.meshgrid(ticks, ticks, indexing="ij")
    grid = torch.stack([xs.reshape(-1), ys.reshape(-1)], dim=1).to(DEV)
    total = (model(grid).exp() * 0.01).sum()
    torch.testing.assert_close(total.cpu(), torch.tensor(1.0))


# ---- memory ------------------------------------------------------------------------------------------------------------

def test_kde_memory_is_inputs_outputs_and_workspace(lib, monkeypatch):
    """test 4096 x train 60000 x d 784: the reference's difference tensor would be 770 GB. The peak comes from the
    caching allocator's statistics; the canary allocator of PG_GUARD=1 keeps none, so there every device tensor the
    call creates is added up instead (an upper bound of the peak)."""
    from pytorch_generative_amd import ops

    m, n, d = 4096, 60000, 784
    g = torch.Generator(device=DEV).manual_seed(0)
    train = torch.rand(n, d, device=DEV, generator=g)
    test = torch.rand(m, d, device=DEV, generator=g)
    torch.cuda.synchronize()
    try:
        torch.cuda.reset_peak_memory_stats()
        have_stats = True
    except RuntimeError:
        have_stats = False
    created = []
    if not have_stats:
        real_empty = torch.empty

        def counting_empty(*args, **kwargs):
            t = real_empty(*args, **kwargs)
            if t.is_cuda:
                created.append(t.numel() * t.element_size())
            return t

        monkeypatch.setattr(torch, "empty", counting_empty)
    base = torch.cuda.memory_allocated() if have_stats else 0
    out = ops.kde_gaussian(test, train, 0.5)
    torch.cuda.synchronize()
    monkeypatch.undo()
    peak = torch.cuda.max_memory_allocated() - base if have_stats else sum(created)
    assert peak >= 4 * m, "the measurement must at least see the output"
    allowed = 4 * m + 4 * int(lib.pg_kde_workspace_floats(m, n, d)) + (64 << 20)
    print(f"[density] kde 4096 x 60000 x 784: peak extra memory {peak / 2**20:.2f} MiB (allowed {allowed / 2**20:.2f})")
    assert out.shape == (m,) and bool(torch.isfinite(out).all())
    assert peak <= allowed, (peak, allowed)
    # a few rows against the float64 restatement
    want = kde_gaussian_truth(test[:3].cpu(), train.cpu(), 0.5)
    _util.assert_close(out[:3], want, 1e-4, "kde 4096 x 60000 x 784, first rows")
