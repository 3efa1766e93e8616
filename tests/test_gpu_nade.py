"""GPU: NADE on the chunked prefix-scan kernels (csrc/nade.hip) — forward and all four gradients against the float64 closed form
of tests/_nade_ref.py over every branch of the plan (tests/nade_cases.py; tests/test_nade_cpu.py checks the conditions on the
inputs), bit reproducibility, exact linearity in the incoming gradient; the model against the reference fixture
(tests/golden/nade/cases.pt) with recipes.bce_loss and FlatAdam; graph replay; sample() on both routes; the errors."""

import copy
import os

import pytest
import torch

import _nade_ref as nref
import _util
import nade_cases as nc

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
CASES = os.path.join(_util.GOLDEN_DIR, "nade", "cases.pt")
LR = 1e-3
OUT_TOL = 1e-4  # the project's output gate: max |got - want| <= OUT_TOL * max |want|


def load_cases():
    return torch.load(CASES, map_location="cpu", weights_only=False)["cases"]


def nade_mod():
    from pytorch_generative_amd.models.autoregressive import nade

    return nade


def _reference(t, slice_n=32):
    """(p, logits, grads) in float64, the sums over samples accumulated slice by slice (memory of the recipe's shape)."""
    w = nc.params(t)
    ps, ls, grads = [], [], None
    for s in range(0, t["x"].shape[0], slice_n):
        x, g = t["x"][s:s + slice_n], t["g"][s:s + slice_n]
        p, l, _ = nref.forward(x, *w)
        ps.append(p)
        ls.append(l)
        part = nref.grads(x, *w, g)
        grads = part if grads is None else {k: grads[k] + part[k] for k in part}
    return torch.cat(ps), torch.cat(ls), grads


def _run(t, g_scale=1.0):
    """(p, logits, {key: gradient}) of ops.nade on the GPU."""
    from pytorch_generative_amd import ops

    w = [t[k].to(DEV).requires_grad_(True) for k in nref.KEYS]
    p, logits = ops.nade(t["x"].to(DEV), *w, return_logits=True)
    assert not logits.requires_grad
    p.backward(t["g"].to(DEV) * g_scale)
    torch.cuda.synchronize()
    return p.detach(), logits, {k: wi.grad for k, wi in zip(nref.KEYS, w)}


def _check(t, what):
    want_p, want_l, want_g = _reference(t)
    p, logits, grads = _run(t)
    assert p.shape == t["x"].shape and logits.shape == t["x"].shape
    print(f"[nade] {what}: logits {_util.rel_err(logits, want_l):.3e}, probabilities {_util.rel_err(p, want_p):.3e}")
    _util.assert_close(logits, want_l, OUT_TOL, f"{what} logits")
    _util.assert_close(p, want_p, OUT_TOL, f"{what} probabilities")
    rep = _util.GradReport(what)
    for k in nref.KEYS:
        rep.add(k, grads[k], want_g[k])
    rep.finish()
    # the same again: bit for bit; and half the incoming gradient: exactly half of every gradient
    p2, logits2, grads2 = _run(t)
    assert torch.equal(p, p2) and torch.equal(logits, logits2)
    _, _, half = _run(t, 0.5)
    for k in nref.KEYS:
        assert torch.equal(grads[k], grads2[k]), f"{what}: d{k} differs between two runs"
        assert torch.equal(half[k] * 2, grads[k]), f"{what}: d{k} is not linear in the incoming gradient"


@pytest.mark.parametrize("shape", nc.EXACT_SHAPES, ids=nc.shape_id)
def test_exact_cases_float64(shape):
    _check(nc.exact_inputs(shape), f"exact {nc.shape_id(shape)}")


@pytest.mark.parametrize("shape", nc.GENERIC_SHAPES, ids=nc.shape_id)
def test_generic_cases_float64(shape):
    _check(nc.generic_inputs(shape)[0], f"generic {nc.shape_id(shape)}")


def test_a_row_does_not_depend_on_the_batch_or_its_slot():
    """A sample's output row: the same bits for any N and any slot of its tile."""
    from pytorch_generative_amd import ops

    t = nc.exact_inputs((nc.CHUNK + 1, 65, nc.TILE + 6))
    w = [t[k].to(DEV) for k in nref.KEYS]
    x = t["x"].to(DEV)
    p, logits = ops.nade(x, *w, return_logits=True)
    for lo, hi in ((5, 38), (0, 1), (nc.TILE - 1, nc.TILE + 6), (nc.TILE + 5, nc.TILE + 6)):
        ps, ls = ops.nade(x[lo:hi].contiguous(), *w, return_logits=True)
        assert torch.equal(ps, p[lo:hi]) and torch.equal(ls, logits[lo:hi]), (lo, hi)
    perm = torch.randperm(x.shape[0], generator=torch.Generator().manual_seed(0)).to(DEV)
    pp = ops.nade(x[perm].contiguous(), *w)
    assert torch.equal(pp, p[perm])


def test_rows_permuted_within_a_tile_keep_the_bias_gradient_within_the_gates():
    """The order of the sum over samples changes, so bit equality is not claimed; the gates hold."""
    shape = (nc.CHUNK + 1, 65, nc.TILE + 1)
    t = nc.exact_inputs(shape)
    _, _, want = _reference(t)
    perm = torch.arange(shape[2])
    perm[:nc.BWD_TILE] = torch.randperm(nc.BWD_TILE, generator=torch.Generator().manual_seed(1))
    assert not torch.equal(perm, torch.arange(shape[2]))
    tp = dict(t, x=t["x"][perm].contiguous(), g=t["g"][perm].contiguous())
    _, _, grads = _run(tp)
    rep = _util.GradReport("rows permuted within a tile")
    for k in nref.KEYS:
        rep.add(k, grads[k], want[k])
    rep.finish()


# ---------------------------------------------------------------------------------------------
# the model against the reference's recorded step
def _model_from(state, kwargs):
    model = nade_mod().NADE(**kwargs)
    model.load_state_dict(state, strict=True)
    return model.to(DEV)


@pytest.mark.parametrize("name", sorted(load_cases()))
def test_model_parity_with_fixture(name):
    from pytorch_generative_amd import optim, recipes

    case = load_cases()[name]
    model = _model_from(case["state"], case["kwargs"])
    opt = optim.FlatAdam(model.parameters(), lr=LR)
    x = case["x"].to(DEV)
    opt.zero_grad()
    p = model(x)
    loss = recipes.bce_loss(x, None, p)
    loss.backward()
    torch.cuda.synchronize()
    assert p.shape == x.shape
    _util.assert_close(p, case["probs"], OUT_TOL, f"{name} probabilities")
    _util.assert_close(loss, case["loss"], OUT_TOL, f"{name} loss")
    named = dict(model.named_parameters())
    rep = _util.GradReport(name)
    for k, want in case["grads"].items():
        rep.add(k, named[k].grad, want)
    rep.finish()
    opt.step()
    torch.cuda.synchronize()
    for k, want in case["params_after_adam"].items():
        # 1e-4 relative above the gradient noise floor; below it Adam's first step is lr * sign(round-off)
        got, gref = named[k].detach().double().cpu(), case["grads"][k].double()
        above = gref.abs() > 1e-5 * float(gref.abs().max())
        d = (got - want.double()).abs()
        assert float(d[above].max()) <= 1e-4 * float(want.abs().max()) + 1e-7, k
        assert float(d.max()) <= 2 * LR + 1e-6, k


def _recipe_like(seed=0, d=70, h=100):
    torch.manual_seed(seed)
    return nade_mod().NADE(d, h).to(DEV)


def test_graphed_steps_equal_eager_bitwise():
    from pytorch_generative_amd import graph, ops, optim

    loss_fn = lambda x, preds: ops.bce_with_logits_sum_mean(preds, x)  # noqa: E731
    g = torch.Generator().manual_seed(5)
    xs = [torch.bernoulli(torch.full((40, 1, 7, 10), 0.3), generator=g).to(DEV) for _ in range(3)]
    m1 = _recipe_like()
    m2 = copy.deepcopy(m1)
    o1, o2 = optim.FlatAdam(m1.parameters(), lr=LR), optim.FlatAdam(m2.parameters(), lr=LR)
    step = graph.GraphedTrainStep(m2, o2, loss_fn, xs[0], preserve_state=True)
    for x in xs:
        o1.zero_grad()
        loss_fn(x, m1(x)).backward()
        o1.step()
        step(x)
        torch.cuda.synchronize()
        for (k, p1), (_, p2) in zip(m1.named_parameters(), m2.named_parameters()):
            assert torch.equal(p1, p2), f"{k}: graph replay differs from the eager step"
            assert torch.equal(p1.grad, p2.grad), f"{k}: gradient of the graph replay differs from the eager step"
    assert float(m1._in_W.grad.abs().max()) > 0


# ---------------------------------------------------------------------------------------------
# sampling
def _half(shape, device, generator):
    return torch.full(shape, 0.5, device=device)


@pytest.mark.parametrize("name", sorted(load_cases()))
def test_sample_matches_fixture_on_both_routes(name):
    case = load_cases()[name]
    model = _model_from(case["sample_state"], case["kwargs"])
    model._uniforms = _half                       # the chain draws u < p: p > 0.5
    model._draw = lambda p: (p > 0.5).float()     # the full route's Bernoulli draw, as the fixture was recorded
    cond = case["conditioned_on"].to(DEV)
    given = case["conditioned_on"] >= 0
    for incremental, route in ((True, "chain"), (False, "full")):
        got = model.sample(conditioned_on=cond, incremental=incremental)
        assert model._sample_route == route
        assert got.shape == cond.shape and torch.equal(got.cpu(), case["sample"]), route
        assert torch.equal(got.cpu()[given], case["conditioned_on"][given])
        assert torch.equal(cond.cpu(), case["conditioned_on"]), "conditioned_on must not be modified"
    got, logits = model.sample(conditioned_on=cond, return_logits=True)
    n = cond.shape[0]
    _, want = nref.sample(case["conditioned_on"].reshape(n, -1), *[case["sample_state"][k] for k in nref.KEYS],
                          torch.full((n, case["kwargs"]["input_dim"]), 0.5))
    assert logits.shape == cond.shape and torch.equal(got.cpu(), case["sample"])
    _util.assert_close(logits.reshape(n, -1), want, 1e-4, f"{name} chain logits")  # made_sample_cases.LOGIT_TOL


def test_sample_from_scratch_and_generator():
    model = _recipe_like(seed=3, d=12, h=20)
    assert tuple(model.sample(5).shape) == (5, 12) and model._sample_route == "chain"  # no image batch seen: vectors
    draws = []
    for seed in (11, 11, 12):
        gen = torch.Generator(device=DEV).manual_seed(seed)
        draws.append(model.sample(64, generator=gen))
        assert bool(((draws[-1] == 0) | (draws[-1] == 1)).all())
    assert torch.equal(draws[0], draws[1]) and not torch.equal(draws[0], draws[2])
    model(torch.zeros(2, 1, 3, 4, device=DEV))
    assert tuple(model.sample(3).shape) == (3, 1, 3, 4)


# ---------------------------------------------------------------------------------------------
# errors
def test_errors():
    from pytorch_generative_amd import ops

    t = nc.exact_inputs((12, 20, 5))
    x = t["x"].to(DEV)
    w = [t[k].to(DEV) for k in nref.KEYS]
    with pytest.raises(RuntimeError, match="cuda"):
        ops.nade(t["x"], *w)
    with pytest.raises(RuntimeError, match="cuda"):
        ops.nade(x, w[0].cpu(), *w[1:])
    with pytest.raises(ValueError, match="requires_grad"):
        ops.nade(x.clone().requires_grad_(True), *w)
    with pytest.raises(ValueError, match="shape"):
        ops.nade(x, w[0], w[1], w[2].t().contiguous(), w[3])
    with pytest.raises(ValueError, match="shape"):
        ops.nade(x[:, :11].contiguous(), *w)
    with pytest.raises(ValueError, match="expected x"):
        ops.nade(x.view(5, 3, 4), *w)
    with pytest.raises(ValueError, match="contiguous"):
        ops.nade(x.t().contiguous().t(), *w)
    with pytest.raises(ValueError, match="contiguous"):
        ops.nade(x, w[0].t().contiguous().t(), *w[1:])
    with pytest.raises(TypeError, match="float32"):
        ops.nade(x.double(), *w)
    big = nade_mod().NADE(12, 8193).to(DEV)
    with pytest.raises(ValueError, match="8193 hidden units unsupported"):
        big(x)
    model = nade_mod().NADE(12, 20).to(DEV)
    model.input_codes = 4
    with pytest.raises(ValueError, match="input_codes"):
        model(x)
    with pytest.raises(ValueError, match="input_codes"):
        model.sample(2)


def test_reproduce_debug_loader(tmp_path):
    nade = nade_mod()

    class _Loader:
        def __iter__(self):
            g = torch.Generator().manual_seed(0)
            return iter([(torch.bernoulli(torch.full((8, 1, 28, 28), 0.2), generator=g), torch.zeros(8)) for _ in range(2)])

    t = nade.reproduce(n_epochs=1, log_dir=str(tmp_path), debug_loader=_Loader())
    assert t._epoch == 1 and t._step == 2 and t._use_graph
    assert all(torch.isfinite(p).all() for p in t.model.parameters())
    assert isinstance(t.model, nade.NADE) and tuple(t.model._in_W.shape) == (500, 784)
