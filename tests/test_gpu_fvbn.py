"""GPU: the FVBN on the packed-triangular kernels (csrc/fvbn.hip) — forward and weight gradient against the float64 closed form
of tests/_fvbn_ref.py over every branch of the plan, the exact properties of the packed layout (row 0, pads, bit
reproducibility, independence of the batch), pack / unpack; the model against the reference fixture
(tests/golden/fvbn/cases.pt) with recipes.bce_loss and FlatAdam; graph replay; sample() on both routes; the errors.

Gates: outputs max |got - want| <= 1e-4 max |want|; gradients that AND |d| <= 1e-4 |want| + 5e-6 max |want| per element
(_util.GradReport)."""

import copy
import functools
import os

import pytest
import torch

import _fvbn_ref as fref
import _util

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
CASES = os.path.join(_util.GOLDEN_DIR, "fvbn", "cases.pt")
LR = 1e-3
OUT_TOL = 1e-4  # the project's output gate: max |got - want| <= OUT_TOL * max |want|
TILE = 64
D_LIST = (1, 2, 3, 4, 5, 15, 16, 17, 63, 64, 65, 130, 200, 3 * TILE + 1)  # the last: above two (and three) tile rows
N_LIST = (1, 3, 64, 65, 257)
WALKED = (200, 33 * TILE - 62)  # 132 output tiles: no k-split, a workgroup walks the slices of its column tile itself
SHAPES = [(d, n) for d in D_LIST for n in N_LIST] + [WALKED]


def shape_id(shape):
    return "d{}-n{}".format(*shape)


def load_cases():
    return torch.load(CASES, map_location="cpu", weights_only=False)["cases"]


def fvbn_mod():
    from pytorch_generative_amd.models.autoregressive import fvbn

    return fvbn


@functools.lru_cache(maxsize=None)
def inputs(shape):
    """{x, w (dense, with a dummy weight at [0, 0] and values above the diagonal that must not matter), b, g} on the CPU and the
    float64 results {logits, dw, db}: made once per shape and not modified."""
    d, n = shape
    g = torch.Generator().manual_seed((d * 1009 + n) * 31)
    t = {"x": torch.randn(n, d, generator=g), "w": torch.randn(d, d, generator=g) / max(1, d) ** 0.5,
         "b": torch.randn(d, generator=g) * 0.3, "g": torch.randn(n, d, generator=g)}
    t["logits"] = fref.forward(t["x"], t["w"], t["b"])
    t["dw"], t["db"] = fref.grads(t["x"], t["g"])
    return t


def _run(t, g_scale=1.0, x=None):
    """(logits, packed dW, db) of ops.fvbn on the GPU, the gradients through the returned-tensor path."""
    from pytorch_generative_amd import ops

    wp = ops.fvbn_pack(t["w"].to(DEV)).requires_grad_(True)
    b = t["b"].to(DEV).requires_grad_(True)
    logits = ops.fvbn((t["x"] if x is None else x).to(DEV), wp, b)
    logits.backward(t["g"].to(DEV) * g_scale)
    torch.cuda.synchronize()
    return logits.detach(), wp.grad, b.grad


@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_forward_and_gradients_float64(shape):
    d, n = shape
    t = inputs(shape)
    logits, dwp, db = _run(t)
    assert logits.shape == (n, d) and dwp.shape == (fref.packed_floats(d),) and db.shape == (d,)
    print(f"[fvbn] {shape_id(shape)}: logits {_util.rel_err(logits, t['logits']):.3e}")
    _util.assert_close(logits, t["logits"], OUT_TOL, f"{shape_id(shape)} logits")
    dw = fref.unpack(dwp.cpu(), d)
    rep = _util.GradReport(shape_id(shape))
    if d > 1:
        rep.add("dW", dw, t["dw"])
    rep.add("db", db, t["db"])
    rep.finish()
    # exact: logits[:, 0] is the bias, row 0 and every pad of the gradient are zero
    assert torch.equal(logits[:, 0], t["b"][0].to(DEV).expand(n))
    assert not bool(dwp[fref.pad_mask(d).to(DEV)].any()), "pads of the weight gradient"
    assert float(dwp[0]) == 0.0 and not bool(dw[0].any()), "row 0 of the weight gradient"
    # the same again: bit for bit; and half the incoming gradient: exactly half of every gradient
    logits2, dwp2, db2 = _run(t)
    assert torch.equal(logits, logits2) and torch.equal(dwp, dwp2) and torch.equal(db, db2)
    _, dwp_h, db_h = _run(t, 0.5)
    assert torch.equal(dwp_h * 2, dwp) and torch.equal(db_h * 2, db)


def test_the_shapes_hit_every_branch_of_the_plan():
    """Read from the plan: a tile strictly below the diagonal, a split weight gradient and a ragged last tile all occur (and so do
    their opposites), so none of those branches can vanish silently."""
    from pytorch_generative_amd import ops

    seen = {}
    for d, n in SHAPES:
        p = ops.fvbn_plan(d, n)
        assert p is not None and p["tile"] == TILE
        tiles = ops.fvbn_tiles(d, 1)
        facts = {"a tile strictly below the diagonal": any(j1 <= i0 for i0, _, _, j1 in tiles),
                 "a forward k chunk strictly below the diagonal": any(j1 <= i0 for i0, _, _, j1 in ops.fvbn_tiles(d, 0)),
                 "several k chunks": p["forward_weight_tiles"] > p["column_tiles"],
                 "forward split along k": p["forward_split"] == 1,
                 "several k slices walked by one workgroup": p["forward_split"] == 0 and p["forward_slices"] > p["column_tiles"],
                 "two or more weight-gradient slices": p["wgrad_slices"] >= 2, "ragged last tile": d % p["tile"] != 0,
                 "ragged sample tile": n % p["tile"] != 0, "several sample tiles": p["forward_row_tiles"] > 1,
                 "ragged last slice": n % p["samples_per_slice"] != 0}
        for k, v in facts.items():
            seen.setdefault(k, set()).add(v)
    assert all(v == {True, False} for v in seen.values()), seen
    assert max(D_LIST) > 2 * TILE


def test_entries_at_and_behind_a_dimension_do_not_reach_it():
    """Replacing x[:, j >= i0] by other finite values leaves logits[:, :i0 + 1] bit-identical."""
    for shape, i0 in (((200, 65), 0), ((200, 65), 63), ((200, 65), 64), ((200, 65), 130), ((17, 3), 5), ((65, 64), 64)):
        t = inputs(shape)
        base, _, _ = _run(t)
        x = t["x"].clone()
        x[:, i0:] = torch.randn(x[:, i0:].shape, generator=torch.Generator().manual_seed(i0)) * 1e3
        got, _, _ = _run(t, x=x)
        assert torch.equal(got[:, :i0 + 1], base[:, :i0 + 1]), (shape, i0)
        assert shape[0] == i0 + 1 or not torch.equal(got[:, i0 + 1:], base[:, i0 + 1:])


def test_a_row_does_not_depend_on_the_batch_or_its_slot():
    from pytorch_generative_amd import ops

    t = inputs((200, 65))
    wp, b, x = ops.fvbn_pack(t["w"].to(DEV)), t["b"].to(DEV), t["x"].to(DEV)
    logits = ops.fvbn(x, wp, b)
    for lo, hi in ((0, 1), (7, 8), (64, 65), (5, 38)):
        assert torch.equal(ops.fvbn(x[lo:hi].contiguous(), wp, b), logits[lo:hi]), (lo, hi)
    perm = torch.randperm(65, generator=torch.Generator().manual_seed(0)).to(DEV)
    assert torch.equal(ops.fvbn(x[perm].contiguous(), wp, b), logits[perm])
    # with and without the forward's k-split: the slices are added in one order either way
    t = inputs(WALKED)
    assert ops.fvbn_plan(*WALKED)["forward_split"] == 0 and ops.fvbn_plan(WALKED[0], 65)["forward_split"] == 1
    wp, b, x = ops.fvbn_pack(t["w"].to(DEV)), t["b"].to(DEV), t["x"].to(DEV)
    logits = ops.fvbn(x, wp, b)
    for lo, hi in ((0, 1), (100, 165), (WALKED[1] - 3, WALKED[1])):
        assert torch.equal(ops.fvbn(x[lo:hi].contiguous(), wp, b), logits[lo:hi]), (lo, hi)


@pytest.mark.parametrize("shape", [(130, 257), (200, 64), (5, 3)], ids=shape_id)
def test_sink_path_equals_returned_path(shape):
    """Gradients added into FlatAdam's sinks are the bits of the tensors autograd gets without an optimiser."""
    from pytorch_generative_amd import ops, optim

    t = inputs(shape)
    _, dwp, db = _run(t)
    wp = torch.nn.Parameter(ops.fvbn_pack(t["w"].to(DEV)))
    b = torch.nn.Parameter(t["b"].to(DEV))
    opt = optim.FlatAdam([b, wp], lr=LR)  # the bias first: the packed weight does not start the flat buffer
    assert wp.data_ptr() % 16 == 0
    opt.zero_grad()
    ops.fvbn(t["x"].to(DEV), wp, b).backward(t["g"].to(DEV))
    torch.cuda.synchronize()
    assert wp.grad is wp._pg_grad and torch.equal(wp.grad, dwp) and torch.equal(b.grad, db)


@pytest.mark.parametrize("d", [1, 2, 5, 65, 200])
def test_pack_and_unpack(d):
    from pytorch_generative_amd import ops

    w = inputs((d, 3))["w"]
    packed = ops.fvbn_pack(w.to(DEV))
    assert torch.equal(packed.cpu(), fref.pack(w))
    dense = ops.fvbn_unpack(packed, d)
    assert torch.equal(dense.cpu(), fref.unpack(fref.pack(w), d))
    assert torch.equal(ops.fvbn_pack(dense), packed)


# ---------------------------------------------------------------------------------------------
# the model against the reference's recorded step
def _model_from(state, kwargs, **extra):
    model = fvbn_mod().FullyVisibleBeliefNetwork(**kwargs, **extra)
    model.load_state_dict(state, strict=True)
    return model.to(DEV)


@pytest.mark.parametrize("name", sorted(load_cases()))
def test_model_parity_with_fixture(name):
    from pytorch_generative_amd import optim, recipes

    case = load_cases()[name]
    d = case["kwargs"]["n_dims"]
    model = _model_from(case["state"], case["kwargs"])
    opt = optim.FlatAdam(model.parameters(), lr=LR)
    x = case["x"].to(DEV)
    opt.zero_grad()
    logits = model(x)
    loss = recipes.bce_loss(x, None, logits)
    loss.backward()
    torch.cuda.synchronize()
    assert logits.shape == x.shape
    _util.assert_close(logits, case["logits"], OUT_TOL, f"{name} logits")
    _util.assert_close(loss, case["loss"], OUT_TOL, f"{name} loss")
    grads = fref.packed_to_keys(model._weight.grad.cpu(), model._bias.grad.cpu(), d)
    assert list(grads) == list(case["grads"])
    rep = _util.GradReport(name)
    for k, want in case["grads"].items():
        assert grads[k].shape == want.shape
        rep.add(k, grads[k], want)
    rep.finish()
    pads = fref.pad_mask(d).to(DEV)
    assert not bool(model._weight.grad[pads].any())
    opt.step()
    torch.cuda.synchronize()
    after = model.state_dict()
    assert not bool(model._weight.detach()[pads].any()), "pads after the step"
    assert torch.equal(after["_net.0.weight"].cpu(), case["state"]["_net.0.weight"]), "the dummy weight has no gradient"
    for k, want in case["params_after_adam"].items():
        # 1e-4 relative above the gradient noise floor; below it Adam's first step is lr * sign(round-off)
        got, gref = after[k].detach().double().cpu(), case["grads"][k].double()
        above = gref.abs() > 1e-5 * float(gref.abs().max())
        d_abs = (got - want.double()).abs()
        if bool(above.any()):
            assert float(d_abs[above].max()) <= 1e-4 * float(want.abs().max()) + 1e-7, k
        assert float(d_abs.max()) <= 2 * LR + 1e-6, k


def test_graphed_steps_equal_eager_bitwise():
    from pytorch_generative_amd import graph, ops, optim

    loss_fn = lambda x, preds: ops.bce_with_logits_sum_mean(preds, x)  # noqa: E731
    g = torch.Generator().manual_seed(5)
    xs = [torch.bernoulli(torch.full((40, 1, 7, 10), 0.3), generator=g).to(DEV) for _ in range(4)]
    torch.manual_seed(0)
    m1 = fvbn_mod().FullyVisibleBeliefNetwork(70).to(DEV)
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
    assert float(m1._weight.grad.abs().max()) > 0
    pads = fref.pad_mask(70).to(DEV)
    for m in (m1, m2):
        assert not bool(m._weight.detach()[pads].any()) and not bool(m._weight.grad[pads].any()), "pads after four steps"


# ---------------------------------------------------------------------------------------------
# sampling
def _half(shape, device, generator):
    return torch.full(shape, 0.5, device=device)


# (D, N): one, two and four samples per workgroup; rows longer than the chunks requested one row ahead (D > 1024); two samples
# per workgroup forced by the LDS (D > 3072)
@pytest.mark.parametrize("shape", [(1, 1), (5, 2), (130, 5), (1100, 3), (3100, 3)], ids=shape_id)
def test_chain_with_a_given_canvas_float64(shape):
    """Everything given: logits_out is the teacher-forced forward, within 1e-4 of the float64 chain, and the canvas is unchanged."""
    from pytorch_generative_amd import ops

    d, n = shape
    g = torch.Generator().manual_seed(d)
    w = torch.randn(d, d, generator=g) / d ** 0.5
    b = torch.randn(d, generator=g) * 0.3
    canvas = torch.bernoulli(torch.full((n, d), 0.5), generator=g)
    want_x, want_l = fref.sample(canvas, w, b, torch.rand(n, d, generator=g))
    plan = ops.fvbn_plan(d, n)
    assert plan["sampler_samples_per_workgroup"] == {(1, 1): 1, (5, 2): 2, (130, 5): 4, (1100, 3): 4, (3100, 3): 2}[shape]
    dev_canvas = canvas.to(DEV)
    got, logits = ops.fvbn_sample_chain(dev_canvas, ops.fvbn_pack(w.to(DEV)), b.to(DEV), torch.rand(n, d, device=DEV),
                                        return_logits=True)
    torch.cuda.synchronize()
    assert got is dev_canvas and torch.equal(got.cpu(), canvas) and torch.equal(want_x.float(), canvas)
    print(f"[fvbn] chain {shape_id(shape)}: logits {_util.rel_err(logits, want_l):.3e}")
    _util.assert_close(logits, want_l, OUT_TOL, f"chain {shape_id(shape)} logits")
    assert torch.equal(logits[:, 0], b[0].to(DEV).expand(n))


@pytest.mark.parametrize("name", sorted(load_cases()))
def test_sample_matches_fixture_on_both_routes(name):
    case = load_cases()[name]
    cond = case["conditioned_on"].to(DEV)
    given = case["conditioned_on"] >= 0
    chain = _model_from(case["sample_state"], case["kwargs"])
    chain._uniforms = _half  # the chain draws u < sigmoid(l): l > 0
    full = _model_from(case["sample_state"], case["kwargs"], sample_fn=lambda l: (l > 0).float())
    for model, route in ((chain, "chain"), (full, "full")):
        got = model.sample(conditioned_on=cond)
        assert model._sample_route == route
        assert got.shape == cond.shape and torch.equal(got.cpu(), case["sample"]), route
        assert torch.equal(got.cpu()[given], case["conditioned_on"][given])
        assert torch.equal(cond.cpu(), case["conditioned_on"]), "conditioned_on must not be modified"
    got = chain.sample(conditioned_on=cond, incremental=False)  # the default sample_fn draws: only the given entries are fixed
    assert chain._sample_route == "full" and torch.equal(got.cpu()[given], case["conditioned_on"][given])
    assert bool(((got == 0) | (got == 1)).all())
    with pytest.raises(ValueError, match="return_logits"):
        full.sample(conditioned_on=cond, return_logits=True)
    with pytest.raises(ValueError, match="return_logits"):
        chain.sample(conditioned_on=cond, incremental=False, return_logits=True)
    d = case["kwargs"]["n_dims"]
    n = cond.shape[0]
    got, logits = chain.sample(conditioned_on=cond, return_logits=True)
    w, b = fref.state_to_dense(case["sample_state"], d)
    _, want = fref.sample(case["conditioned_on"].reshape(n, -1), w, b, torch.full((n, d), 0.5))
    assert logits.shape == cond.shape and torch.equal(got.cpu(), case["sample"])
    _util.assert_close(logits.reshape(n, -1), want, OUT_TOL, f"{name} chain logits")


def test_sample_from_scratch_draws_u_below_sigmoid():
    """(N, D) = (64, 130): every drawn entry is u < sigmoid(logits_out), recomputed in float64; entries with |u - p| <= 1e-6 are
    left out (about 0.02 expected among 8320: at most one). The logits are the float64 forward of the finished sample."""
    n, d = 64, 130
    torch.manual_seed(3)
    model = fvbn_mod().FullyVisibleBeliefNetwork(d).to(DEV)
    with torch.no_grad():
        model._weight.mul_(4.0)  # logits of order 1: probabilities away from 1/2
    got, logits = model.sample(n, return_logits=True, generator=torch.Generator(device=DEV).manual_seed(11))
    assert model._sample_route == "chain" and tuple(got.shape) == (n, d) == tuple(logits.shape)
    u = torch.rand((n, d), device=DEV, generator=torch.Generator(device=DEV).manual_seed(11)).double().cpu()
    p = torch.sigmoid(logits.double().cpu())
    clear = (u - p).abs() > 1e-6
    assert int((~clear).sum()) <= 1
    assert torch.equal(got.cpu().double()[clear], (u < p).double()[clear])
    assert 0.05 < float(got.mean()) < 0.95
    want = fref.forward(got.cpu(), fref.unpack(model._weight.detach().cpu(), d), model._bias.detach().cpu())
    _util.assert_close(logits, want, OUT_TOL, "logits of the finished sample")
    # a sample's row: the same bits alone and in any slot of a batch, given its uniforms
    from pytorch_generative_amd import ops

    dev_u = u.float().to(DEV)
    for lo, hi in ((0, 1), (5, 6), (62, 64), (3, 6)):
        canvas = torch.full((hi - lo, d), -1.0, device=DEV)
        x1, l1 = ops.fvbn_sample_chain(canvas, model._weight.data, model._bias.data, dev_u[lo:hi].contiguous(), return_logits=True)
        assert torch.equal(x1, got[lo:hi]) and torch.equal(l1, logits[lo:hi]), (lo, hi)


def test_sample_keeps_given_entries_and_generators_repeat():
    torch.manual_seed(3)
    model = fvbn_mod().FullyVisibleBeliefNetwork(12).to(DEV)
    assert tuple(model.sample(5).shape) == (5, 12) and model._sample_route == "chain"  # no image batch seen: vectors
    draws = []
    for seed in (11, 11, 12):
        gen = torch.Generator(device=DEV).manual_seed(seed)
        draws.append(model.sample(64, generator=gen))
        assert bool(((draws[-1] == 0) | (draws[-1] == 1)).all())
    assert torch.equal(draws[0], draws[1]) and not torch.equal(draws[0], draws[2])
    cond = torch.full((7, 12), -1.0, device=DEV)
    cond[:, 3], cond[:, 8], cond[2, :] = 1.0, 0.25, 0.0
    before = cond.clone()
    for incremental in (True, False):
        got = model.sample(conditioned_on=cond, incremental=incremental)
        assert torch.equal(cond, before) and torch.equal(got[before >= 0], before[before >= 0])
        assert bool(((got == 0) | (got == 1))[before < 0].all())
    model(torch.zeros(2, 1, 3, 4, device=DEV))
    assert tuple(model.sample(3).shape) == (3, 1, 3, 4)
    assert tuple(model.sample(3, incremental=False).shape) == (3, 1, 3, 4) and model._sample_route == "full"


# ---------------------------------------------------------------------------------------------
# errors
def test_errors():
    from pytorch_generative_amd import ops

    t = inputs((12, 5))
    x = t["x"].to(DEV)
    wp, b = ops.fvbn_pack(t["w"].to(DEV)), t["b"].to(DEV)
    with pytest.raises(RuntimeError, match="cuda"):
        ops.fvbn(t["x"], wp, b)
    with pytest.raises(RuntimeError, match="cuda"):
        ops.fvbn(x, wp.cpu(), b)
    with pytest.raises(ValueError, match="requires_grad"):
        ops.fvbn(x.clone().requires_grad_(True), wp, b)
    with pytest.raises(ValueError, match="shape"):
        ops.fvbn(x, wp[:-4], b)
    with pytest.raises(ValueError, match="shape"):
        ops.fvbn(x, t["w"].to(DEV), b)
    with pytest.raises(ValueError, match="shape"):
        ops.fvbn(x[:, :11].contiguous(), wp, b)
    with pytest.raises(ValueError, match="expected x"):
        ops.fvbn(x.view(5, 3, 4), wp, b)
    with pytest.raises(ValueError, match="contiguous"):
        ops.fvbn(x.t().contiguous().t(), wp, b)
    with pytest.raises(TypeError, match="float32"):
        ops.fvbn(x.double(), wp, b)
    with pytest.raises(ValueError, match="aligned"):
        ops.fvbn(x, torch.cat([wp.new_zeros(1), wp])[1:], b)
    with pytest.raises(ValueError, match="D = 8193 unsupported"):
        ops.fvbn(torch.zeros(2, 8193, device=DEV), wp, b)
    with pytest.raises(ValueError, match="expected a"):
        ops.fvbn_pack(x)
    with pytest.raises(ValueError, match="shape"):
        ops.fvbn_unpack(wp, 13)
    with pytest.raises(ValueError, match="uniforms"):
        ops.fvbn_sample_chain(x.clone(), wp, b, x[:4].contiguous())
    model = fvbn_mod().FullyVisibleBeliefNetwork(12).to(DEV)
    model.input_codes = 4
    with pytest.raises(ValueError, match="input_codes"):
        model(x)
    with pytest.raises(ValueError, match="input_codes"):
        model.sample(2)


def test_reproduce_debug_loader(tmp_path):
    fvbn = fvbn_mod()

    class _Loader:
        def __iter__(self):
            g = torch.Generator().manual_seed(0)
            return iter([(torch.bernoulli(torch.full((8, 1, 28, 28), 0.2), generator=g), torch.zeros(8)) for _ in range(2)])

    t = fvbn.reproduce(n_epochs=1, log_dir=str(tmp_path), debug_loader=_Loader())
    assert t._epoch == 1 and t._step == 2 and t._use_graph
    assert all(torch.isfinite(p).all() for p in t.model.parameters())
    assert isinstance(t.model, fvbn.FullyVisibleBeliefNetwork) and t.model.n_dims == 784
    assert tuple(t.model._weight.shape) == (fref.packed_floats(784),)
    assert not bool(t.model._weight.detach()[fref.pad_mask(784).to(t.model._weight.device)].any())
    assert list(t.model.state_dict())[:5] == ["_c", "_h", "_w", "_net.0.weight", "_net.0.bias"]
