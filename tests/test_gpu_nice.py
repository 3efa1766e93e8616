"""GPU: NICE on the dense fp32-MFMA GEMMs of csrc/dense_linear.hip — every shape of tests/nice_cases.py against the float64
restatement (tests/_nice_ref.py), the fixture cases also against the reference's recorded fp32 results; the three GEMM launches
called directly with row strides and every epilogue; inverse, sampler, bit reproducibility, exact linearity in the incoming
gradient, hipGraph replay against eager steps, gradient sinks, the recipe."""

import copy
import ctypes
import os

import pytest
import torch

import _nice_ref as nref
import _util
import nice_cases as nc

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0) if torch.cuda.is_available() else None
FIXTURES = os.path.join(_util.GOLDEN_DIR, "nice", "cases.pt")
OUT_TOL = 1e-4
LR = 1e-3
SENTINEL = -7.25


def nice_mod():
    from pytorch_generative_amd.models.flows import nice

    return nice


def load_cases():
    return torch.load(FIXTURES, map_location="cpu", weights_only=False)["cases"]


def _model_from(state, kwargs):
    model = nice_mod().NICE(**kwargs)
    model.load_state_dict(state, strict=True)
    return model.to(DEV)


def _close(got, want, what, tol=OUT_TOL):
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    err = float((got.reshape(want.shape) - want).abs().max()) / max(float(want.abs().max()), 1e-30)
    print(f"[nice] {what}: {err:.3e}")
    assert err <= tol, (what, err)


def _step(model, x):
    """One forward + loss + backward; returns (z, log_det_J, loss dict, {name: gradient})."""
    from pytorch_generative_amd import recipes

    for p in model.parameters():
        p.grad = None
    z, ldj = model(x)
    losses = recipes.nice_loss(x, None, (z, ldj))
    losses["loss"].backward()
    torch.cuda.synchronize()
    return z, ldj, losses, {k: p.grad.clone() for k, p in model.named_parameters()}


def _against_float64(name, state, x, got):
    z, ldj, losses, grads = got
    want_z, want_ldj = nref.forward(x, state)
    want_losses, _ = nref.recipe_loss(want_z, want_ldj)
    assert z.shape == x.shape
    _close(z, want_z.reshape(x.shape), f"{name} z")
    _close(ldj, want_ldj, f"{name} log_det_J")
    for k in ("loss", "prior_log_likelihood", "log_det_J"):
        _close(losses[k], want_losses[k], f"{name} {k}")
    rep = _util.GradReport(name)
    for k, want in nref.grads(x, state).items():
        rep.add(k, grads[k], want)
    rep.finish()


# ---------------------------------------------------------------------------------------------
# the model against float64 and the fixture
@pytest.mark.parametrize("case", nc.CASES, ids=nc.case_id)
def test_cases_float64(case):
    state, x = nc.case_inputs(case)
    model = _model_from(state, nc.kwargs(case))
    _against_float64(nc.case_id(case), state, x, _step(model, x.to(DEV)))


@pytest.mark.parametrize("name", sorted(load_cases()))
def test_model_parity_with_fixture(name):
    from pytorch_generative_amd import optim, recipes

    case = load_cases()[name]
    model = _model_from(case["state"], case["kwargs"])
    opt = optim.FlatAdam(model.parameters(), lr=LR)
    x = case["x"].to(DEV)
    opt.zero_grad()
    z, ldj = model(x)
    losses = recipes.nice_loss(x, None, (z, ldj))
    losses["loss"].backward()
    torch.cuda.synchronize()
    named = dict(model.named_parameters())
    got = (z, ldj, losses, {k: p.grad for k, p in named.items()})
    _against_float64(name, case["state"], case["x"], got)
    _close(z, case["z"], f"{name} z (fixture)")
    _close(ldj, case["log_det_J"], f"{name} log_det_J (fixture)")
    for k, want in case["losses"].items():
        _close(losses[k], want, f"{name} {k} (fixture)")
    rep = _util.GradReport(name + " fixture")
    for k, want in case["grads"].items():
        rep.add(k, named[k].grad, want)
    rep.finish()
    with torch.no_grad():  # the recorded inverse is the initial state's
        inv = model._inverse(case["z0"].to(DEV))
    _close(inv, case["inverse"], f"{name} inverse (fixture)")
    _close(inv, nref.inverse(case["z0"], case["state"]).reshape(case["z0"].shape), f"{name} inverse")
    opt.step()
    torch.cuda.synchronize()
    for k, want in case["params_after_adam"].items():
        # 1e-4 relative above the gradient noise floor; below it Adam's first step is lr * sign(round-off)
        gotp, gref = named[k].detach().double().cpu(), case["grads"][k].double()
        above = gref.abs() > 1e-5 * float(gref.abs().max())
        d = (gotp - want.double()).abs()
        assert float(d[above].max()) <= 1e-4 * float(want.abs().max()) + 1e-7, k
        assert float(d.max()) <= 2 * LR + 1e-6, k


# ---------------------------------------------------------------------------------------------
# the launches, directly: row strides, every epilogue, columns outside the written range untouched
def _lib():
    from pytorch_generative_amd import _lib

    return _lib


def _ws(n, i, o, kind):
    from pytorch_generative_amd import ops

    floats = ops.dense_linear_plan(n, i, o, kind)["workspace_floats"]
    return torch.empty(max(floats, 1), device=DEV), floats


def _strided(rows, cols, ld, g, fill=None):
    """(the (rows, ld) buffer on the device, its first `cols` columns in float64 on the CPU)."""
    buf = torch.full((rows, ld), SENTINEL)
    buf[:, :cols] = torch.randn(rows, cols, generator=g) if fill is None else fill
    return buf.to(DEV), buf[:, :cols].double()


def _untouched(buf, cols):
    assert bool((buf[:, cols:] == SENTINEL).all()), "columns outside the written range were modified"


# (N, in, out): small tile without and with a k-split, ragged everywhere; then the large tile (>= 192 tiles of 128 x 128) at
# depths that straddle its k chunk of 16, with ragged rows, columns and last chunk: forward at depth in = 33 and at depth 2
# (one partly filled chunk), data gradient at depth out = 17, weight gradient (below) at depth N = 33
DIRECT_SHAPES = [(5, 7, 3), (65, 33, 70), (8, 1500, 32), (130, 129, 258), (1537, 2, 2049), (1537, 33, 2049), (1537, 2049, 17)]


@pytest.mark.parametrize("shape", DIRECT_SHAPES, ids=lambda s: "n{}-i{}-o{}".format(*s))
def test_forward_launch_directly(shape):
    lib, cl = _lib().load(), _lib().check
    n, i, o = shape
    g = torch.Generator().manual_seed(n * 31 + i * 7 + o)
    w = torch.randn(o, i, generator=g) / i ** 0.5
    b = torch.randn(o, generator=g)
    x, x64 = _strided(n, i, i + 3, g)
    res, res64 = _strided(n, o, o + 5, g)
    wd, bd = w.to(DEV), b.to(DEV)
    ws, ws_floats = _ws(n, i, o, "fwd")
    st = torch.cuda.current_stream().cuda_stream
    lin = x64 @ w.double().t()
    for bias, relu, sign in ((True, 0, 0), (False, 0, 0), (True, 1, 0), (True, 0, 1), (False, 0, -1)):
        y = torch.full((n, o + 2), SENTINEL, device=DEV)
        want = lin + (b.double() if bias else 0)
        if relu:
            want = want.clamp_min(0)
        if sign:
            want = res64 + sign * want
        cl(lib.pg_dense_linear_fwd(x.data_ptr(), i + 3, wd.data_ptr(), bd.data_ptr() if bias else 0, res.data_ptr() if sign else 0, o + 5,
                                   sign or 1, y.data_ptr(), o + 2, n, i, o, relu, ws.data_ptr(), ws_floats, st), "fwd")
        torch.cuda.synchronize()
        _close(y[:, :o], want, f"fwd {shape} bias={bias} relu={relu} sign={sign}")
        _untouched(y, o)
    # in place: y is res (the coupling law writes the half it reads)
    y = res.clone()
    cl(lib.pg_dense_linear_fwd(x.data_ptr(), i + 3, wd.data_ptr(), bd.data_ptr(), y.data_ptr(), o + 5, 1, y.data_ptr(), o + 5, n, i, o, 0,
                               ws.data_ptr(), ws_floats, st), "fwd")
    torch.cuda.synchronize()
    _close(y[:, :o], res64 + lin + b.double(), f"fwd {shape} in place")
    _untouched(y, o)
    _untouched(x, i)


@pytest.mark.parametrize("shape", DIRECT_SHAPES, ids=lambda s: "n{}-i{}-o{}".format(*s))
def test_data_gradient_launch_directly(shape):
    lib, cl = _lib().load(), _lib().check
    n, i, o = shape
    g = torch.Generator().manual_seed(n * 37 + i * 5 + o)
    w = torch.randn(o, i, generator=g) / o ** 0.5
    dy, dy64 = _strided(n, o, o + 1, g)
    relu_out, relu64 = _strided(n, i, i + 2, g, fill=torch.randn(n, i, generator=g).clamp_min(0))
    add, add64 = _strided(n, i, i + 4, g)
    wd = w.to(DEV)
    ws, ws_floats = _ws(n, i, o, "dgrad")
    st = torch.cuda.current_stream().cuda_stream
    lin = dy64 @ w.double()
    assert bool((relu64 == 0).any()) and bool((relu64 > 0).any())
    for gate, addend, sign in ((False, False, 1), (True, False, 1), (False, True, -1), (True, True, 1), (True, True, -1)):
        dx = torch.full((n, i + 3), SENTINEL, device=DEV)
        want = sign * lin
        if gate:
            want = want * (relu64 > 0)
        if addend:
            want = want + add64
        cl(lib.pg_dense_linear_dgrad(dy.data_ptr(), o + 1, wd.data_ptr(), relu_out.data_ptr() if gate else 0, i + 2,
                                     add.data_ptr() if addend else 0, i + 4, sign, dx.data_ptr(), i + 3, n, i, o, ws.data_ptr(), ws_floats,
                                     st), "dgrad")
        torch.cuda.synchronize()
        _close(dx[:, :i], want, f"dgrad {shape} gate={gate} addend={addend} sign={sign}")
        _untouched(dx, i)


@pytest.mark.parametrize("shape", DIRECT_SHAPES + [(3, 1665, 1665), (33, 1665, 1665)], ids=lambda s: "n{}-i{}-o{}".format(*s))
def test_weight_gradient_launch_directly(shape):
    lib, cl = _lib().load(), _lib().check
    n, i, o = shape
    g = torch.Generator().manual_seed(n * 41 + i * 3 + o)
    x, x64 = _strided(n, i, i + 3, g)
    dy, dy64 = _strided(n, o, o + 2, g)
    ws, ws_floats = _ws(n, i, o, "wgrad")
    st = torch.cuda.current_stream().cuda_stream
    dw_want, db_want = dy64.t() @ x64, dy64.sum(0)
    for sign, with_db in ((1, True), (-1, True), (1, False)):
        # added into a buffer that is not zero: buffer + gradient
        dw0, db0 = torch.randn(o, i, generator=g), torch.randn(o, generator=g)
        dw, db = dw0.to(DEV), db0.to(DEV)
        cl(lib.pg_dense_linear_wgrad(x.data_ptr(), i + 3, dy.data_ptr(), o + 2, sign, dw.data_ptr(), db.data_ptr() if with_db else 0, n, i, o,
                                     ws.data_ptr(), ws_floats, st), "wgrad")
        torch.cuda.synchronize()
        # the gate is set by the gradient's magnitude: the buffer is of its order
        scale = max(float(dw_want.abs().max()), float(dw0.abs().max()))
        err = float((dw.double().cpu() - (dw0.double() + sign * dw_want)).abs().max()) / scale
        print(f"[nice] wgrad {shape} sign={sign}: dw {err:.3e}")
        assert err <= OUT_TOL
        if with_db:
            _close(db, db0.double() + sign * db_want, f"wgrad {shape} sign={sign} db")
        else:
            assert torch.equal(db.cpu(), db0)
    _untouched(x, i)
    _untouched(dy, o)


def test_streaming_kernels_directly():
    from pytorch_generative_amd import ops

    g = torch.Generator().manual_seed(3)
    for n, f in ((1, 2), (5, 70), (300, 258), (1025, 784)):
        y = torch.randn(n, f, generator=g)
        s = torch.randn(1, f, generator=g) * 0.5
        gz = torch.randn(n, f, generator=g)
        for sign in (1, -1):
            yd, sd = y.to(DEV).requires_grad_(True), s.to(DEV).requires_grad_(True)
            z = ops.nice_scale(yd, sd, sign)
            z.backward(gz.to(DEV))
            e = torch.exp(sign * s.double())
            _close(z, y.double() * e, f"scale {n}x{f} sign={sign} z")
            _close(yd.grad, gz.double() * e, f"scale {n}x{f} sign={sign} dy")
            _close(sd.grad, sign * (gz.double() * y.double() * e).sum(0, keepdim=True), f"scale {n}x{f} sign={sign} ds")
        z = (torch.randn(n, f, generator=g) * 8)  # both tails of the softplus pair
        z[0, 0], z[-1, -1] = 90.0, -90.0
        zd = z.to(DEV).requires_grad_(True)
        lp = ops.logistic_logprob(zd)
        gl = torch.randn(n, generator=g)
        lp.backward(gl.to(DEV))
        z64 = z.double()
        want = -(torch.nn.functional.softplus(z64) + torch.nn.functional.softplus(-z64)).sum(1)
        _close(lp, want, f"logistic {n}x{f} lp")
        _close(zd.grad, -gl.double()[:, None] * torch.tanh(z64 / 2), f"logistic {n}x{f} dz")
        assert bool(torch.isfinite(lp).all()) and bool(torch.isfinite(zd.grad).all())


# ---------------------------------------------------------------------------------------------
# inverse and sampling
@pytest.mark.parametrize("case", nc.CASES, ids=nc.case_id)
def test_inverse_undoes_forward(case):
    state, x = nc.case_inputs(case)
    model = _model_from(state, nc.kwargs(case))
    xd = x.to(DEV)
    with torch.no_grad():
        z = model._forward(xd)
        _close(model._inverse(z), x, f"{nc.case_id(case)} inverse(forward(x))")
        z0 = torch.randn(x.shape, generator=torch.Generator().manual_seed(1))
        _close(model._forward(model._inverse(z0.to(DEV))), z0, f"{nc.case_id(case)} forward(inverse(z))")
        assert model.forward(model._inverse(z0.to(DEV)))[0].shape == x.shape


def test_sample():
    case = (4, 16, 9, 2, 4)
    state, x = nc.case_inputs(case)
    model = _model_from(state, nc.kwargs(case))
    with pytest.raises(RuntimeError, match="shape"):
        model.sample(2)
    model(x.to(DEV))
    draws = []
    for seed in (11, 11, 12):
        gen = torch.Generator(device=DEV).manual_seed(seed)
        draws.append(model.sample(6, temp=0.7, generator=gen))
        assert tuple(draws[-1].shape) == (6, 1, 4, 4) and bool(torch.isfinite(draws[-1]).all())
    assert torch.equal(draws[0], draws[1]) and not torch.equal(draws[0], draws[2])
    gen = torch.Generator(device=DEV).manual_seed(11)
    noise = torch.randn((6, 1, 4, 4), device=DEV, generator=gen) * 0.7
    assert torch.equal(model._inverse(noise), draws[0])
    cold = model.sample(3, temp=0.0)
    want = model._inverse(torch.zeros(1, 1, 4, 4, device=DEV))
    assert all(torch.equal(cold[k], want[0]) for k in range(3))
    _close(want, nref.inverse(torch.zeros(1, 16), state).reshape(1, 1, 4, 4), "inverse(0)")


# ---------------------------------------------------------------------------------------------
# reproducibility, linearity, capture, sinks
@pytest.mark.parametrize("case", [nc.CAPTURE_CASE, (129, 258, 130, 2, 3), (8, 64, 1500, 1, 2)], ids=nc.case_id)
def test_bit_identical_runs_and_exact_linearity(case):
    from pytorch_generative_amd import ops

    state, x = nc.case_inputs(case)
    model = _model_from(state, nc.kwargs(case))
    xd = x.to(DEV)
    a, b = _step(model, xd), _step(model, xd)
    assert torch.equal(a[0], b[0]) and torch.equal(a[2]["loss"], b[2]["loss"])
    for k in a[3]:
        assert torch.equal(a[3][k], b[3][k]), k

    def grads_for(scale):
        for p in model.parameters():
            p.grad = None
        xin = xd.clone().requires_grad_(True)
        z, _ = model(xin)
        g = torch.randn(z.shape, generator=torch.Generator().manual_seed(2)).to(DEV)
        z.backward(g * scale)
        torch.cuda.synchronize()
        return [xin.grad.clone()] + [p.grad.clone() for k, p in model.named_parameters()]

    full, half = grads_for(1.0), grads_for(0.5)
    for f, h in zip(full, half):
        assert float(f.abs().max()) > 0 and torch.equal(f * 0.5, h)
    # the input gradient of the whole flow against float64
    g = torch.randn(x.shape, generator=torch.Generator().manual_seed(2))
    _, want_dx = nref.grads_from(x, state, g)
    _close(full[0], want_dx.reshape(x.shape), f"{nc.case_id(case)} dx")
    assert callable(ops.coupling)


def test_graphed_steps_equal_eager_bitwise_and_sinks_equal_plain_gradients():
    from pytorch_generative_amd import graph, optim, recipes

    case = nc.CAPTURE_CASE
    state, _ = nc.case_inputs(case)
    g = torch.Generator().manual_seed(5)
    xs = [torch.rand(65, 1, 7, 10, generator=g).to(DEV) for _ in range(4)]
    plain = _model_from(state, nc.kwargs(case))
    plain_grads = _step(plain, xs[0])[3]  # no sinks: autograd's param.grad protocol
    m1 = _model_from(state, nc.kwargs(case))
    m2 = copy.deepcopy(m1)
    o1, o2 = optim.FlatAdam(m1.parameters(), lr=LR), optim.FlatAdam(m2.parameters(), lr=LR)
    loss_fn = lambda x, preds: recipes.nice_loss(x, None, preds)  # noqa: E731
    step = graph.GraphedTrainStep(m2, o2, loss_fn, xs[0], preserve_state=True)
    for it, x in enumerate(xs):
        o1.zero_grad()
        loss_fn(x, m1(x))["loss"].backward()
        if it == 0:
            torch.cuda.synchronize()
            for k, p in m1.named_parameters():
                assert p.grad is p._pg_grad
                assert torch.equal(p.grad, plain_grads[k]), f"{k}: gradient in the sink differs from the plain one"
        o1.step()
        out = step(x)
        torch.cuda.synchronize()
        assert set(out) == {"loss", "prior_log_likelihood", "log_det_J"}
        for (k, p1), (_, p2) in zip(m1.named_parameters(), m2.named_parameters()):
            assert torch.equal(p1, p2), f"{k}: graph replay differs from the eager step"
            assert torch.equal(p1.grad, p2.grad), f"{k}: gradient of the graph replay differs from the eager step"
    assert float(m1.scaling.log_scale.grad.abs().max()) > 0 and float(m1.net[0].net[0].weight.grad.abs().max()) > 0


def test_errors():
    from pytorch_generative_amd import ops

    state, x = nc.case_inputs((3, 6, 5, 1, 3))
    model = _model_from(state, nc.kwargs((3, 6, 5, 1, 3)))
    layers = [(m.weight, m.bias) for m in model.net[0].net if isinstance(m, torch.nn.Linear)]
    xd = x.to(DEV)
    with pytest.raises(RuntimeError, match="cuda"):
        ops.coupling(x, layers, False)
    with pytest.raises(ValueError, match="F even"):
        ops.coupling(xd[:, :5].contiguous(), layers, False)
    with pytest.raises(ValueError, match="contiguous"):
        ops.coupling(xd.t().contiguous().t(), layers, False)
    with pytest.raises(ValueError, match="does not take"):
        ops.coupling(torch.zeros(3, 8, device=DEV), layers, False)
    with pytest.raises(ValueError, match="sign"):
        ops.coupling(xd, layers, False, sign=2)
    with pytest.raises(TypeError, match="float32"):
        ops.coupling(xd.double(), layers, False)
    with pytest.raises(RuntimeError, match="cuda"):
        ops.nice_scale(x, model.scaling.log_scale)
    with pytest.raises(RuntimeError, match="cuda"):
        ops.logistic_logprob(x)
    lib = _lib().load()
    out = (ctypes.c_longlong * 14)()
    assert lib.pg_dense_linear_plan(0, 4, 4, 0, out, 14) == -2 and ops.dense_linear_plan(0, 4, 4) is None


def test_reproduce_debug_loader(tmp_path):
    nice = nice_mod()

    class _Loader:
        def __iter__(self):
            g = torch.Generator().manual_seed(0)
            return iter([(torch.rand(2, 1, 28, 28, generator=g), torch.zeros(2))])

    t = nice.reproduce(n_epochs=1, n_gpus=1, log_dir=str(tmp_path), debug_loader=_Loader())
    assert t._epoch == 1 and t._step == 1 and t._use_graph
    assert os.path.exists(os.path.join(str(tmp_path), "trainer_state_1.ckpt"))
    assert all(torch.isfinite(p).all() for p in t.model.parameters())
    assert isinstance(t.model, nice.NICE) and tuple(t.model.net[0].net[0].weight.shape) == (1000, 392)
    assert tuple(t.model.sample(2).shape) == (2, 1, 28, 28)
