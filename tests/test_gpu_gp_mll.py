"""GPU: the marginal likelihood of the Gaussian process on the kernels of csrc/gp_mll.hip — the triangular inverse and the
product X X^T against float64 from the same fp32 operands, inside marked buffers; the fused reduction against float64 sums,
bit-identical over two runs; the model's value and its four gradients against the float64 closed forms of tests/_gp_mll_ref.py;
an appended factor against a fresh one, bit for bit; the Adam loop against the same loop in float64.

Gates: matrices max |got - want| <= 1e-4 max |want|; the sums 1e-4 of the sum of |terms|; the model 1e-4 relative."""

import functools

import pytest
import torch
from torch import nn

import _gp_mll_ref as mref
import _gp_ref as gref

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
OUT_TOL = 1e-4  # the project's output gate
MARK = 7.0      # what the memory around an operand holds: it must still hold it afterwards
SIZES = (1, 2, 63, 64, 65, 130, 321)
START = (1.3, 0.7, 0.1, 0.2)  # std, lengthscale, noise_var, value


def gp_mod():
    from pytorch_generative_amd.models import gaussian_process

    return gaussian_process


def _err(got, want, what, scale=None):
    scale = float(want.double().abs().max()) if scale is None else scale
    err = float((got.detach().double().cpu() - want.double()).abs().max()) / max(scale, 1e-30)
    print(f"[gp mll] {what}: {err:.3e}")
    return err


@functools.lru_cache(maxsize=None)
def factor_case(n):
    """The float32 rounding of the float64 factor of A = B B^T / n + I (cond <= 5.1), its float64 inverse transposed X and the
    float32 rounding of X: made once per n and not modified."""
    l = gref.cholesky(gref.spd(n, 100 + n)).float()
    x = mref.tri_inverse_t(l)
    return l, x, x.float()


def _in_buffer(matrix, ld, upper):
    """An (n, ld) buffer of MARK holding the lower (upper) triangle of the (n, n) matrix; returns (buffer, the (n, n) view, the
    mask of the matrix's own triangle inside the buffer)."""
    n = matrix.shape[0]
    tri = torch.ones(n, n, dtype=torch.bool)
    tri = torch.triu(tri) if upper else torch.tril(tri)
    buf = torch.full((n, ld), MARK)
    buf[:, :n][tri] = matrix[tri]
    own = torch.zeros(n, ld, dtype=torch.bool)
    own[:, :n] = tri
    buf = buf.to(DEV)
    return buf, buf[:, :n], own.to(DEV)


# ---------------------------------------------------------------------------------------------
# 1. the inverse and the product
@pytest.mark.parametrize("n", SIZES)
def test_inverse_against_float64(n):
    """Measured on the MI355X, worst over these sizes (n = 321): 8.3e-8 of the maximum, X L^T - I 9.1e-8."""
    from pytorch_generative_amd import ops

    l, want, _ = factor_case(n)
    lbuf, lview, lown = _in_buffer(l, n + 5, upper=False)
    xbuf = torch.full((n, n + 11), MARK, device=DEV)
    xown = torch.zeros(n, n + 11, dtype=torch.bool)
    xown[:, :n] = torch.triu(torch.ones(n, n, dtype=torch.bool))
    xown = xown.to(DEV)
    out = ops.tri_inverse_t(lview, out=xbuf[:, :n])
    torch.cuda.synchronize()
    assert out.data_ptr() == xbuf.data_ptr()
    assert bool((xbuf[~xown] == MARK).all()), "the strict lower triangle of x or the memory beside it was written"
    assert bool((lbuf[~lown] == MARK).all()) and torch.equal(torch.tril(lview).cpu(), l)
    got = torch.triu(xbuf[:, :n]).cpu()
    assert _err(got, want, f"inverse n={n}") <= OUT_TOL
    assert _err(got.double() @ l.double().t(), torch.eye(n, dtype=torch.float64), f"X L^T n={n}") <= OUT_TOL
    again = torch.full((n, n + 11), MARK, device=DEV)
    ops.tri_inverse_t(lview, out=again[:, :n])
    assert torch.equal(again, xbuf), "two runs of the inverse differ"
    made = ops.tri_inverse_t(lview)  # no `out`: the triangular matrix itself
    assert torch.equal(made.cpu(), got)


@pytest.mark.parametrize("mirror", [False, True], ids=["lower", "mirrored"])
@pytest.mark.parametrize("n", SIZES)
def test_gram_against_float64(n, mirror):
    """Measured on the MI355X, worst over these sizes (n = 321): 1.3e-6 of the maximum."""
    from pytorch_generative_amd import ops

    _, _, x = factor_case(n)
    want = mref.gram_upper(x)
    xbuf, xview, xown = _in_buffer(x, n + 3, upper=True)  # MARK below the diagonal: it must not be read
    hbuf = torch.full((n, n + 9), MARK, device=DEV)
    out = ops.gram_upper_(hbuf[:, :n], xview, mirror=mirror)
    torch.cuda.synchronize()
    assert out.data_ptr() == hbuf.data_ptr()
    assert torch.equal(xbuf, _in_buffer(x, n + 3, upper=True)[0]) and bool((hbuf[:, n:] == MARK).all())
    got = hbuf[:, :n].cpu()
    if mirror:
        assert torch.equal(got, got.t())
    else:
        strict_upper = torch.triu(torch.ones(n, n, dtype=torch.bool), 1)
        assert bool((got[strict_upper] == MARK).all()), "the strict upper triangle of h was written"
    assert _err(torch.tril(got), torch.tril(want), f"gram n={n} mirror={mirror}") <= OUT_TOL
    again = torch.full((n, n + 9), MARK, device=DEV)
    ops.gram_upper_(again[:, :n], xview, mirror=mirror)
    assert torch.equal(again, hbuf), "two runs of the product differ"


# ---------------------------------------------------------------------------------------------
# 2. the reduction
@functools.lru_cache(maxsize=None)
def sums_case(n, d, p):
    g = torch.Generator().manual_seed(1000 * n + 10 * d + p)
    x = 4.0 * torch.rand(n, d, generator=g)
    h = torch.randn(n, n, generator=g)
    h = torch.tril(h) + torch.tril(h, -1).t()
    alpha_t = torch.randn(p, n, generator=g)
    lengthscale = 0.7 if d <= 3 else 3.0
    want, sizes = mref.se_sums(x, 1.3, lengthscale, h, alpha_t)
    return x, h, alpha_t, lengthscale, want, sizes


@pytest.mark.parametrize("p", [1, 3])
@pytest.mark.parametrize("d", [1, 3, 16, 17, 40])
@pytest.mark.parametrize("n", SIZES)
def test_sums_against_float64(n, d, p):
    """Measured on the MI355X, worst over the grid: 2.9e-6 of sum |terms| (n = 2, d = 40, p = 3, d/d lengthscale: the MFMA
    route's |a|^2 + |b|^2 - 2 a.b, as in se_kernel)."""
    from pytorch_generative_amd import ops

    x, h, alpha_t, lengthscale, want, sizes = sums_case(n, d, p)
    assert ops.gp_mll_plan(n, d, p)["se_route"] == int(d > 16)
    xbuf = torch.full((n, d + 2), MARK, device=DEV)
    xbuf[:, :d] = x.to(DEV)
    hbuf, hview, hown = _in_buffer(h, n + 7, upper=False)  # MARK above the diagonal: it must not be read
    abuf = torch.full((p, n + 4), MARK, device=DEV)
    abuf[:, :n] = alpha_t.to(DEV)
    keep = [b.clone() for b in (xbuf, hbuf, abuf)]
    out = torch.full((5,), MARK, device=DEV)
    got = ops.se_mll_sums(xbuf[:, :d], 1.3, lengthscale, hview, abuf[:, :n], out=out[1:4])
    again = ops.se_mll_sums(xbuf[:, :d], 1.3, lengthscale, hview, abuf[:, :n])
    torch.cuda.synchronize()
    assert got.data_ptr() == out[1:4].data_ptr() and float(out[0]) == MARK and float(out[4]) == MARK
    assert all(torch.equal(a, b) for a, b in zip(keep, (xbuf, hbuf, abuf)))
    assert torch.equal(got, again), "two runs of the reduction differ"
    for k, name in enumerate(("std", "lengthscale", "noise_var")):
        err = abs(float(got[k]) - float(want[k])) / max(float(sizes[k]), 1e-30)
        print(f"[gp mll] sums n={n} d={d} p={p} d/d {name}: {err:.3e} of sum |terms| (want {float(want[k]):.4g})")
        assert err <= OUT_TOL, name
    if n == 1:
        assert float(got[1]) == 0.0  # one point: D2 = 0 exactly


@pytest.mark.parametrize("n,p", [(1, 1), (65, 3), (321, 2)])
def test_value_against_float64(n, p):
    from pytorch_generative_amd import ops

    l = factor_case(n)[0]
    g = torch.Generator().manual_seed(n + p)
    zt, alpha_t = torch.randn(p, n, generator=g), torch.randn(p, n, generator=g)
    want = mref.value_sums(l, zt, alpha_t)
    lbuf, lview, _ = _in_buffer(l, n + 5, upper=False)
    zbuf = torch.full((p, n + 3), MARK, device=DEV)
    zbuf[:, :n] = zt.to(DEV)
    abuf = torch.full((p, n + 8), MARK, device=DEV)
    abuf[:, :n] = alpha_t.to(DEV)
    got = ops.mll_value(lview, zbuf[:, :n], abuf[:, :n])
    assert torch.equal(got, ops.mll_value(lview, zbuf[:, :n], abuf[:, :n]))
    assert abs(float(got[0]) - float(want[0])) <= OUT_TOL * abs(float(want[0]))
    assert abs(float(got[1]) - float(want[1])) <= OUT_TOL * float(alpha_t.double().abs().sum())


# ---------------------------------------------------------------------------------------------
# 3. the model
def _data(n, d, p, seed):
    g = torch.Generator().manual_seed(seed)
    x = 4.0 * torch.rand(n, d, generator=g)
    y = torch.sin(x.sum(1, keepdim=True)) + 0.3 * torch.randn(n, p, generator=g)
    return x, y


def _model(std, lengthscale, noise_var, value):
    gp = gp_mod()
    model = gp.GaussianProcess(gp.Const(nn.Parameter(torch.tensor(value))),
                               gp.SquaredExponential(nn.Parameter(torch.tensor(std)), nn.Parameter(torch.tensor(lengthscale))),
                               noise_var=noise_var).to(DEV)
    model.noise_var.requires_grad_()
    return model


def _value_and_grads(model):
    for t in (model.kernel.std, model.kernel.lengthscale, model.noise_var, model.mean.value):
        t.grad = None
    value = model.log_marginal_likelihood()
    value.backward()
    return value.detach(), {"std": model.kernel.std.grad, "lengthscale": model.kernel.lengthscale.grad, "noise_var": model.noise_var.grad,
                            "value": model.mean.value.grad}


def _rel(got, want, what):
    got, want = float(got), float(want)
    if want == 0.0:
        print(f"[gp mll] {what}: want 0, got {got:g}")
        return abs(got)
    err = abs(got - want) / abs(want)
    print(f"[gp mll] {what}: {err:.3e} (want {want:.6g})")
    return err


@pytest.mark.parametrize("n,d,p,lengthscale", [(1, 1, 1, 0.7), (2, 1, 1, 0.7), (63, 2, 1, 0.7), (64, 2, 2, 0.7), (65, 2, 1, 0.7), (130, 3, 1, 0.7),
                                               (321, 2, 3, 0.7), (321, 20, 1, 3.0)])
def test_model_against_float64(n, d, p, lengthscale):
    """Measured on the MI355X, worst relative error over the cases: 1.9e-5 (d/d std at (321, 2, 3)); the value 4.0e-7 at most."""
    x, y = _data(n, d, p, seed=7 * n + d + p)
    hyper = (START[0], lengthscale, START[2], START[3])
    model = _model(*hyper)
    model.fit(x.to(DEV), y.to(DEV))
    value, grads = _value_and_grads(model)
    hyper32 = tuple(float(torch.tensor(v, dtype=torch.float32)) for v in hyper)
    want, want_grads = mref.closed_form(x, y, *hyper32)
    assert value.shape == () and value.dtype == torch.float32 and value.is_cuda
    errs = [_rel(value, want, f"model n={n} d={d} p={p} value")]
    errs += [_rel(grads[name], want_grads[name], f"model n={n} d={d} p={p} d/d {name}") for name in mref.NAMES]
    assert max(errs) <= OUT_TOL
    with torch.no_grad():
        assert torch.equal(model.log_marginal_likelihood(), value) and model._factor_route == "full"


def test_after_an_append_the_bits_of_a_fresh_model():
    x, y = _data(130, 2, 1, seed=11)
    x, y = x.to(DEV), y.to(DEV)
    grown = _model(*START)
    grown.fit(x[:65], y[:65])
    first = grown.log_marginal_likelihood()
    grown.fit(x[65:], y[65:])
    value, grads = _value_and_grads(grown)
    assert grown._factor_route == "append" and not torch.equal(first.detach(), value)
    fresh = _model(*START)
    fresh.fit(x, y)
    want, want_grads = _value_and_grads(fresh)
    assert fresh._factor_route == "full"
    assert torch.equal(value, want)
    for name in mref.NAMES:
        assert torch.equal(grads[name], want_grads[name]), name


def test_optimize_hyperparameters_follows_the_float64_loop():
    """n = 130, d = 2, y drawn from the float64 process with (1.3, 0.7, 0.1, mean 0.2); start all ones and mean 0."""
    g = torch.Generator().manual_seed(2024)
    x = 4.0 * torch.rand(130, 2, generator=g)
    cov = gref.se(x, x, START[0], START[1]) + START[2] * torch.eye(130, dtype=torch.float64)
    y = (START[3] + gref.cholesky(cov) @ torch.randn(130, 1, generator=g, dtype=torch.float64)).float()
    start = (1.0, 1.0, 1.0, 0.0)
    ref_seen, ref_final = mref.adam_loop(x, y, start, n_steps=50, lr=0.05)

    gp = gp_mod()
    model = gp.GaussianProcess(gp.Const(), gp.SquaredExponential(), noise_var=1.0).to(DEV)
    model.fit(x.to(DEV), y.to(DEV))
    seen = model.optimize_hyperparameters(50, 0.05)
    final = tuple(float(t.detach()) for t in (model.kernel.std, model.kernel.lengthscale, model.noise_var, model.mean.value))
    at_start = float(mref.log_evidence(x, y, *start))
    at_final = float(mref.log_evidence(x, y, *final))
    at_ref = float(mref.log_evidence(x, y, *ref_final))
    print(f"[gp mll] optimise: start {at_start:.4f}, reached {at_final:.6f}, float64 loop {at_ref:.6f}; final {final}, float64 {ref_final}")
    assert len(seen) == 50 and abs(seen[0] - at_start) <= OUT_TOL * abs(at_start)
    print(f"[gp mll]   the values seen differ from the float64 loop's by at most {max(abs(a - b) / abs(b) for a, b in zip(seen, ref_seen)):.3e}")
    assert at_final > at_start
    assert abs(at_final - at_ref) <= OUT_TOL * abs(at_ref)
    for k, name in enumerate(("std", "lengthscale", "noise_var")):
        err = abs(torch.tensor(final[k]).log() - torch.tensor(ref_final[k]).log())
        print(f"[gp mll]   log {name}: {float(err):.3e}")
        assert err <= 1e-3, name
    assert abs(final[3] - ref_final[3]) <= 1e-3
    # a predict afterwards serves the new hyperparameters from a factor made afresh
    q = 4.0 * torch.rand(40, 2, generator=g)
    mu, sig = model.predict(q.to(DEV))
    assert model._factor_route == "full"
    want_mu, want_sig = gref.posterior(x, y, q, final[0], final[1], final[3], final[2])
    assert _err(mu, want_mu, "predict after optimise: mu") <= OUT_TOL
    assert _err(sig, want_sig, "predict after optimise: sig", scale=float(gref.se(q, q, final[0], final[1]).abs().max())) <= OUT_TOL
