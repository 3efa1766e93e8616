"""GPU: ARD lengthscales and Matern kernels of the Gaussian process — ops.stationary_kernel in every form against float64, inside
marked buffers; ops.ard_mll_sums and ops.stationary_mll_sums against the float64 sums of tests/_gp_ard_ref.py, bit-identical over
two runs; the model on the "stationary" route (value, all 3 + d gradients, predict, an appended factor against a fresh one bit for
bit, a replayed graph, the Adam loop against the same loop in float64); and that the "se" route is what it was.

Gates: covariances max |got - want| <= 1e-4 max |want|; every sum 1e-4 of the sum of |terms|; the model's value, d/d std,
d/d noise_var and d/d value 1e-4 relative, every d/d l_c 1e-4 of sum |terms_c| / (2 l_c) (tests/test_gp_ard_cpu.py shows that this
is at most 1 % of the value on these inputs)."""

import functools
import math

import pytest
import torch
from torch import nn

import _gp_ard_ref as aref

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
OUT_TOL = 1e-4  # the project's output gate
MARK = 7.0      # what the memory around an operand holds: it must still hold it afterwards
STD, NOISE = 1.3, 0.25
COV_SIZES = (1, 63, 64, 65, 130)
COV_DIMS = (1, 3, 16, 17, 33, 70)
SUM_SIZES = (1, 2, 63, 64, 65, 130, 321)
SUM_DIMS = (1, 3, 16, 17, 64, 65, 130)
NU = {"matern32": 1.5, "matern52": 2.5}


def gp_mod():
    from pytorch_generative_amd.models import gaussian_process

    return gaussian_process


def _err(got, want, what, scale=None):
    scale = float(want.double().abs().max()) if scale is None else scale
    err = float((got.detach().double().cpu() - want.double()).abs().max()) / max(scale, 1e-30)
    print(f"[gp ard] {what}: {err:.3e}")
    return err


def _marked(t, extra):
    """A (rows, columns + extra) buffer of MARK on the device with t in its first columns; returns (buffer, the view of t)."""
    buf = torch.full((t.shape[0], t.shape[1] + extra), MARK)
    buf[:, :t.shape[1]] = t
    buf = buf.to(DEV)
    return buf, buf[:, :t.shape[1]]


# ---------------------------------------------------------------------------------------------
# 1. the covariance
@functools.lru_cache(maxsize=None)
def cov_case(d):
    """Two sets of 130 rows, one lengthscale per column and one shared, made once per d and not modified."""
    g = torch.Generator().manual_seed(40 + d)
    a, b = torch.randn(130, d, generator=g), torch.randn(130, d, generator=g)
    vector = ((0.7 + 1.3 * torch.rand(d, generator=g)) * math.sqrt(d)).float()
    return a, b, vector, float(torch.tensor(1.3 * math.sqrt(d), dtype=torch.float32))


def _lengthscales(d, ard):
    """(what the operator takes, what the float64 reference takes)."""
    _, _, vector, shared = cov_case(d)
    return (vector.to(DEV), vector) if ard else (shared, shared)


def _check_forms(d, kind, ard, route):
    """Every form of the covariance at every size against float64; returns the worst error."""
    from pytorch_generative_amd import ops

    a, b, _, _ = cov_case(d)
    ls_dev, ls_ref = _lengthscales(d, ard)
    want_sym = aref.covariance(a, a, STD, ls_ref, kind)
    want_cross = aref.covariance(a, b, STD, ls_ref, kind)
    abuf, aview = _marked(a, 2)
    bbuf, bview = _marked(b, 3)
    keep = (abuf.clone(), bbuf.clone())
    diag = float(torch.tensor(STD, dtype=torch.float32) ** 2 + torch.tensor(NOISE, dtype=torch.float32))
    kw = dict(kind=kind, route=route)
    worst = 0.0
    for n in COV_SIZES:
        x = aview[:n]
        want = want_sym[:n, :n].clone()
        want.diagonal().fill_(diag)
        out = torch.full((n, n + 5), MARK, device=DEV)
        got = ops.stationary_kernel(x, x, STD, ls_dev, NOISE, out=out[:, :n], **kw)
        assert got.data_ptr() == out.data_ptr() and bool((out[:, n:] == MARK).all())
        got = got.cpu()
        assert torch.equal(got, got.t()), "the mirrored form is not exactly symmetric"
        assert torch.equal(got.diagonal(), torch.full((n,), diag)), "the diagonal is not exactly std^2 + noise_var"
        worst = max(worst, _err(got, want, f"{kind} ard={ard} d={d} symmetric n={n}"))
        low = torch.full((n, n + 5), MARK, device=DEV)
        ops.stationary_kernel(x, x, STD, ls_dev, NOISE, out=low[:, :n], mirror=False, **kw)
        low = low.cpu()
        strict_upper = torch.triu(torch.ones(n, n, dtype=torch.bool), 1)
        assert bool((low[:, :n][strict_upper] == MARK).all()) and bool((low[:, n:] == MARK).all()), "the lower form wrote above the diagonal"
        assert torch.equal(torch.tril(low[:, :n]), torch.tril(got)), "the lower form and the mirrored form differ"
        for m in COV_SIZES:
            out = torch.full((n, m + 4), MARK, device=DEV)
            got = ops.stationary_kernel(x, bview[:m], STD, ls_dev, NOISE, out=out[:, :m], **kw)  # noise_var is not used
            assert bool((out[:, m:] == MARK).all())
            worst = max(worst, _err(got, want_cross[:n, :m], f"{kind} ard={ard} d={d} cross {n}x{m}"))
            if m >= n:  # rows m - n .. m of the symmetric (m, m) matrix: columns 0 .. their own, the diagonal exact
                lo = m - n
                out = torch.full((n, m + 4), MARK, device=DEV)
                ops.stationary_kernel(aview[lo:m], aview[:m], STD, ls_dev, NOISE, out=out[:, :m], diag_offset=lo, **kw)
                out = out.cpu()
                inside = torch.tril(torch.ones(n, m, dtype=torch.bool), lo)
                assert bool((out[:, :m][~inside] == MARK).all()) and bool((out[:, m:] == MARK).all())
                want = want_sym[lo:m, :m].clone()
                want.diagonal(lo).fill_(diag)
                assert torch.equal(out[:, :m].diagonal(lo), torch.full((n,), diag))
                worst = max(worst, _err(torch.where(inside, out[:, :m], torch.zeros(())), torch.where(inside, want, torch.zeros((), dtype=torch.float64)),
                                        f"{kind} ard={ard} d={d} rows {lo}..{m}", scale=float(want.abs().max())))
    torch.cuda.synchronize()
    assert torch.equal(abuf, keep[0]) and torch.equal(bbuf, keep[1])
    return worst


@pytest.mark.parametrize("ard", [False, True], ids=["shared", "ard"])
@pytest.mark.parametrize("kind", aref.KINDS)
@pytest.mark.parametrize("d", COV_DIMS)
def test_covariance_against_float64(d, kind, ard):
    """Measured on the MI355X, worst over the grid: 4.3e-7 of the maximum (Matern 5/2, ARD, d = 33, the MFMA route)."""
    from pytorch_generative_amd import ops

    assert ops.gp_plan(130, 130, d, 1)["se_route"] == int(d > 16)
    assert _check_forms(d, kind, ard, None) <= OUT_TOL


@pytest.mark.parametrize("route", ["direct", "mfma"])
@pytest.mark.parametrize("ard", [False, True], ids=["shared", "ard"])
@pytest.mark.parametrize("kind", aref.KINDS)
def test_covariance_forced_routes_at_d_16(kind, ard, route):
    assert _check_forms(16, kind, ard, route) <= OUT_TOL


@pytest.mark.parametrize("ard", [False, True], ids=["shared", "ard"])
@pytest.mark.parametrize("kind", aref.KINDS)
def test_duplicated_rows_give_exactly_std2_on_the_exact_difference_route(kind, ard):
    """Far from the origin too: the difference is formed first, then scaled."""
    from pytorch_generative_amd import ops

    for d, route in ((3, None), (16, None), (33, "direct")):
        a = (cov_case(d)[0] + 1000.0).clone()
        a[40] = a[5]
        x = a.to(DEV)
        ls_dev, _ = _lengthscales(d, ard)
        k = ops.stationary_kernel(x, x, STD, ls_dev, NOISE, kind=kind, route=route).cpu()
        std2 = float(torch.tensor(STD, dtype=torch.float32) ** 2)
        assert float(k[40, 5]) == std2 and float(k[5, 40]) == std2, (d, float(k[40, 5]))
        y = a.clone().to(DEV)
        cross = ops.stationary_kernel(x, y, STD, ls_dev, kind=kind, route=route).cpu()
        assert float(cross[40, 5]) == std2 and bool((cross.diagonal() == std2).all())
        assert bool(torch.isfinite(k).all())


@pytest.mark.parametrize("ard", [False, True], ids=["shared", "ard"])
@pytest.mark.parametrize("kind", aref.KINDS)
@pytest.mark.parametrize("d", [3, 33])
def test_an_element_depends_on_its_two_rows_alone(d, kind, ard):
    """The same two rows give the same bits inside an (n, m) of another size, at another place, in another form: the appended
    factor rests on that."""
    from pytorch_generative_amd import ops

    a, b, _, _ = cov_case(d)
    a, b = a.to(DEV), b.to(DEV)
    ls_dev, _ = _lengthscales(d, ard)
    big = ops.stationary_kernel(a, b, STD, ls_dev, kind=kind)
    for n, m in ((1, 1), (63, 65), (65, 130), (130, 1)):
        assert torch.equal(ops.stationary_kernel(a[:n], b[:m], STD, ls_dev, kind=kind), big[:n, :m]), (n, m)
    moved = ops.stationary_kernel(a[60:129], b[3:70], STD, ls_dev, kind=kind)
    assert torch.equal(moved, big[60:129, 3:70])
    sym = ops.stationary_kernel(a, a, STD, ls_dev, kind=kind)
    as_cross = ops.stationary_kernel(a, a.clone(), STD, ls_dev, kind=kind)
    assert torch.equal(torch.tril(sym, -1), torch.tril(as_cross, -1))
    rows = ops.stationary_kernel(a[65:130], a, STD, ls_dev, NOISE, kind=kind, diag_offset=65)
    assert torch.equal(torch.tril(rows, 64), torch.tril(sym[65:130], 64))
    if ard:  # the caller's cached reciprocal is the reciprocal the operator makes
        assert torch.equal(ops.stationary_kernel(a, b, STD, None, kind=kind, inv_lengthscale=ls_dev.reciprocal()), big)


# ---------------------------------------------------------------------------------------------
# 2. the reductions
@functools.lru_cache(maxsize=None)
def sums_case(n, d):
    g = torch.Generator().manual_seed(1000 * n + d)
    x = torch.randn(n, d, generator=g)
    h = torch.randn(n, n, generator=g)
    h = torch.tril(h) + torch.tril(h, -1).t()
    alpha_t = torch.randn(3, n, generator=g)
    vector = ((0.7 + 1.3 * torch.rand(d, generator=g)) * math.sqrt(d)).float()
    shared = float(torch.tensor(1.3 * math.sqrt(d), dtype=torch.float32))
    return x, h, alpha_t, vector, shared


def _lower_in_buffer(h, extra):
    """An (n, n + extra) buffer of MARK holding the lower triangle of h: MARK above the diagonal must not be read."""
    n = h.shape[0]
    tri = torch.tril(torch.ones(n, n, dtype=torch.bool))
    buf = torch.full((n, n + extra), MARK)
    buf[:, :n][tri] = h[tri]
    buf = buf.to(DEV)
    return buf, buf[:, :n]


def _check_sums(x, h, alpha_t, vector, shared, what):
    """Both reductions for the three kinds and p = 1, 3 on the given operands; returns the worst error of sum |terms|."""
    from pytorch_generative_amd import ops

    n, d = x.shape
    xbuf, xview = _marked(x, 2)
    hbuf, hview = _lower_in_buffer(h, 7)
    abuf, aview = _marked(alpha_t, 4)
    keep = [t.clone() for t in (xbuf, hbuf, abuf)]
    ls_dev = vector.to(DEV)
    terms = aref.scaled_sq_terms(x, x, vector)
    std32 = float(torch.tensor(STD, dtype=torch.float32))
    worst = 0.0
    for p in (1, 3):
        at = aview[:p]
        for kind in aref.KINDS:
            out = torch.full((d + 4,), MARK, device=DEV)
            got = ops.ard_mll_sums(xview, STD, ls_dev, hview, at, kind=kind, out=out[1:d + 3])
            again = ops.ard_mll_sums(xview, STD, ls_dev, hview, at, kind=kind)
            assert got.data_ptr() == out[1:].data_ptr() and float(out[0]) == MARK and float(out[-1]) == MARK
            assert torch.equal(got, again), "two runs of the ARD reduction differ"
            want, sizes = aref.ard_sums(x, std32, vector, h, alpha_t[:p], kind, terms=terms)
            got = got.double().cpu()
            assert bool(torch.isfinite(got).all())
            errs = (got - want).abs() / sizes.clamp_min(1e-30)
            k = int(errs.argmax())
            print(f"[gp ard] {what} p={p} {kind} ard sums: {float(errs[k]):.3e} of sum |terms| at entry {k} of {d + 2}")
            worst = max(worst, float(errs[k]))
            if n == 1:
                assert bool((got[2:] == 0.0).all())  # one point: every difference is 0 exactly
            got = ops.stationary_mll_sums(xview, STD, shared, hview, at, kind=kind, out=out[:3])
            again = ops.stationary_mll_sums(xview, STD, shared, hview, at, kind=kind)
            assert torch.equal(got, again), "two runs of the shared-lengthscale reduction differ"
            if kind == "se":
                assert torch.equal(got, ops.se_mll_sums(xview, STD, shared, hview, at)), "kind se is not se_mll_sums"
            want, sizes = aref.stat_sums(x, std32, shared, h, alpha_t[:p], kind)
            got = got.double().cpu()
            assert bool(torch.isfinite(got).all())
            errs = (got - want).abs() / sizes.clamp_min(1e-30)
            print(f"[gp ard] {what} p={p} {kind} shared sums: {[f'{float(e):.3e}' for e in errs]}")
            worst = max(worst, float(errs.max()))
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(keep, (xbuf, hbuf, abuf)))
    return worst


@pytest.mark.parametrize("d", SUM_DIMS)
@pytest.mark.parametrize("n", SUM_SIZES)
def test_sums_against_float64(n, d):
    """Measured on the MI355X, worst over the grid: the ARD sums 7.1e-7 of sum |terms| (n = 2, d = 130, Matern 3/2), the
    shared-lengthscale sums 5.0e-7 (n = 2, d = 65, Matern 3/2, d/d lengthscale on the MFMA route)."""
    from pytorch_generative_amd import ops

    plan = ops.gp_ard_plan(n, d, 3)
    assert plan["column_chunks"] == -(-d // 64) and plan["partial_row_floats"] == d + 2
    assert _check_sums(*sums_case(n, d), f"n={n} d={d}") <= OUT_TOL


@pytest.mark.parametrize("d", [3, 17, 70])
def test_sums_with_a_duplicated_row_pair(d):
    """r = 0 off the diagonal: omega is finite there, and the MFMA route's clamped distance may be a rounding above 0."""
    x, h, alpha_t, vector, shared = sums_case(65, d)
    x = x.clone()
    x[40] = x[5]
    assert _check_sums(x, h, alpha_t, vector, shared, f"duplicate rows d={d}") <= OUT_TOL


def test_ard_sums_refuses_what_the_plan_refuses():
    from pytorch_generative_amd import ops

    x = torch.zeros(4, 257, device=DEV)
    h, at = torch.eye(4, device=DEV), torch.zeros(1, 4, device=DEV)
    with pytest.raises(ValueError, match="256"):
        ops.ard_mll_sums(x, 1.0, torch.ones(257, device=DEV), h, at)
    with pytest.raises(ValueError, match="3.*4 columns|shape"):
        ops.ard_mll_sums(x[:, :4], 1.0, torch.ones(3, device=DEV), h, at)
    with pytest.raises(ValueError, match="kind"):
        ops.stationary_kernel(x, x, 1.0, 1.0, kind="matern12")


# ---------------------------------------------------------------------------------------------
# 3. the model
def _kernel(kind, std, lengthscale):
    gp = gp_mod()
    std = nn.Parameter(torch.tensor(std))
    lengthscale = nn.Parameter(lengthscale.clone() if torch.is_tensor(lengthscale) else torch.tensor(lengthscale))
    return gp.SquaredExponential(std, lengthscale) if kind == "se" else gp.Matern(NU[kind], std, lengthscale)


def _model(kind, lengthscale, std=aref.STD, noise_var=aref.NOISE_VAR, value=aref.VALUE):
    gp = gp_mod()
    model = gp.GaussianProcess(gp.Const(nn.Parameter(torch.tensor(value))), _kernel(kind, std, lengthscale), noise_var=noise_var).to(DEV)
    model.noise_var.requires_grad_()
    return model


def _value_and_grads(model):
    tensors = {"std": model.kernel.std, "lengthscale": model.kernel.lengthscale, "noise_var": model.noise_var, "value": model.mean.value}
    for t in tensors.values():
        t.grad = None
    value = model.log_marginal_likelihood()
    value.backward()
    return value.detach(), {name: t.grad for name, t in tensors.items()}


def _rel(got, want, what):
    got, want = float(got), float(want)
    err = abs(got - want) / abs(want) if want != 0.0 else abs(got)
    print(f"[gp ard] {what}: {err:.3e} (want {want:.6g})")
    return err


HYPER32 = tuple(float(torch.tensor(v, dtype=torch.float32)) for v in (aref.STD, aref.NOISE_VAR, aref.VALUE))


def _check_model(model, x, y, lengthscale, kind, what):
    value, grads = _value_and_grads(model)
    want, want_grads, sizes = aref.closed_form(x, y, HYPER32[0], lengthscale, HYPER32[1], HYPER32[2], kind)
    assert value.shape == () and value.dtype == torch.float32 and value.is_cuda
    assert grads["lengthscale"].shape == model.kernel.lengthscale.shape
    errs = [_rel(value, want, f"{what} value")]
    errs += [_rel(grads[name], want_grads[name], f"{what} d/d {name}") for name in ("std", "noise_var", "value")]
    err_ls = (grads["lengthscale"].double().cpu() - want_grads["lengthscale"]).abs() / sizes.clamp_min(1e-30)
    print(f"[gp ard] {what} d/d lengthscale: worst {float(err_ls.max()):.3e} of sum |terms_c| / (2 l_c); worst relative "
          f"{float(((grads['lengthscale'].double().cpu() - want_grads['lengthscale']).abs() / want_grads['lengthscale'].abs().clamp_min(1e-300)).max()):.3e}")
    assert max(errs) <= OUT_TOL and float(err_ls.max()) <= OUT_TOL
    with torch.no_grad():
        assert torch.equal(model.log_marginal_likelihood(), value)
    return value, grads


@pytest.mark.parametrize("kind", ["matern32", "matern52", "se"])
@pytest.mark.parametrize("n,d,p", aref.MODEL_SHAPES)
def test_model_against_float64(n, d, p, kind):
    """Measured on the MI355X, worst over the cases: a d/d l_c 5.2e-8 of sum |terms_c| / (2 l_c) and 9.3e-7 relative (Matern 5/2 at
    (130, 33, 3)), the value and the other gradients 1.5e-6 relative (d/d std, Matern 3/2 at (64, 2, 2))."""
    x, y, lengthscale = aref.model_case(kind, n, d, p)
    model = _model(kind, lengthscale)
    assert model._kernel_route == "stationary"
    model.fit(x.to(DEV), y.to(DEV))
    _check_model(model, x, y, lengthscale, kind, f"model {kind} n={n} d={d} p={p}")
    assert model._factor_route == "full"


@pytest.mark.parametrize("kind", ["matern32", "matern52"])
@pytest.mark.parametrize("n,d,p", [(65, 2, 1), (321, 17, 1)])
def test_model_with_one_shared_lengthscale_against_float64(n, d, p, kind):
    x, y, _ = aref.model_case(kind, n, d, p)
    shared = float(torch.tensor(0.8 * math.sqrt(d), dtype=torch.float32))
    model = _model(kind, shared)
    assert model._kernel_route == "stationary" and model.kernel.lengthscale.shape == ()
    model.fit(x.to(DEV), y.to(DEV))
    _check_model(model, x, y, shared, kind, f"model {kind} shared n={n} d={d} p={p}")


@pytest.mark.parametrize("kind,ard", [("se", True), ("matern32", False), ("matern32", True), ("matern52", False), ("matern52", True)])
def test_predict_against_the_float64_posterior(kind, ard):
    """The "stationary" route at the gates of tests/test_gpu_gp.py (a shared-lengthscale squared exponential is the "se" route)."""
    x, y, lengthscale = aref.model_case(kind, 130, 3, 2)
    if not ard:
        lengthscale = float(lengthscale[0])
    g = torch.Generator().manual_seed(77)
    q = torch.randn(70, 3, generator=g)
    model = _model(kind, lengthscale)
    prior_mu, prior_sig = model.predict(q.to(DEV))
    assert _err(prior_sig, aref.covariance(q, q, HYPER32[0], lengthscale, kind), f"prior {kind} ard={ard}") <= OUT_TOL
    assert torch.equal(prior_mu.cpu(), torch.full((70, 1), HYPER32[2]))
    model.fit(x.to(DEV), y.to(DEV))
    mu, sig = model.predict(q.to(DEV))
    want_mu, want_sig = aref.posterior(x, y, q, HYPER32[0], lengthscale, HYPER32[2], HYPER32[1], kind)
    assert mu.shape == (70, 2) and torch.equal(sig, sig.t())
    assert _err(mu, want_mu, f"predict {kind} ard={ard} mu") <= OUT_TOL
    assert _err(sig, want_sig, f"predict {kind} ard={ard} sig", scale=HYPER32[0] ** 2) <= OUT_TOL
    # sample() takes its jitter scale std^2 on this route too
    single = _model(kind, lengthscale)
    single.fit(x.to(DEV), y[:, :1].to(DEV))
    draws = single.sample(q[:20].to(DEV), 3, generator=torch.Generator(device=DEV).manual_seed(1))
    assert draws.shape == (3, 20) and bool(torch.isfinite(draws).all())
    factor = single._sample_factor.double().cpu()
    target = single.predict(q[:20].to(DEV))[1].double().cpu() + single._sample_jitter * HYPER32[0] ** 2 * torch.eye(20, dtype=torch.float64)
    assert _err(factor @ factor.t(), target, f"sample {kind} ard={ard}: L_s L_s^T against sig + jitter std^2", scale=HYPER32[0] ** 2) <= OUT_TOL


@pytest.mark.parametrize("kind", ["matern52", "se"])
def test_after_an_append_the_bits_of_a_fresh_model(kind):
    x, y, lengthscale = aref.model_case(kind, 130, 3, 2)
    q = torch.randn(40, 3, generator=torch.Generator().manual_seed(5)).to(DEV)
    x, y = x.to(DEV), y.to(DEV)
    grown = _model(kind, lengthscale)
    grown.fit(x[:65], y[:65])
    first = grown.log_marginal_likelihood()
    grown.fit(x[65:], y[65:])
    value, grads = _value_and_grads(grown)
    assert grown._factor_route == "append" and not torch.equal(first.detach(), value)
    mu, sig = grown.predict(q)
    fresh = _model(kind, lengthscale)
    fresh.fit(x, y)
    want, want_grads = _value_and_grads(fresh)
    assert fresh._factor_route == "full"
    want_mu, want_sig = fresh.predict(q)
    assert torch.equal(torch.tril(grown._factor[:130, :130]), torch.tril(fresh._factor[:130, :130]))
    assert torch.equal(mu, want_mu) and torch.equal(sig, want_sig) and torch.equal(value, want)
    for name in aref.NAMES:
        assert torch.equal(grads[name], want_grads[name]), name
    # an in-place change of one lengthscale makes the factor afresh, and then it appends again
    with torch.no_grad():
        grown.kernel.lengthscale[1] *= 1.5
    more = torch.randn(2, 3, generator=torch.Generator().manual_seed(6)).to(DEV)
    grown.fit(more[:1], y[:1])
    changed_mu, _ = grown.predict(q)
    assert grown._factor_route == "full" and not torch.equal(changed_mu, mu)
    grown.fit(more[1:], y[1:2])
    grown.predict(q)
    assert grown._factor_route == "append"


def test_predict_replays_in_a_graph_with_identical_bits():
    x, y, lengthscale = aref.model_case("matern52", 130, 33, 3)
    model = _model("matern52", lengthscale)
    model.fit(x.to(DEV), y.to(DEV))
    q = torch.randn(70, 33, generator=torch.Generator().manual_seed(8)).to(DEV)
    mu, sig = model.predict(q)  # makes the factor; from here on predict does not synchronise
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        model.predict(q)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        mu_g, sig_g = model.predict(q)
    for _ in range(2):
        mu_g.zero_()
        sig_g.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(mu_g, mu) and torch.equal(sig_g, sig)


def test_optimize_hyperparameters_follows_the_float64_loop_and_finds_the_irrelevant_column():
    """n = 130, d = 3, Matern 5/2 with one lengthscale per column, 30 steps from all ones; the third column is pure noise."""
    x, y = aref.relevance_case()
    start = (1.0, (1.0, 1.0, 1.0), 1.0, 0.0)
    ref_seen, ref_final = aref.adam_loop(x, y, start, "matern52", n_steps=30, lr=0.05)
    gp = gp_mod()
    model = gp.GaussianProcess(gp.Const(), gp.Matern(2.5, n_dims=3), noise_var=1.0).to(DEV)
    model.fit(x.to(DEV), y.to(DEV))
    seen = model.optimize_hyperparameters(30, 0.05)
    final = (float(model.kernel.std.detach()), tuple(model.kernel.lengthscale.detach().tolist()), float(model.noise_var), float(model.mean.value.detach()))
    at_start = float(aref.log_evidence(x, y, *start, "matern52"))
    at_final = float(aref.log_evidence(x, y, *final, "matern52"))
    at_ref = float(aref.log_evidence(x, y, *ref_final, "matern52"))
    print(f"[gp ard] optimise: start {at_start:.4f}, reached {at_final:.6f}, float64 loop {at_ref:.6f}; final {final}, float64 {ref_final}")
    print(f"[gp ard]   the values seen differ from the float64 loop's by at most {max(abs(a - b) / abs(b) for a, b in zip(seen, ref_seen)):.3e}")
    assert len(seen) == 30 and abs(seen[0] - at_start) <= OUT_TOL * abs(at_start)
    assert at_ref > at_start and at_final >= at_ref - OUT_TOL * (at_ref - at_start)
    assert final[1][2] > max(final[1][:2]) and ref_final[1][2] > max(ref_final[1][:2])
    model.predict(x[:10].to(DEV))
    assert model._factor_route == "full"


# ---------------------------------------------------------------------------------------------
# 4. the "se" route is what it was
def test_scalar_squared_exponential_keeps_the_se_route_and_its_bits():
    from pytorch_generative_amd import ops

    gp = gp_mod()
    g = torch.Generator().manual_seed(12)
    x = (4.0 * torch.rand(130, 3, generator=g)).to(DEV)
    y = torch.sin(x.sum(1, keepdim=True)) + 0.3 * torch.randn(130, 1, generator=g).to(DEV)
    q = (4.0 * torch.rand(70, 3, generator=g)).to(DEV)
    std, lengthscale, noise, value = 1.3, 0.7, 0.1, 0.2
    model = gp.GaussianProcess(gp.Const(nn.Parameter(torch.tensor(value))),
                               gp.SquaredExponential(nn.Parameter(torch.tensor(std)), nn.Parameter(torch.tensor(lengthscale))), noise).to(DEV)
    model.noise_var.requires_grad_()
    assert model._kernel_route == "se"
    model.fit(x, y)
    mu, sig = model.predict(q)
    got_value, grads = _value_and_grads(model)
    std, lengthscale, noise, value = (float(torch.tensor(v, dtype=torch.float32)) for v in (std, lengthscale, noise, value))
    # the same through the entry points the route has always called
    lower = torch.zeros(130, 130, device=DEV)
    ops.se_kernel(x, x, std, lengthscale, noise, out=lower, mirror=False)
    assert int(ops.cholesky_(lower)) == 0
    zt = (y - value).t().contiguous()
    ops.trsm_right_(lower, zt)
    alpha_t = zt.clone()
    ops.trsm_right_(lower, alpha_t, transposed=True)
    w = ops.se_kernel(q, x, std, lengthscale)
    want_mu = torch.full((70, 1), value, device=DEV)
    ops.gemm_nt_(want_mu, w, alpha_t, add=True)
    ops.trsm_right_(lower, w)
    want_sig = ops.se_kernel(q, q, std, lengthscale, mirror=False)
    ops.gemm_nt_(want_sig, w, w, lower=True, mirror=True)
    assert torch.equal(mu, want_mu) and torch.equal(sig, want_sig)
    both = ops.mll_value(lower, zt, alpha_t)
    precision = torch.empty(130, 130, device=DEV)
    ops.gram_upper_(precision, ops.tri_inverse_t(lower))
    sums = ops.se_mll_sums(x, std, lengthscale, precision, alpha_t)
    assert torch.equal(got_value, both[0]) and torch.equal(grads["value"], both[1])
    for k, name in enumerate(("std", "lengthscale", "noise_var")):
        assert torch.equal(grads[name], sums[k]), name
    # and the SE, shared-lengthscale instantiation of the new entry points is the old entry point
    for a, b in ((x, x), (q, x)):
        assert torch.equal(ops.stationary_kernel(a, b, std, lengthscale, noise, kind="se"), ops.se_kernel(a, b, std, lengthscale, noise))
    wide = torch.randn(130, 40, generator=torch.Generator().manual_seed(3)).to(DEV)
    assert torch.equal(ops.stationary_kernel(wide, wide, std, 3.0, kind="se"), ops.se_kernel(wide, wide, std, 3.0))
    assert torch.equal(ops.stationary_mll_sums(x, std, lengthscale, precision, alpha_t, kind="se"), sums)
