"""GPU: the Gaussian process on the kernels of csrc/gp.hip — the blocked Cholesky factorisation, both triangular solves and the
squared-exponential covariance against the float64 closed forms of tests/_gp_ref.py; the appended factorisation and the solve
that completes columns against the full ones, bit for bit; the failed pivot; the model against the reference fixture
(tests/golden/gp/cases.pt) and against float64; graph replay; sampling.

Gates: outputs max |got - want| <= 1e-4 max |want|; the posterior covariance, a difference that cancels, against
max |kernel(x, x)|."""

import functools
import os

import numpy as np
import pytest
import torch

import _gp_ref as gref
import _util

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
CASES = os.path.join(_util.GOLDEN_DIR, "gp", "cases.pt")
OUT_TOL = 1e-4  # the project's output gate
MARK = 7.0      # what the memory around an operand holds: it must still hold it afterwards
FACTOR_N = (1, 2, 63, 64, 65, 130, 321)


def load_cases():
    return torch.load(CASES, map_location="cpu", weights_only=False)["cases"]


def gp_mod():
    from pytorch_generative_amd.models import gaussian_process

    return gaussian_process


def _err(got, want, what, scale=None):
    scale = float(want.double().abs().max()) if scale is None else scale
    err = float((got.detach().double().cpu() - want.double()).abs().max()) / max(scale, 1e-30)
    print(f"[gp] {what}: {err:.3e}")
    return err


@functools.lru_cache(maxsize=None)
def factor_case(n):
    """A = B B^T / n + I (cond <= 5.1) in float32 and its float64 Cholesky factor: made once per n and not modified."""
    a = gref.spd(n, 100 + n)
    return a, gref.cholesky(a)


def _in_buffer(lower_of, ld):
    """An (n, ld) buffer of MARK with the lower triangle of the (n, n) matrix in its first n columns; returns (buffer, the (n, n)
    view, the mask of what must not change)."""
    n = lower_of.shape[0]
    buf = torch.full((n, ld), MARK)
    low = torch.tril(torch.ones(n, n, dtype=torch.bool))
    buf[:, :n][low] = lower_of[low]
    keep = torch.ones(n, ld, dtype=torch.bool)
    keep[:, :n] = ~low
    buf = buf.to(DEV)
    return buf, buf[:, :n], keep.to(DEV)


# ---------------------------------------------------------------------------------------------
# 1. the factor
@pytest.mark.parametrize("pad", [0, 37], ids=["ld=n", "ld>n"])
@pytest.mark.parametrize("n", FACTOR_N)
def test_factor_against_float64(n, pad):
    from pytorch_generative_amd import ops

    a, want = factor_case(n)
    buf, view, keep = _in_buffer(a, n + pad)
    info = ops.cholesky_(view)
    torch.cuda.synchronize()
    assert int(info) == 0
    got = torch.tril(view).cpu()
    assert _err(got, want, f"factor n={n} pad={pad}") <= OUT_TOL
    assert _err(got.double() @ got.double().t(), a, f"L L^T n={n} pad={pad}") <= OUT_TOL
    assert bool((buf[keep] == MARK).all()), "the strict upper triangle or the memory beside the matrix was written"


# ---------------------------------------------------------------------------------------------
# 2. the solves
@pytest.mark.parametrize("transposed", [False, True], ids=["XLt=B", "XL=B"])
@pytest.mark.parametrize("rows", [1, 3, 64, 65])
@pytest.mark.parametrize("n", [1, 64, 130, 321])
def test_solves_against_float64(n, rows, transposed):
    from pytorch_generative_amd import ops

    l = factor_case(n)[1].float()  # the operand is the float32 rounding of the float64 factor, for both sides
    g = torch.Generator().manual_seed(n * 7 + rows)
    b = torch.randn(rows, n, generator=g)
    want = gref.solve_right(l, b, transposed)
    lbuf, lview, lkeep = _in_buffer(l, n + 5)
    xbuf = torch.full((rows, n + 11), MARK, device=DEV)
    xbuf[:, :n] = b.to(DEV)
    out = ops.trsm_right_(lview, xbuf[:, :n], transposed=transposed)
    torch.cuda.synchronize()
    assert out.data_ptr() == xbuf.data_ptr()
    assert _err(xbuf[:, :n], want, f"solve n={n} rows={rows} transposed={transposed}") <= OUT_TOL
    assert bool((xbuf[:, n:] == MARK).all()) and bool((lbuf[lkeep] == MARK).all())
    assert torch.equal(torch.tril(lview).cpu(), l)


# ---------------------------------------------------------------------------------------------
# 3. append
def _full_factor(n, ld):
    from pytorch_generative_amd import ops

    buf, view, _ = _in_buffer(factor_case(n)[0], ld)
    assert int(ops.cholesky_(view)) == 0
    return buf


@pytest.mark.parametrize("done,n", [(1, 2), (63, 65), (64, 65), (65, 130), (130, 321)])
def test_appended_factor_has_the_bits_of_the_full_one(done, n):
    from pytorch_generative_amd import ops

    ld = 384
    a = factor_case(n)[0]
    full = _full_factor(n, ld)
    again = _full_factor(n, ld)
    assert torch.equal(full, again), "two runs of the full factorisation differ"
    buf, view, keep = _in_buffer(a, ld)
    assert int(ops.cholesky_(view[:done, :done])) == 0  # the leading block alone: a's leading block is what it factors
    info = ops.cholesky_(view, n_done=done)
    torch.cuda.synchronize()
    assert int(info) == 0
    assert bool((buf[keep] == MARK).all())
    assert torch.equal(buf, full), f"append {done} -> {n}: max difference {float((buf - full).abs().max()):.3e}"


def test_ten_single_row_appends_from_60():
    from pytorch_generative_amd import ops

    n, ld = 70, 128
    full = _full_factor(n, ld)
    buf, view, _ = _in_buffer(factor_case(n)[0], ld)
    assert int(ops.cholesky_(view[:60, :60])) == 0
    for k in range(60, n):
        assert int(ops.cholesky_(view[:k + 1, :k + 1], n_done=k)) == 0
    assert torch.equal(buf, full), f"max difference {float((buf - full).abs().max()):.3e}"


@pytest.mark.parametrize("done,n", [(1, 2), (63, 65), (64, 65), (65, 130), (130, 321)])
def test_completed_columns_have_the_bits_of_the_full_solve(done, n):
    from pytorch_generative_amd import ops

    l = factor_case(n)[1].float().contiguous().to(DEV)
    g = torch.Generator().manual_seed(n)
    b = torch.randn(3, n, generator=g).to(DEV)
    full = ops.trsm_right_(l, b.clone())
    part = b.clone()
    ops.trsm_right_(l[:done, :done], part[:, :done])
    assert torch.equal(part[:, :done], full[:, :done]), "the leading columns depend on the columns behind them"
    ops.trsm_right_(l, part, col_done=done)
    assert torch.equal(part, full), f"columns {done} -> {n}: max difference {float((part - full).abs().max()):.3e}"


# ---------------------------------------------------------------------------------------------
# 4. the failed pivot
def test_failed_pivot_is_recorded_and_the_launch_returns():
    from pytorch_generative_amd import ops

    a = factor_case(130)[0].clone()
    a[70, 70] = -5.0  # indefinite: the pivots before index 70 are those of the positive definite matrix
    buf, view, keep = _in_buffer(a, 130)
    info = ops.cholesky_(view)
    torch.cuda.synchronize()
    assert int(info) == 71
    assert bool(torch.isnan(view[70, 70])) and bool(torch.isnan(torch.tril(view)[71:, 70:]).any()), "NaNs propagate"
    assert torch.equal(torch.tril(view)[:70, :70].cpu(), torch.tril(_full_factor(130, 130)[:70, :70]).cpu())
    assert bool((buf[keep] == MARK).all())
    # a later pivot does not overwrite the first one, a NaN pivot counts
    b = factor_case(130)[0].clone()
    b[3, 3] = float("nan")
    b[100, 100] = -1.0
    _, view, _ = _in_buffer(b, 130)
    assert int(ops.cholesky_(view)) == 4


def test_model_raises_linalg_error_and_drops_its_cache():
    gp = gp_mod()
    model = gp.GaussianProcess(gp.Const(), gp.SquaredExponential(), None)  # noiseless
    x = torch.zeros(80, 1, device=DEV)  # 80 copies of one point: K is all ones, the pivot at index 1 is exactly 0
    model.fit(x, torch.zeros(80, 1, device=DEV))
    with pytest.raises(torch.linalg.LinAlgError, match=r"index 1 of 80.*noise_var"):
        model.predict(torch.ones(3, 1, device=DEV))
    assert model._factor is None and model._n_factored == 0
    model.noise_var.fill_(0.1)  # an in-place change is seen; the same data now factor
    mu, sig = model.predict(torch.ones(3, 1, device=DEV))
    assert bool(torch.isfinite(mu).all()) and bool(torch.isfinite(sig).all()) and model._factor_route == "full"


# ---------------------------------------------------------------------------------------------
# 5. the covariance
@functools.lru_cache(maxsize=None)
def se_case(d):
    g = torch.Generator().manual_seed(d)
    a, b = torch.randn(130, d, generator=g), torch.randn(70, d, generator=g)
    std, lengthscale = 1.3, 0.9 * d ** 0.5
    return a, b, std, lengthscale, gref.se(a, b, std, lengthscale), gref.se(a, a, std, lengthscale)


@pytest.mark.parametrize("route", [None, "direct", "mfma"])
@pytest.mark.parametrize("d", [1, 3, 16, 17, 40])
def test_se_kernel_against_float64(d, route):
    from pytorch_generative_amd import ops

    a, b, std, lengthscale, cross, sym = se_case(d)
    noise = 0.05
    assert ops.gp_plan(130, 70, d, 1)["se_route"] == int(d > 16)
    ad, bd = a.to(DEV), b.to(DEV)
    out = torch.full((130, 70 + 9), MARK, device=DEV)
    ops.se_kernel(ad, bd, std, lengthscale, noise, out=out[:, :70], route=route)
    assert _err(out[:, :70], cross, f"se cross d={d} route={route}") <= OUT_TOL
    assert bool((out[:, 70:] == MARK).all())
    k = ops.se_kernel(ad, ad, std, lengthscale, noise, route=route)
    diag = float(np.float32(std) * np.float32(std) + np.float32(noise))
    assert torch.equal(k, k.t()), "not exactly symmetric"
    assert bool((k.diagonal() == diag).all()), "the diagonal is not exactly std^2 + noise_var"
    want = sym + noise * torch.eye(130, dtype=torch.float64)
    assert _err(k, want, f"se symmetric d={d} route={route}") <= OUT_TOL
    # rows of the symmetric matrix by the cross form: the bits of the symmetric form, and nothing above the diagonal written
    rows = torch.full((60, 130), MARK, device=DEV)
    ops.se_kernel(ad[70:], ad, std, lengthscale, noise, out=rows, diag_offset=70, route=route)
    low = torch.tril(torch.ones(130, 130, dtype=torch.bool, device=DEV))[70:]
    assert torch.equal(rows[low], k[70:][low]) and bool((rows[~low] == MARK).all())
    # mirror=False: the tiles above the diagonal are not visited
    half = torch.full((130, 130), MARK, device=DEV)
    ops.se_kernel(ad, ad, std, lengthscale, noise, out=half, mirror=False, route=route)
    assert torch.equal(torch.tril(half), torch.tril(k)) and bool((half[:64, 64:] == MARK).all())


def test_gemm_update_is_one_chain_whatever_the_blocking():
    """c - a b^T in one call and in three pieces along k: the same bits (the accumulator is seeded with c); and against float64."""
    from pytorch_generative_amd import ops

    g = torch.Generator().manual_seed(11)
    a, b, c = torch.randn(70, 160, generator=g), torch.randn(90, 160, generator=g), torch.randn(70, 90, generator=g)
    ad, bd = a.to(DEV), b.to(DEV)
    once = ops.gemm_nt_(c.to(DEV), ad, bd)
    pieces = c.to(DEV)
    for lo, hi in ((0, 64), (64, 128), (128, 160)):
        ops.gemm_nt_(pieces, ad[:, lo:hi], bd[:, lo:hi])
    assert torch.equal(once, pieces)
    assert _err(once, c.double() - a.double() @ b.double().t(), "gemm c - a b^T") <= OUT_TOL
    plus = ops.gemm_nt_(c.to(DEV), ad, bd.t().contiguous(), add=True, b_transposed=True)
    assert _err(plus, c.double() + a.double() @ b.double().t(), "gemm c + a b (b transposed)") <= OUT_TOL
    sq = torch.randn(70, 70, generator=g)
    low = ops.gemm_nt_(sq.to(DEV), ad, ad, lower=True, mirror=True)
    want = torch.tril(sq.double() - a.double() @ a.double().t())
    want = want + torch.tril(want, -1).t()
    assert torch.equal(low, low.t()) and _err(low, want, "gemm lower mirrored") <= OUT_TOL


# ---------------------------------------------------------------------------------------------
# 6. the model
def _model(case, **kw):
    gp = gp_mod()
    model = gp.GaussianProcess(gp.Const(case["value"]), gp.SquaredExponential(case["std"], case["lengthscale"]), case["noise_var"])
    for k, v in kw.items():
        setattr(model, k, v)
    return model.to(DEV)


@pytest.mark.parametrize("name", sorted(load_cases()))
def test_model_against_the_reference_fixture(name):
    case = load_cases()[name]
    model = _model(case)
    x, tx, ty = case["x"].to(DEV), case["train_x"].to(DEV), case["train_y"].to(DEV)
    prior_max = case["std"] ** 2
    n1 = case["n1"]
    for tag, lo, hi, route in (("", 0, n1, "full"), ("2", n1, case["n"], "append")):
        model.fit(tx[lo:hi], ty[lo:hi])
        mu, sig = model.predict(x)
        assert model._factor_route == route and model._kernel_route == "se" and model._n_factored == hi
        assert mu.shape == case["mu" + tag].shape and sig.shape == case["sig" + tag].shape and not mu.requires_grad
        assert _err(mu, case["mu" + tag], f"{name}{tag} mu") <= OUT_TOL
        assert _err(sig, case["sig" + tag], f"{name}{tag} sig", scale=prior_max) <= OUT_TOL
        assert torch.equal(sig, sig.t())


@functools.lru_cache(maxsize=None)
def big_case():
    """(n, m, d, noise_var, lengthscale) = (321, 130, 3, 0.05, 0.7) with its float64 posterior, made once."""
    g = torch.Generator().manual_seed(321)
    case = {"std": 1.2, "lengthscale": 0.7, "value": 0.3, "noise_var": 0.05, "train_x": torch.randn(321, 3, generator=g),
            "x": torch.randn(130, 3, generator=g)}
    case["train_y"] = torch.sin(case["train_x"].sum(1, keepdim=True)) + 0.3 + 0.05 ** 0.5 * torch.randn(321, 1, generator=g)
    noise = float(torch.tensor(0.05, dtype=torch.float32))
    case["mu"], case["sig"] = gref.posterior(case["train_x"], case["train_y"], case["x"], 1.2, 0.7, 0.3, noise)
    return case


def test_model_against_float64():
    case = big_case()
    model = _model(case)
    model.fit(case["train_x"].to(DEV), case["train_y"].to(DEV))
    mu, sig = model.predict(case["x"].to(DEV))
    assert _err(mu, case["mu"], "n=321 mu") <= OUT_TOL
    assert _err(sig, case["sig"], "n=321 sig", scale=case["std"] ** 2) <= OUT_TOL
    assert torch.equal(sig, sig.t()) and model._factor_route == "full"


def test_append_equals_full_across_capacity_doublings():
    case = big_case()
    tx, ty, x = case["train_x"].to(DEV), case["train_y"].to(DEV), case["x"].to(DEV)
    grown = _model(case)
    caps = []
    for lo, hi in ((0, 40), (40, 70), (70, 130)):  # capacities 64, 128, 256
        grown.fit(tx[lo:hi], ty[lo:hi])
        mu, sig = grown.predict(x)
        caps.append(grown._factor.shape[0])
        once = _model(case, incremental=False)
        once.fit(tx[:hi], ty[:hi])
        mu1, sig1 = once.predict(x)
        assert once._factor_route == "full" and grown._factor_route == ("append" if lo else "full")
        assert torch.equal(torch.tril(grown._factor[:hi, :hi]), torch.tril(once._factor[:hi, :hi])), f"factor after {hi} rows"
        assert torch.equal(grown._zt[:, :hi], once._zt[:, :hi]) and torch.equal(mu, mu1) and torch.equal(sig, sig1)
    assert caps == [64, 128, 256]
    # incremental = False on the growing model: the factor is made afresh
    off = _model(case, incremental=False)
    off.fit(tx[:40], ty[:40])
    off.predict(x)
    off.fit(tx[40:70], ty[40:70])
    off.predict(x)
    assert off._factor_route == "full"


def test_callable_kernel_agrees_with_the_se_route():
    case = big_case()
    gp = gp_mod()
    tx, ty, x = case["train_x"][:130].to(DEV), case["train_y"][:130].to(DEV), case["x"].to(DEV)
    std, lengthscale, value = case["std"], case["lengthscale"], case["value"]
    calls = []

    def kernel(a, b):
        calls.append((a.shape[0], b.shape[0]))
        return std ** 2 * torch.exp(-0.5 * (torch.cdist(a, b) / lengthscale) ** 2)

    model = gp.GaussianProcess(lambda t: torch.full((t.shape[0], 1), value, device=t.device), kernel, case["noise_var"]).to(DEV)
    assert model._kernel_route == "callable"
    model.fit(tx[:100], ty[:100])
    model.predict(x)
    model.fit(tx[100:], ty[100:])
    mu, sig = model.predict(x)
    assert model._factor_route == "full", "a callable's state cannot be seen: no append"
    se = _model(case)
    se.fit(tx, ty)
    mu_se, sig_se = se.predict(x)
    noise = float(torch.tensor(case["noise_var"], dtype=torch.float32))
    mu64, sig64 = gref.posterior(tx.cpu(), ty.cpu(), x.cpu(), std, lengthscale, value, noise)
    for got_mu, got_sig, what in ((mu, sig, "callable"), (mu_se, sig_se, "se")):
        assert _err(got_mu, mu64, f"{what} mu") <= OUT_TOL and _err(got_sig, sig64, f"{what} sig", scale=std ** 2) <= OUT_TOL
    assert _err(mu, mu_se.cpu(), "callable against se, mu") <= OUT_TOL
    assert _err(sig, sig_se.cpu(), "callable against se, sig", scale=std ** 2) <= OUT_TOL
    # the cached factor serves the next predict: the training covariance is not asked for again
    calls.clear()
    model.predict(x[:50])
    assert sorted(calls) == [(50, 50), (50, 130)]
    model.reset_cache()
    model.predict(x[:50])
    assert (130, 130) in calls



def test_callable_route_reads_only_the_lower_triangle_and_watches_what_it_can_see():
    case = big_case()
    gp = gp_mod()
    tx, ty, x = case["train_x"][:100].to(DEV), case["train_y"][:100].to(DEV), case["x"][:50].to(DEV)

    def mean(t):
        return torch.full((t.shape[0], 1), 0.3, device=t.device)

    def build(poison):
        kernel = gp.SquaredExponential(case["std"], case["lengthscale"])

        def wrapped(a, b):
            out = kernel(a, b)
            if poison and a is b:  # a square covariance: NaNs above the diagonal must not matter
                out = out.masked_fill(torch.triu(torch.ones_like(out, dtype=torch.bool), 1), float("nan"))
            return out

        model = gp.GaussianProcess(mean, wrapped, case["noise_var"]).to(DEV)
        model.fit(tx, ty)
        return model

    clean, poisoned = build(False), build(True)
    assert poisoned._kernel_route == "callable"
    (mu0, sig0), (mu1, sig1) = clean.predict(x), poisoned.predict(x)
    assert bool(torch.isfinite(sig1).all()) and torch.equal(mu0, mu1) and torch.equal(sig0, sig1) and torch.equal(sig1, sig1.t())
    # a SquaredExponential beside a callable mean is still watched
    model = gp.GaussianProcess(mean, gp.SquaredExponential(case["std"], case["lengthscale"]), case["noise_var"]).to(DEV)
    model.fit(tx, ty)
    mu_a, _ = model.predict(x)
    model.kernel.lengthscale = 1.1
    model._factor_route = None
    mu_b, _ = model.predict(x)
    assert model._factor_route == "full" and not torch.equal(mu_a, mu_b)
    noise = float(torch.tensor(case["noise_var"], dtype=torch.float32))
    mu64, _ = gref.posterior(tx.cpu(), ty.cpu(), x.cpu(), case["std"], 1.1, 0.3, noise)
    assert _err(mu_b, mu64, "callable mean, changed lengthscale") <= OUT_TOL


def test_predict_before_fit_is_the_prior():
    case = big_case()
    model = _model(case)
    x = case["x"].to(DEV)
    mu, sig = model.predict(x)
    mu64, sig64 = gref.prior(case["x"], case["std"], case["lengthscale"], case["value"])
    assert mu.shape == (130, 1) and _err(mu, mu64, "prior mu") <= OUT_TOL and _err(sig, sig64, "prior sig") <= OUT_TOL
    assert torch.equal(sig, sig.t()) and model._factor is None


def test_hyperparameter_change_forces_a_full_factorisation():
    case = big_case()
    gp = gp_mod()
    tx, ty, x = case["train_x"].to(DEV), case["train_y"].to(DEV), case["x"].to(DEV)
    model = gp.GaussianProcess(gp.Const(), gp.SquaredExponential(), 0.05).to(DEV)  # Parameters, on the GPU
    model.fit(tx[:50], ty[:50])
    model.predict(x)
    model.fit(tx[50:80], ty[50:80])
    model.predict(x)
    assert model._factor_route == "append"
    with torch.no_grad():
        model.kernel.lengthscale.fill_(0.7)
    model.fit(tx[80:100], ty[80:100])
    mu, sig = model.predict(x)
    assert model._factor_route == "full"
    noise = float(torch.tensor(0.05, dtype=torch.float32))
    mu64, sig64 = gref.posterior(case["train_x"][:100], case["train_y"][:100], case["x"], 1.0, 0.7, 0.0, noise)
    assert _err(mu, mu64, "after the change, mu") <= OUT_TOL and _err(sig, sig64, "after the change, sig", scale=1.0) <= OUT_TOL
    # without new data too: the cached factor is not served
    model.noise_var.fill_(0.2)
    model._factor_route = None
    mu2, _ = model.predict(x)
    assert model._factor_route == "full" and not torch.equal(mu, mu2)
    for name, value in (("std", 1.5), ("value", 0.4)):
        owner = model.kernel if name == "std" else model.mean
        with torch.no_grad():
            getattr(owner, name).fill_(value)
        model.fit(tx[100:101], ty[100:101])
        model.predict(x)
        assert model._factor_route == "full", name
        model.fit(tx[101:102], ty[101:102])
        model.predict(x)
        assert model._factor_route == "append", name


def test_predict_replays_in_a_graph_with_identical_bits():
    case = big_case()
    model = _model(case)
    model.fit(case["train_x"][:130].to(DEV), case["train_y"][:130].to(DEV))
    x = case["x"].to(DEV)
    mu, sig = model.predict(x)  # makes the factor; from here on predict does not synchronise
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        model.predict(x)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        mu_g, sig_g = model.predict(x)
    for _ in range(2):
        mu_g.zero_()
        sig_g.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(mu_g, mu) and torch.equal(sig_g, sig)


# ---------------------------------------------------------------------------------------------
# 7. sampling
def _dense_1d(noise_var):
    """n = 200 training points and m = 65 query points on a line: the posterior covariance is numerically singular."""
    gp = gp_mod()
    tx = torch.linspace(-3, 3, 200).reshape(-1, 1)
    g = torch.Generator().manual_seed(9)
    ty = torch.sin(2 * tx) + noise_var ** 0.5 * torch.randn(200, 1, generator=g)
    model = gp.GaussianProcess(gp.Const(0.0), gp.SquaredExponential(1.0, 1.0), noise_var).to(DEV)
    model.fit(tx.to(DEV), ty.to(DEV))
    return model, torch.linspace(-3, 3, 65).reshape(-1, 1).to(DEV)


def test_sample_is_mean_plus_z_times_factor_and_the_ladder_step_is_the_first_that_factors():
    from pytorch_generative_amd import ops

    gp = gp_mod()
    model, x = _dense_1d(0.01)
    gen = torch.Generator(device=DEV).manual_seed(5)
    out = model.sample(x, 4, generator=gen)
    mu, sig = model.predict(x)
    jitter, factor = model._sample_jitter, model._sample_factor
    print(f"[gp] ladder step taken at noise_var = 0.01: {jitter:g}")
    assert out.shape == (4, 65) and out.dtype == torch.float32 and out.device == x.device
    assert jitter in gp.JITTER_LADDER and bool((torch.triu(factor, 1) == 0).all())
    z = torch.randn((4, 65), device=DEV, generator=torch.Generator(device=DEV).manual_seed(5))
    want = mu.double().t().cpu() + z.double().cpu() @ factor.double().t().cpu()
    assert _err(out, want, "sample against mu^T + Z L_s^T") <= OUT_TOL
    scale = 1.0  # the prior diagonal std^2
    target = sig.double().cpu() + jitter * scale * torch.eye(65, dtype=torch.float64)
    assert _err(factor.double() @ factor.double().t(), target, "L_s L_s^T against sig + jitter", scale=scale) <= OUT_TOL
    # the recorded step is the first of the ladder that factors
    for step in gp.JITTER_LADDER:
        trial = sig.clone()
        ops.add_diag_(trial, step * scale)
        failed = int(ops.cholesky_(trial)) != 0
        assert failed == (step < jitter), (step, jitter)
        if step == jitter:
            break


def test_sample_of_a_well_separated_prior_against_float64():
    gp = gp_mod()
    model = gp.GaussianProcess(gp.Const(0.5), gp.SquaredExponential(1.5, 1.0)).to(DEV)
    x = (torch.arange(70, dtype=torch.float32) * 1.5).reshape(-1, 1)  # neighbours 1.5 lengthscales apart: cond about 5
    out = model.sample(x.to(DEV), 6, generator=torch.Generator(device=DEV).manual_seed(1))
    assert model._sample_jitter == 0.0 and model._factor is None
    z = torch.randn((6, 70), device=DEV, generator=torch.Generator(device=DEV).manual_seed(1)).double().cpu()
    mu64, sig64 = gref.prior(x, 1.5, 1.0, 0.5)
    want = mu64.t() + z @ gref.cholesky(sig64).t()
    assert _err(out, want, "prior sample against float64") <= OUT_TOL
    assert _err(model._sample_factor, gref.cholesky(sig64), "prior sample factor") <= OUT_TOL
    with pytest.raises(ValueError, match="one output column"):
        wide = gp.GaussianProcess(lambda t: torch.zeros(t.shape[0], 2, device=t.device), gp.SquaredExponential(1.0, 1.0)).to(DEV)
        wide.sample(x.to(DEV), 1)
