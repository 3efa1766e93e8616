"""CPU: ARD lengthscales and Matern kernels of the Gaussian process without a device — the float64 closed forms of
tests/_gp_ard_ref.py against float64 autograd; pg_gp_ard_plan against an enumeration; every new entry point refuses what the plan
refuses and reports a missing device only for a call it accepted; what the kernel classes and the model raise; the conditioning
of the inputs the GPU model tests use; and that the float64 Adam loop tells the irrelevant input column from the others."""

import ctypes
import itertools

import numpy as np
import pytest
import torch

import _gp_ard_ref as aref
import _gp_mll_ref as mref

PLAN_INTS = 8
EINVAL, ESHAPE, NO_DEVICE = -1, -2, 100  # hipErrorNoDevice
MAX_N, MAX_D, MAX_P, ARD_MAX_D = 16384, 4096, 4096, 256
TILE, CHUNK = 64, 64
CLOSED_FORM_TOL = 1e-10
CONDITION = 1e-2  # |d/d l_c| >= 1e-2 of the magnitude of its terms: the GPU gate is then never looser than 1 % of the value


def gp_mod():
    from pytorch_generative_amd.models import gaussian_process

    return gaussian_process


# ---------------------------------------------------------------------------------------------
# the float64 closed forms
def _distinct_problem(n, d, p, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, d, generator=g, dtype=torch.float64)
    y = torch.sin(x.sum(1, keepdim=True)) + 0.3 * torch.randn(n, p, generator=g, dtype=torch.float64)
    lengthscale = (0.7 + 1.3 * torch.rand(d, generator=g, dtype=torch.float64)) * d ** 0.5
    assert float(aref.scaled_sq_terms(x, x, 1.0).sum(-1).add(torch.eye(n, dtype=torch.float64)).min()) > 0  # no duplicate rows
    return x, y, lengthscale


def _worst(got, want):
    return float(((got - want).abs() / want.abs()).max())


@pytest.mark.parametrize("kind", aref.KINDS)
@pytest.mark.parametrize("n,d,p", [(50, 2, 3), (65, 17, 1)])
def test_closed_forms_equal_float64_autograd(kind, n, d, p):
    x, y, lengthscale = _distinct_problem(n, d, p, seed=n + d)
    hyper = (1.3, lengthscale, 0.1, 0.2)
    value, grads, sizes = aref.closed_form(x, y, *hyper, kind)
    want, want_grads = aref.autograd_form(x, y, *hyper, kind)
    assert grads["lengthscale"].shape == (d,) and sizes.shape == (d,) and bool((sizes >= grads["lengthscale"].abs()).all())
    errs = {"value": _worst(value, want)}
    errs.update({name: _worst(grads[name], want_grads[name]) for name in aref.NAMES})
    print(f"[gp ard] closed form {kind} n={n} d={d} p={p}: " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert max(errs.values()) <= CLOSED_FORM_TOL
    # the operand-level forms the GPU tests use give the same numbers from the same factor
    kf = aref.covariance(x, x, hyper[0], lengthscale, kind)
    l = torch.linalg.cholesky(kf + hyper[2] * torch.eye(n, dtype=torch.float64))
    zt = torch.linalg.solve_triangular(l, y - hyper[3], upper=False).t()
    xinv = mref.tri_inverse_t(l)
    alpha_t = zt @ xinv.t()
    sums, magnitudes = aref.ard_sums(x, hyper[0], lengthscale, mref.gram_upper(xinv), alpha_t, kind)
    want_sums = torch.cat([torch.stack([want_grads["std"], want_grads["noise_var"]]), want_grads["lengthscale"]])
    assert bool(((sums - want_sums).abs() <= 1e-9 * magnitudes).all())


@pytest.mark.parametrize("kind", aref.KINDS)
def test_equal_lengthscales_sum_to_the_shared_derivative(kind):
    x, y, _ = _distinct_problem(40, 3, 2, seed=9)
    shared = 1.7
    value, grads, size = aref.closed_form(x, y, 1.3, shared, 0.1, 0.2, kind)
    same, vector, sizes = aref.closed_form(x, y, 1.3, torch.full((3,), shared, dtype=torch.float64), 0.1, 0.2, kind)
    assert grads["lengthscale"].shape == () and vector["lengthscale"].shape == (3,)
    assert _worst(same, value) <= CLOSED_FORM_TOL
    assert abs(float(vector["lengthscale"].sum() - grads["lengthscale"])) <= CLOSED_FORM_TOL * float(size)
    for name in ("std", "noise_var", "value"):
        assert _worst(vector[name], grads[name]) <= CLOSED_FORM_TOL, name
    # ... and the shared derivative is what autograd gives for one scalar
    scalar = torch.tensor(shared, dtype=torch.float64, requires_grad=True)
    aref.log_evidence(x, y, 1.3, scalar, 0.1, 0.2, kind).backward()
    assert abs(float(scalar.grad - grads["lengthscale"])) <= CLOSED_FORM_TOL * float(size)


def test_shared_squared_exponential_is_the_existing_closed_form():
    x, y, _ = _distinct_problem(50, 2, 3, seed=4)
    hyper = (1.3, 0.9, 0.1, 0.2)
    value, grads, _ = aref.closed_form(x, y, *hyper, "se")
    want, want_grads = mref.closed_form(x, y, *hyper)
    assert _worst(value, want) <= CLOSED_FORM_TOL
    for name in mref.NAMES:
        assert _worst(grads[name], want_grads[name]) <= CLOSED_FORM_TOL, name
    q = torch.randn(7, 2, dtype=torch.float64)
    assert torch.allclose(aref.covariance(q, x, 1.3, 0.9, "se"), 1.3 ** 2 * torch.exp(-((q[:, None] - x[None]) ** 2).sum(-1) / (2 * 0.9 ** 2)),
                          rtol=1e-13, atol=0)


def test_duplicate_rows_are_finite_in_the_closed_form():
    """omega is finite at r = 0: the closed form never divides by r."""
    x, y, lengthscale = _distinct_problem(20, 3, 1, seed=2)
    x[7] = x[3]
    for kind in aref.KINDS:
        value, grads, sizes = aref.closed_form(x, y, 1.3, lengthscale, 0.1, 0.2, kind)
        assert bool(torch.isfinite(value)) and bool(torch.isfinite(grads["lengthscale"]).all()) and bool(torch.isfinite(sizes).all())
        assert float(aref.covariance(x, x, 1.3, lengthscale, kind)[7, 3]) == 1.3 ** 2


# ---------------------------------------------------------------------------------------------
# the plan and the entry points, host side only
def _plan(lib, n, d, p):
    out = (ctypes.c_longlong * PLAN_INTS)()
    rc = lib.pg_gp_ard_plan(n, d, p, out, PLAN_INTS)
    return rc, list(out)


GRID = list(itertools.product((1, 64, 65, MAX_N, MAX_N + 1), (1, 64, 65, ARD_MAX_D, ARD_MAX_D + 1), (1, MAX_P + 1)))


def _inside(n, d, p):
    return 1 <= n <= MAX_N and 1 <= d <= ARD_MAX_D and 1 <= p <= MAX_P


def test_ard_plan_against_an_enumeration(lib):
    from pytorch_generative_amd import ops

    for n, d, p in GRID + [(0, 1, 1), (8, 0, 1), (8, 1, 0), (-1, 2, 1)]:
        rc, out = _plan(lib, n, d, p)
        assert rc == (0 if _inside(n, d, p) else ESHAPE), (n, d, p, rc)
        assert ops.gp_ard_plan_status(n, d, p)[0] == rc
        if rc:
            assert lib.pg_last_error() and ops.gp_ard_plan(n, d, p) is None
            continue
        tile, tiles, row, ws_floats, chunks, launches, max_d, chunk = out
        panels = len(range(0, n, TILE))
        lower = panels * (panels + 1) // 2 if panels > 64 else sum(1 for i in range(panels) for j in range(panels) if j <= i)
        assert (tile, launches, max_d, chunk) == (TILE, 2, ARD_MAX_D, CHUNK)
        assert tiles == lower == ops.gp_mll_plan(n, d, p)["sums_tiles"]
        assert row == d + 2 and ws_floats == lower * (d + 2) and chunks == len(range(0, d, CHUNK))
        plan = ops.gp_ard_plan(n, d, p)
        assert plan["workspace_floats"] == ws_floats and plan["column_chunks"] == chunks and plan["partial_row_floats"] == row
    assert b"256" in (_plan(lib, 8, ARD_MAX_D + 1, 1), lib.pg_last_error())[1]  # the refusal names the limit
    assert lib.pg_gp_ard_plan(8, 1, 1, (ctypes.c_longlong * PLAN_INTS)(), PLAN_INTS - 1) == EINVAL  # short array
    assert lib.pg_gp_ard_plan(8, 1, 1, None, PLAN_INTS) == EINVAL


def _buf():
    buf = np.zeros(1 << 12, dtype=np.float32)
    return buf, buf.ctypes.data


def _entries(lib, p, n, d, pp, kind=2, ld=1 << 20):
    """Every new launch on the problem (n, d, pp) with strides that fit any accepted size: (largest d, uses p, call)."""
    return (
        (MAX_D, False, lambda: lib.pg_gp_stat_kernel(kind, p, ld, n, p, ld, n, d, 1.0, 1.0, None, 0.0, p, ld, 0, 0, None)),
        (MAX_D, False, lambda: lib.pg_gp_stat_kernel(kind, p, ld, n, p, ld, n, d, 1.0, 1.0, p, 0.0, p, ld, 0, 0, None)),
        (MAX_D, True, lambda: lib.pg_gp_stat_mll_sums(kind, p, ld, n, d, 1.0, 1.0, p, ld, p, ld, pp, p, 1 << 40, p, None)),
        (ARD_MAX_D, True, lambda: lib.pg_gp_ard_mll_sums(kind, p, ld, n, d, 1.0, p, p, ld, p, ld, pp, p, 1 << 40, p, None)),
    )


def test_launches_refuse_what_the_plan_refuses(lib):
    """Host side only: every check comes before the device is looked for, so these statuses are those of any machine."""
    _keep, p = _buf()
    no_gpu = not torch.cuda.is_available()
    calls = 0
    for n, d, pp in GRID + [(8, MAX_D, 1), (8, MAX_D + 1, 1), (0, 2, 1), (8, 0, 1), (8, 2, 0)]:
        for kind in (0, 1, 2):
            for max_d, uses_p, call in _entries(lib, p, n, d, pp, kind):
                accepted = 1 <= n <= MAX_N and 1 <= d <= max_d and (1 <= pp <= MAX_P or not uses_p)
                if not accepted:
                    assert call() == ESHAPE and lib.pg_last_error(), (n, d, pp, kind)
                elif no_gpu:
                    assert call() == NO_DEVICE and b"no HIP device" in lib.pg_last_error(), (n, d, pp, kind)
                    calls += 1
    if no_gpu:
        assert calls > 100
    # an unknown kind, null pointers, strides below the row length, a short workspace, the hyperparameters
    for kind in (-1, 3):
        assert [call() for *_, call in _entries(lib, p, 8, 2, 1, kind)] == [EINVAL] * 4 and b"kind" in lib.pg_last_error()
    good = [2, p, 2, 8, p, 2, 8, 2, 1.0, 1.0, p, 0.0, p, 8, 0, 0, None]  # stat_kernel
    for k in (1, 4, 12):
        args = list(good)
        args[k] = None
        assert lib.pg_gp_stat_kernel(*args) == EINVAL, k
    for k, low in ((2, 1), (5, 1), (13, 7), (15, 128)):  # the strides of a, b, k; an unknown flag
        args = list(good)
        args[k] = low
        assert lib.pg_gp_stat_kernel(*args) == EINVAL, k
    args = list(good)
    args[9], args[10] = 0.0, None  # a shared lengthscale must be > 0 ...
    assert lib.pg_gp_stat_kernel(*args) == EINVAL
    args[10] = p  # ... and is ignored beside per-dimension ones
    assert lib.pg_gp_stat_kernel(*args) == (NO_DEVICE if no_gpu else 0)
    args = list(good)
    args[15] = 32 | 1  # the forced exact-difference route holds d <= 64
    args[2] = args[5] = args[7] = 65
    assert lib.pg_gp_stat_kernel(*args) == ESHAPE
    good = [2, p, 2, 8, 2, 1.0, p, p, 8, p, 8, 1, p, 10 * 4, p, None]  # ard_mll_sums: 1 tile x (d + 2) floats
    for k in (1, 6, 7, 9, 12, 14):
        args = list(good)
        args[k] = None
        assert lib.pg_gp_ard_mll_sums(*args) == EINVAL, k
    for k, low in ((2, 1), (8, 7), (10, 7), (13, 3)):  # the strides of x, h, alpha_t; a workspace one float short
        args = list(good)
        args[k] = low
        assert lib.pg_gp_ard_mll_sums(*args) == EINVAL, k
    assert b"workspace" in lib.pg_last_error()
    for std in (0.0, float("nan")):
        args = list(good)
        args[5] = std
        assert lib.pg_gp_ard_mll_sums(*args) == EINVAL, std
    good = [1, p, 2, 8, 2, 1.0, 1.0, p, 8, p, 8, 1, p, 3, p, None]  # stat_mll_sums
    for k, bad in ((1, None), (7, None), (12, None), (14, None), (2, 1), (13, 2), (6, 0.0), (5, 0.0)):
        args = list(good)
        args[k] = bad
        assert lib.pg_gp_stat_mll_sums(*args) == EINVAL, k


# ---------------------------------------------------------------------------------------------
# the kernel classes and the model
def test_kernel_classes_and_routes():
    gp = gp_mod()
    for nu in (0.5, 2, 3.5, "2.5"):
        with pytest.raises(ValueError, match="nu"):
            gp.Matern(nu)
    assert gp.Matern().nu == 2.5 and gp.Matern().kind == "matern52" and gp.Matern(1.5).kind == "matern32"
    default = gp.Matern()
    assert isinstance(default.std, torch.nn.Parameter) and default.lengthscale.shape == () and not default.ard
    for kernel in (gp.Matern(n_dims=3), gp.SquaredExponential(n_dims=3)):
        assert isinstance(kernel.lengthscale, torch.nn.Parameter) and torch.equal(kernel.lengthscale.detach(), torch.ones(3)) and kernel.ard
        assert kernel.hyperparameters() == (1.0, (1.0, 1.0, 1.0))
    with pytest.raises(ValueError, match="3.*2|2.*3"):
        gp.SquaredExponential(lengthscale=torch.ones(3), n_dims=2)
    with pytest.raises(ValueError):
        gp.Matern(lengthscale=torch.ones(2, 2))
    const = gp.Const()
    assert gp.GaussianProcess(const, gp.SquaredExponential())._kernel_route == "se"
    assert gp.GaussianProcess(const, gp.SquaredExponential(1.0, 2.0))._kernel_route == "se"
    assert gp.GaussianProcess(const, gp.SquaredExponential(n_dims=2))._kernel_route == "stationary"
    assert gp.GaussianProcess(const, gp.SquaredExponential(lengthscale=torch.ones(1)))._kernel_route == "stationary"
    assert gp.GaussianProcess(const, gp.Matern())._kernel_route == "stationary"
    assert gp.GaussianProcess(const, gp.Matern(1.5, n_dims=4))._kernel_route == "stationary"
    assert gp.GaussianProcess(lambda x: x[:, :1] * 0, gp.Matern())._kernel_route == "callable"
    # the host values follow an in-place change and nothing else
    kernel = gp.Matern(n_dims=2)
    first = kernel.hyperparameters()
    assert kernel.hyperparameters() is not first and kernel.hyperparameters() == first
    with torch.no_grad():
        kernel.lengthscale[1] = 3.0
    assert kernel.hyperparameters() == (1.0, (1.0, 3.0))
    inverse = gp._device_inverse(kernel, "lengthscale", "cpu")
    assert torch.equal(inverse, torch.tensor([1.0, 1.0 / 3.0])) and gp._device_inverse(kernel, "lengthscale", "cpu") is inverse
    with torch.no_grad():
        kernel.lengthscale[0] = 2.0
    assert torch.equal(gp._device_inverse(kernel, "lengthscale", "cpu"), torch.tensor([0.5, 1.0 / 3.0]))


def test_model_raises():
    gp = gp_mod()
    x, y = torch.zeros(3, 2), torch.zeros(3, 1)
    for kernel in (gp.Matern(n_dims=3), gp.SquaredExponential(lengthscale=torch.ones(3))):
        with pytest.raises(ValueError, match="3 entries.*2 columns"):
            kernel(x, x)
        model = gp.GaussianProcess(gp.Const(), kernel, 0.1)
        with pytest.raises(ValueError, match="3 entries.*2 columns"):
            model.fit(x, y)
        with pytest.raises(ValueError, match="3 entries.*2 columns"):
            model.predict(x)
    for kernel in (gp.Matern(), gp.Matern(1.5, n_dims=2), gp.SquaredExponential(n_dims=2)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            kernel(x, x)
        model = gp.GaussianProcess(gp.Const(), kernel, 0.1)
        with pytest.raises(ValueError, match="fit"):
            model.log_marginal_likelihood()
        model.fit(x, y)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            model.predict(x)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            model.log_marginal_likelihood()
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            model.optimize_hyperparameters(1)
    wide = gp.GaussianProcess(gp.Const(), gp.Matern(n_dims=ARD_MAX_D + 1), 0.1)
    wide.fit(torch.zeros(3, ARD_MAX_D + 1), y)
    with pytest.raises(ValueError, match="256.*257"):  # the gradient: refused by the plan, before any launch
        wide.log_marginal_likelihood()
    with torch.no_grad(), pytest.raises(RuntimeError, match="no CPU fallback"):  # the value is served (it needs the device)
        wide.log_marginal_likelihood()
    other = gp.GaussianProcess(gp.Const(), lambda a, b: a @ b.t(), 0.1)
    other.fit(x, y)
    with pytest.raises(NotImplementedError, match="callable"):
        other.log_marginal_likelihood()


def test_operators_have_no_cpu_fallback(lib):
    import pytorch_generative_amd as pg
    from pytorch_generative_amd import ops

    for name in ("stationary_kernel", "stationary_mll_sums", "ard_mll_sums", "gp_ard_plan", "gp_ard_plan_status"):
        assert callable(getattr(pg.ops, name)), name
    a = torch.eye(4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.stationary_kernel(a, a, 1.0, 1.0, kind="matern52")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.stationary_kernel(a, a, 1.0, torch.ones(4), kind="matern32")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.stationary_mll_sums(a, 1.0, 1.0, a, a[:1], kind="matern52")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.ard_mll_sums(a, 1.0, torch.ones(4), a, a[:1])
    with pytest.raises(ValueError):
        ops.stationary_kernel(torch.zeros(4), a, 1.0, 1.0)
    with pytest.raises(ValueError):
        ops.stationary_kernel(torch.eye(4, requires_grad=True), a, 1.0, 1.0)


def test_autograd_node_returns_the_lengthscales_own_shape(monkeypatch):
    """The node without a device: the kernels' results are stood in for by fixed numbers laid out as the ARD reduction lays
    them out — value, std, noise_var, then one entry per lengthscale."""
    gp = gp_mod()
    model = gp.GaussianProcess(gp.Const(), gp.Matern(n_dims=3), 0.1)
    model.fit(torch.zeros(4, 3), torch.zeros(4, 1))
    model.noise_var.requires_grad_()
    fixed = torch.tensor([-7.0, 0.5, 2.0, 4.0, 10.0, 20.0, 30.0])
    monkeypatch.setattr(model, "_evidence", lambda want: (fixed[0], fixed[1:] if want else None))
    value = model.log_marginal_likelihood()
    (2.0 * value).backward()
    assert model.kernel.lengthscale.grad.shape == (3,) and model.kernel.lengthscale.grad.tolist() == [20.0, 40.0, 60.0]
    assert float(model.mean.value.grad) == 1.0 and float(model.kernel.std.grad) == 4.0 and float(model.noise_var.grad) == 8.0
    # the optimiser learns the logarithm of every entry and writes back in place
    model.noise_var.requires_grad_(False)
    lengthscale, version = model.kernel.lengthscale, model.kernel.lengthscale._version
    seen = model.optimize_hyperparameters(n_steps=2, lr=0.1)
    assert seen == [-7.0, -7.0] and model.kernel.lengthscale is lengthscale and lengthscale._version > version
    assert lengthscale.shape == (3,) and bool((lengthscale.detach().log() - 0.2).abs().max() < 0.02)
    assert abs(float(model.kernel.std.detach().log()) - 0.2) < 0.02 and abs(float(model.noise_var.log()) - (np.log(0.1) + 0.2)) < 0.02


# ---------------------------------------------------------------------------------------------
# the inputs of the GPU model tests
@pytest.mark.parametrize("kind", aref.KINDS)
def test_model_cases_are_well_conditioned(kind):
    """For every case and every column the float64 reference alone has |d/d l_c| >= 1e-2 sum |terms_c| / (2 l_c)."""
    hyper32 = [float(torch.tensor(v, dtype=torch.float32)) for v in (aref.STD, aref.NOISE_VAR, aref.VALUE)]
    for n, d, p in aref.MODEL_SHAPES:
        x, y, lengthscale = aref.model_case(kind, n, d, p)
        assert x.dtype == y.dtype == lengthscale.dtype == torch.float32 and lengthscale.shape == (d,)
        _, grads, sizes = aref.closed_form(x, y, hyper32[0], lengthscale, hyper32[1], hyper32[2], kind)
        ratio = float((grads["lengthscale"].abs() / sizes.clamp_min(1e-300)).min()) if n > 1 else float("inf")
        print(f"[gp ard] {kind} n={n} d={d} p={p}: min |d/d l_c| / magnitude {ratio:.3e}")
        assert bool((grads["lengthscale"].abs() >= CONDITION * sizes).all()), (kind, n, d, p, ratio)


def test_float64_loop_finds_the_irrelevant_column():
    x, y = aref.relevance_case()
    start = (1.0, (1.0, 1.0, 1.0), 1.0, 0.0)
    seen, final = aref.adam_loop(x, y, start, "matern52", n_steps=30, lr=0.05)
    print(f"[gp ard] float64 loop: {seen[0]:.4f} -> {seen[-1]:.4f}, lengthscales {final[1]}")
    assert len(seen) == 30 and seen[-1] > seen[0]
    assert final[1][2] > max(final[1][:2])
