"""CPU: the marginal likelihood of the Gaussian process without a device — pg_gp_mll_plan over the domain's edges and beyond;
the triangular tile counts it reports against counts made here by enumeration (the dense shortcut would show); every new entry
point refuses what the plan refuses and reports a missing device only for a call it accepted; the float64 closed forms of
tests/_gp_mll_ref.py against float64 autograd; what the model raises and which hyperparameters its autograd node serves."""

import ctypes
import random

import numpy as np
import pytest
import torch

import _gp_mll_ref as mref

PLAN_INTS = 16
EINVAL, ESHAPE, NO_DEVICE = -1, -2, 100  # hipErrorNoDevice
MAX_N, MAX_D, MAX_P = 16384, 4096, 4096
MIRROR = 2
TILE = 64
CLOSED_FORM_TOL = 1e-10


def gp_mod():
    from pytorch_generative_amd.models import gaussian_process

    return gaussian_process


def _plan(lib, n, d, p):
    out = (ctypes.c_longlong * PLAN_INTS)()
    rc = lib.pg_gp_mll_plan(n, d, p, out, PLAN_INTS)
    return rc, list(out)


def _sweep(seed=0, count=300):
    rng = random.Random(seed)
    edge_n = (1, 2, 63, 64, 65, 128, 129, 321, 4096, MAX_N - 1, MAX_N)
    shapes = [(n, d, p) for n in edge_n for d, p in ((1, 1), (16, 1), (17, 3), (MAX_D, MAX_P))]
    shapes += [(rng.randint(1, MAX_N), rng.randint(1, MAX_D), rng.randint(1, MAX_P)) for _ in range(count)]
    shapes += [(rng.randint(1, 700), rng.randint(1, 40), rng.randint(1, 70)) for _ in range(count)]
    shapes += [(n, 2, 1) for n in (0, -1, MAX_N + 1, 1 << 20)]
    shapes += [(8, d, 1) for d in (0, -3, MAX_D + 1)] + [(8, 2, p) for p in (0, -3, MAX_P + 1)]
    return shapes


def _inside(n, d, p):
    return 1 <= n <= MAX_N and 1 <= d <= MAX_D and 1 <= p <= MAX_P


def test_plan_domain_and_geometry(lib):
    from pytorch_generative_amd import ops

    for n, d, p in _sweep():
        rc, out = _plan(lib, n, d, p)
        assert rc == (0 if _inside(n, d, p) else ESHAPE), (n, d, p, rc)
        if rc:
            assert lib.pg_last_error() and ops.gp_mll_plan(n, d, p) is None
            continue
        (tile, panels, inv_launches, inv_products, gram_tiles, gram_products, sums_tiles, rows, ws_floats, route, direct_d, max_n, max_d,
         max_p, p_chunks, sums_launches) = out
        assert (tile, direct_d, max_n, max_d, max_p, sums_launches) == (TILE, 16, MAX_N, MAX_D, MAX_P, 2)
        assert panels == -(-n // TILE) and inv_launches == 2 * panels - 1
        assert route == int(d > 16) == ops.gp_plan(n, 1, d, p)["se_route"]  # the routing rule of se_kernel
        assert gram_tiles == sums_tiles == rows == panels * (panels + 1) // 2 and ws_floats == 3 * rows
        assert p_chunks == -(-p // 32)
        assert inv_products == (panels - 1) * panels * (panels + 1) // 6 and gram_products == panels * (panels + 1) * (panels + 2) // 6
        plan = ops.gp_mll_plan(n, d, p)
        assert plan["panels"] == panels and plan["workspace_floats"] == ws_floats and plan["inverse_tile_products"] == inv_products
    assert lib.pg_gp_mll_plan(8, 1, 1, (ctypes.c_longlong * PLAN_INTS)(), PLAN_INTS - 1) == EINVAL  # short array
    assert lib.pg_gp_mll_plan(8, 1, 1, None, PLAN_INTS) == EINVAL


@pytest.mark.parametrize("n", [1, 64, 65, 130, 321, 1000, 4096, MAX_N])
def test_tile_counts_are_triangular(lib, n):
    """The counts the plan reports against an enumeration of the tiles that can be non-zero. X = L^-T is upper triangular:
    after panel k of X L^T = I only the row tiles 0 .. k hold anything, and they update the P - 1 - k column tiles to the right;
    tile (I, J) of X X^T, J <= I, multiplies the k tiles I .. P - 1; the reduction visits the tiles on or below the diagonal.
    The dense solve and the dense update on an identity matrix visit P tiles per row instead: three times as many."""
    rc, out = _plan(lib, n, 2, 1)
    assert rc == 0
    P = -(-n // TILE)
    if P <= 64:  # every (panel, row tile, column tile) and every (row tile, column tile, k tile)
        inverse = sum(1 for k in range(P) for i in range(P) for j in range(P) if i <= k < j)
        gram = sum(1 for i in range(P) for j in range(P) for k in range(P) if j <= i <= k)
    else:  # the same sets, counted per panel and per row tile
        inverse = sum(len(range(0, k + 1)) * len(range(k + 1, P)) for k in range(P))
        gram = sum(len(range(0, i + 1)) * len(range(i, P)) for i in range(P))
    lower = sum(1 for i in range(P) for j in range(P) if j <= i)
    assert inverse == sum((k + 1) * (P - 1 - k) for k in range(P))
    assert out[3] == inverse and out[5] == gram and out[4] == out[6] == out[7] == lower
    dense = P * P * (P - 1) // 2 + P ** 3  # the dense right-looking solve of P row tiles and the dense P x P x P product
    if P >= 8:
        assert 2.4 * (out[3] + out[5]) < dense


def _buf():
    buf = np.zeros(1 << 12, dtype=np.float32)
    return buf, buf.ctypes.data


def _entries(lib, p, n, d, pp, ld=1 << 20):
    """Every new launch on the problem (n, d, pp) with strides that fit any accepted size: (uses d, uses p, call)."""
    return (
        (False, False, lambda: lib.pg_gp_trtri_t(p, ld, n, p + 64, ld, None)),
        (False, False, lambda: lib.pg_gp_gram_upper(p, ld, n, p + 64, ld, 0, None)),
        (False, False, lambda: lib.pg_gp_gram_upper(p, ld, n, p + 64, ld, MIRROR, None)),
        (True, True, lambda: lib.pg_gp_se_mll_sums(p, ld, n, d, 1.0, 1.0, p, ld, p, ld, pp, p, 1 << 40, p, None)),
        (False, True, lambda: lib.pg_gp_mll_value(p, ld, n, p, ld, p, ld, pp, p, None)),
    )


def test_launches_refuse_what_the_plan_refuses(lib):
    """Host side only: every check comes before the device is looked for, so these statuses are those of any machine."""
    _keep, p = _buf()
    for n in (0, -1, MAX_N + 1):
        for _, _, call in _entries(lib, p, n, 2, 1):
            assert call() == ESHAPE and lib.pg_last_error()
    for d in (0, MAX_D + 1):
        assert [call() for uses_d, _, call in _entries(lib, p, 8, d, 1) if uses_d] == [ESHAPE]
    for pp in (0, MAX_P + 1):
        assert [call() for _, uses_p, call in _entries(lib, p, 8, 2, pp) if uses_p] == [ESHAPE, ESHAPE]
    # null pointers, row strides below the row length, aliases, flags, the workspace, the hyperparameters
    assert lib.pg_gp_trtri_t(None, 8, 8, p, 8, None) == EINVAL and lib.pg_gp_trtri_t(p, 8, 8, None, 8, None) == EINVAL
    assert lib.pg_gp_trtri_t(p, 7, 8, p + 64, 8, None) == EINVAL and lib.pg_gp_trtri_t(p, 8, 8, p + 64, 7, None) == EINVAL
    assert lib.pg_gp_trtri_t(p, 8, 8, p, 8, None) == EINVAL  # x is l
    assert lib.pg_gp_gram_upper(None, 8, 8, p, 8, 0, None) == EINVAL and lib.pg_gp_gram_upper(p, 8, 8, None, 8, 0, None) == EINVAL
    assert lib.pg_gp_gram_upper(p, 7, 8, p + 64, 8, 0, None) == EINVAL and lib.pg_gp_gram_upper(p, 8, 8, p + 64, 7, 0, None) == EINVAL
    assert lib.pg_gp_gram_upper(p, 8, 8, p, 8, 0, None) == EINVAL  # h is x
    assert lib.pg_gp_gram_upper(p, 8, 8, p + 64, 8, 1, None) == EINVAL and lib.pg_gp_gram_upper(p, 8, 8, p + 64, 8, 128, None) == EINVAL
    good = [p, 2, 8, 2, 1.0, 1.0, p, 8, p, 8, 1, p, 3, p, None]
    for k in (0, 6, 8, 11, 13):
        args = list(good)
        args[k] = None
        assert lib.pg_gp_se_mll_sums(*args) == EINVAL, k
    for k, low in ((1, 1), (7, 7), (9, 7), (12, 2)):  # the strides of x, h, alpha_t; a workspace one float short
        args = list(good)
        args[k] = low
        assert lib.pg_gp_se_mll_sums(*args) == EINVAL, k
    for std, lengthscale in ((1.0, 0.0), (1.0, -1.0), (0.0, 1.0), (float("nan"), 1.0), (1.0, float("nan"))):
        args = list(good)
        args[4], args[5] = std, lengthscale
        assert lib.pg_gp_se_mll_sums(*args) == EINVAL, (std, lengthscale)
    assert lib.pg_gp_se_mll_sums(p, 2, 65, 2, 1.0, 1.0, p, 65, p, 65, 1, p, 8, p, None) == EINVAL and b"workspace" in lib.pg_last_error()
    good = [p, 8, 8, p, 8, p, 8, 1, p, None]
    for k in (0, 3, 5, 8):
        args = list(good)
        args[k] = None
        assert lib.pg_gp_mll_value(*args) == EINVAL, k
    for k in (1, 4, 6):
        args = list(good)
        args[k] = 7
        assert lib.pg_gp_mll_value(*args) == EINVAL, k


def test_no_device_is_reported_only_for_accepted_problems(lib):
    """Every new entry point over the sweep: a refused problem is PG_ESHAPE on any machine; an accepted one is called only
    where there is no device (the operands are host memory) and must then say hipErrorNoDevice, nothing else."""
    _keep, p = _buf()
    no_gpu = not torch.cuda.is_available()
    calls = 0
    for n, d, pp in _sweep(seed=3, count=40) + [(8, 2, 1)]:
        n_ok, d_ok, p_ok = 1 <= n <= MAX_N, 1 <= d <= MAX_D, 1 <= pp <= MAX_P
        for uses_d, uses_p, call in _entries(lib, p, n, d, pp):
            accepted = n_ok and (d_ok or not uses_d) and (p_ok or not uses_p)
            if not accepted:
                assert call() == ESHAPE, (n, d, pp)
            elif no_gpu:
                assert call() == NO_DEVICE and b"no HIP device" in lib.pg_last_error(), (n, d, pp)
                calls += 1
    if no_gpu:
        assert calls > 200


# ---------------------------------------------------------------------------------------------
# the float64 closed forms
def _problem(n, d, p, seed):
    g = torch.Generator().manual_seed(seed)
    x = 4.0 * torch.rand(n, d, generator=g, dtype=torch.float64)
    y = torch.sin(x.sum(1, keepdim=True)) + 0.3 * torch.randn(n, p, generator=g, dtype=torch.float64)
    return x, y


@pytest.mark.parametrize("n,d,p", [(50, 2, 3), (65, 17, 1)])
def test_closed_forms_equal_float64_autograd(n, d, p):
    x, y = _problem(n, d, p, seed=n)
    hyper = (1.3, 0.7 if d < 10 else 3.0, 0.1, 0.2)
    value, grads = mref.closed_form(x, y, *hyper)
    want, want_grads = mref.autograd_form(x, y, *hyper)
    err = abs(float(value - want)) / abs(float(want))
    print(f"[gp mll] closed form n={n} d={d} p={p}: value {err:.2e}")
    assert err <= CLOSED_FORM_TOL
    for name in mref.NAMES:
        err = abs(float(grads[name] - want_grads[name])) / abs(float(want_grads[name]))
        print(f"[gp mll]   d/d {name}: {err:.2e}")
        assert err <= CLOSED_FORM_TOL, name
    # the operand-level forms the GPU tests use give the same numbers from the same factor
    kf = hyper[0] ** 2 * torch.exp(-mref.sq_dists(x) / (2.0 * hyper[1] ** 2))
    l = torch.linalg.cholesky(kf + hyper[2] * torch.eye(n, dtype=torch.float64))
    zt = torch.linalg.solve_triangular(l, y - hyper[3], upper=False).t()
    xinv = mref.tri_inverse_t(l)
    assert float(xinv.tril(-1).abs().max()) == 0.0
    alpha_t = zt @ xinv.t()
    sums, sizes = mref.se_sums(x, hyper[0], hyper[1], mref.gram_upper(xinv), alpha_t)
    for k, name in enumerate(("std", "lengthscale", "noise_var")):
        assert abs(float(sums[k] - want_grads[name])) <= 1e-9 * float(sizes[k]), name
    both = mref.value_sums(l, zt, alpha_t)
    assert abs(float(both[0] - want)) <= CLOSED_FORM_TOL * abs(float(want))
    assert abs(float(both[1] - want_grads["value"])) <= 1e-9 * float(alpha_t.abs().sum())


def test_adam_loop_ascends():
    x, y = _problem(40, 2, 1, seed=5)
    seen, final = mref.adam_loop(x, y, (1.0, 1.0, 1.0, 0.0), n_steps=20)
    assert len(seen) == 20 and seen[-1] > seen[0] and all(v > 0 for v in final[:3])
    _, fixed = mref.adam_loop(x, y, (1.0, 1.0, 0.5, 0.25), n_steps=3, learn_noise=False, learn_mean=False)
    assert fixed[2:] == (0.5, 0.25)


# ---------------------------------------------------------------------------------------------
# the model's side
def test_model_raises():
    gp = gp_mod()
    model = gp.GaussianProcess(gp.Const(), gp.SquaredExponential(), 0.1)
    with pytest.raises(ValueError, match="fit"):
        model.log_marginal_likelihood()
    with pytest.raises(ValueError, match="fit"):
        model.optimize_hyperparameters()
    for other in (gp.GaussianProcess(gp.Const(), lambda a, b: a @ b.t(), 0.1), gp.GaussianProcess(lambda x: x[:, :1] * 0, gp.SquaredExponential(), 0.1)):
        other.fit(torch.zeros(3, 2), torch.zeros(3, 1))
        with pytest.raises(NotImplementedError, match="callable"):
            other.log_marginal_likelihood()
        with pytest.raises(NotImplementedError, match="callable"):
            other.optimize_hyperparameters()
    model.fit(torch.zeros(3, 2), torch.zeros(3, 1))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        model.log_marginal_likelihood()


def test_autograd_node_serves_the_tensors_that_require_grad(monkeypatch):
    """The node without a device: the kernels' results are stood in for by fixed numbers. A float hyperparameter gets no
    gradient, noise_var only after requires_grad_(), and under no_grad the gradients are not even asked for."""
    gp = gp_mod()
    model = gp.GaussianProcess(gp.Const(), gp.SquaredExponential(std=1.5), 0.1)  # std a Python float
    model.fit(torch.zeros(3, 2), torch.zeros(3, 1))
    asked = []

    def fake(want_grads):
        asked.append(want_grads)
        out = torch.tensor([-7.0, 0.5, 2.0, 3.0, 4.0])  # value, then d/d value, std, lengthscale, noise_var
        return out[0], (out[1:] if want_grads else None)

    monkeypatch.setattr(model, "_evidence", fake)
    value = model.log_marginal_likelihood()
    assert value.shape == () and float(value.detach()) == -7.0 and value.requires_grad and asked == [True]
    (3.0 * value).backward()
    assert float(model.mean.value.grad) == 1.5 and float(model.kernel.lengthscale.grad) == 9.0
    assert model.noise_var.grad is None and model.kernel.std == 1.5
    model.noise_var.requires_grad_()
    model.log_marginal_likelihood().backward()
    assert float(model.noise_var.grad) == 4.0 and float(model.kernel.lengthscale.grad) == 12.0  # accumulated
    with torch.no_grad():
        assert not model.log_marginal_likelihood().requires_grad and asked[-1] is False
    plain = gp.GaussianProcess(gp.Const(0.0), gp.SquaredExponential(1.0, 1.0), 0.1)
    plain.fit(torch.zeros(3, 2), torch.zeros(3, 1))
    monkeypatch.setattr(plain, "_evidence", fake)
    assert not plain.log_marginal_likelihood().requires_grad and asked[-1] is False


def test_optimizer_writes_back_in_place(monkeypatch):
    """The loop without a device, on constant stand-in gradients (all uphill): every learned tensor moves up by about lr per
    step on its own scale and is written IN PLACE (its _version moves, which is what the factor key watches); a float and
    whatever learn_noise / learn_mean exclude stay."""
    gp = gp_mod()
    model = gp.GaussianProcess(gp.Const(), gp.SquaredExponential(lengthscale=2.0), 0.5)  # lengthscale a Python float
    model.fit(torch.zeros(3, 2), torch.zeros(3, 1))
    monkeypatch.setattr(model, "_evidence", lambda want: (torch.tensor(-7.0), torch.tensor([0.5, 2.0, 3.0, 4.0])))
    std, value, noise = model.kernel.std, model.mean.value, model.noise_var
    versions = [t._version for t in (std, value, noise)]
    seen = model.optimize_hyperparameters(n_steps=2, lr=0.1, learn_noise=False)
    assert seen == [-7.0, -7.0]
    assert model.kernel.std is std and model.mean.value is value and model.noise_var is noise
    assert std._version > versions[0] and value._version > versions[1] and noise._version == versions[2]
    assert abs(float(std.detach().log()) - 0.2) < 0.02 and abs(float(value.detach()) - 0.2) < 0.02
    assert model.kernel.lengthscale == 2.0 and float(noise) == 0.5
    model.optimize_hyperparameters(n_steps=1, lr=0.1, learn_mean=False)
    assert abs(float(noise.log()) - (np.log(0.5) + 0.1)) < 1e-3 and abs(float(value.detach()) - 0.2) < 0.02
    silent = gp.GaussianProcess(gp.Const(), gp.SquaredExponential())  # noise_var = 0 is not learned
    silent.fit(torch.zeros(3, 2), torch.zeros(3, 1))
    monkeypatch.setattr(silent, "_evidence", lambda want: (torch.tensor(-7.0), torch.tensor([0.5, 2.0, 3.0, 4.0])))
    silent.optimize_hyperparameters(n_steps=1)
    assert float(silent.noise_var) == 0.0


def test_operators_have_no_cpu_fallback(lib):
    import pytorch_generative_amd as pg
    from pytorch_generative_amd import ops

    for name in ("gp_mll_plan", "tri_inverse_t", "gram_upper_", "se_mll_sums", "mll_value"):
        assert callable(getattr(pg.ops, name)), name
    a = torch.eye(4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.tri_inverse_t(a)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.gram_upper_(a.clone(), a)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.se_mll_sums(a, 1.0, 1.0, a, a[:1])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.mll_value(a, a[:1], a[:1])
    with pytest.raises(ValueError):
        ops.tri_inverse_t(torch.zeros(4))
    with pytest.raises(ValueError):
        ops.tri_inverse_t(torch.eye(4, requires_grad=True))
