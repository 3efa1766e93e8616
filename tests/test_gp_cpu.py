"""CPU: the Gaussian process without a device — pg_gp_plan over a sweep of (n, m, d, p) up to the domain's edges and beyond;
every entry point refuses what the plan refuses and reports a missing device only for a call it accepted; the float64 closed
forms of tests/_gp_ref.py against the reference's recorded results (tests/golden/gp/cases.pt); the public surface and the
drop-in alias. (The helper's own self-checks are in tests/test_gp_ref_cpu.py.)"""

import ctypes
import os
import random

import numpy as np
import pytest
import torch

import _gp_ref as gref
import _util

FIXTURES = os.path.join(_util.GOLDEN_DIR, "gp", "cases.pt")
PLAN_INTS = 16
EINVAL, ESHAPE, NO_DEVICE = -1, -2, 100  # hipErrorNoDevice
MAX_N, MAX_D, MAX_P = 16384, 4096, 4096
LOWER, MIRROR, DIAG, PLUS, B_TRANS, SE_DIRECT, SE_MFMA = 1, 2, 4, 8, 16, 32, 64
GATE = 1e-4


def load_cases():
    return torch.load(FIXTURES, map_location="cpu", weights_only=False)["cases"]


def gp_mod():
    from pytorch_generative_amd.models import gaussian_process

    return gaussian_process


def _plan(lib, n, m, d, p):
    out = (ctypes.c_longlong * PLAN_INTS)()
    rc = lib.pg_gp_plan(n, m, d, p, out, PLAN_INTS)
    return rc, list(out)


def _sweep(seed=0, count=400):
    rng = random.Random(seed)
    edge_n = (1, 2, 63, 64, 65, 128, 129, 4096, MAX_N - 1, MAX_N)
    shapes = [(n, m, d, p) for n in edge_n for m in (1, 64, 65, MAX_N) for d, p in ((1, 1), (16, 1), (17, 3), (MAX_D, MAX_P))]
    shapes += [(rng.randint(1, MAX_N), rng.randint(1, MAX_N), rng.randint(1, MAX_D), rng.randint(1, MAX_P)) for _ in range(count)]
    shapes += [(rng.randint(1, 300), rng.randint(1, 300), rng.randint(1, 40), rng.randint(1, 4)) for _ in range(count)]
    bad = (0, -1, MAX_N + 1, 1 << 20)
    shapes += [(n, 8, 2, 1) for n in bad] + [(8, m, 2, 1) for m in bad]
    shapes += [(8, 8, d, 1) for d in (0, -3, MAX_D + 1)] + [(8, 8, 2, p) for p in (0, -3, MAX_P + 1)]
    return shapes


def test_plan_domain_and_geometry(lib):
    from pytorch_generative_amd import ops

    for n, m, d, p in _sweep():
        rc, out = _plan(lib, n, m, d, p)
        inside = 1 <= n <= MAX_N and 1 <= m <= MAX_N and 1 <= d <= MAX_D and 1 <= p <= MAX_P
        assert rc == (0 if inside else ESHAPE), (n, m, d, p, rc)
        if rc:
            assert lib.pg_last_error() and ops.gp_plan(n, m, d, p) is None
            continue
        (tile, kc, panels, row_tiles, route, direct_d, sym_tiles, cross_tiles, potrf_launches, trsm_launches, trailing, max_n, max_d,
         max_p, p_tiles, forced_d) = out
        assert (tile, kc, direct_d, forced_d, max_n, max_d, max_p) == (64, 32, 16, 64, MAX_N, MAX_D, MAX_P)
        assert panels == -(-n // 64) and row_tiles == -(-m // 64) and p_tiles == -(-p // 64)
        assert route == int(d > 16)
        assert sym_tiles == panels * (panels + 1) // 2 and cross_tiles == panels * row_tiles
        assert potrf_launches == 3 * panels - 2 <= 3 * panels and trsm_launches == 2 * panels - 1
        assert trailing == (panels - 1) ** 2
        assert (n - 1) * n + n - 1 < 2 ** 31  # element offsets of a dense (n, n) matrix fit 32 bits
        assert ops.gp_plan(n, m, d, p)["panels"] == panels
    assert lib.pg_gp_plan(8, 8, 1, 1, (ctypes.c_longlong * PLAN_INTS)(), PLAN_INTS - 1) == EINVAL  # short array
    assert lib.pg_gp_plan(8, 8, 1, 1, None, PLAN_INTS) == EINVAL


def _buf():
    buf = np.zeros(1 << 12, dtype=np.float32)
    return buf, buf.ctypes.data


def test_launches_refuse_what_the_plan_refuses(lib):
    """Host side only: every check comes before the device is looked for, so these statuses are those of any machine."""
    _keep, p = _buf()
    for n in (0, -1, MAX_N + 1):
        assert lib.pg_gp_potrf(p, 1 << 20, n, 0, p, None) == ESHAPE
        assert lib.pg_gp_trsm_right(p, 1 << 20, n, p, 1 << 20, 4, 0, 0, None) == ESHAPE
        assert lib.pg_gp_trsm_right(p, 64, 8, p, 64, n, 0, 0, None) == ESHAPE
        assert lib.pg_gp_se_kernel(p, 4, n, p, 4, 8, 2, 1.0, 1.0, 0.0, p, 1 << 20, 0, 0, None) == ESHAPE
        assert lib.pg_gp_se_kernel(p, 4, 8, p, 4, n, 2, 1.0, 1.0, 0.0, p, 1 << 20, 0, 0, None) == ESHAPE
        assert lib.pg_gp_gemm_nt(p, 64, p, 64, p, 1 << 20, n, 8, 8, 0, 0, None) == ESHAPE
        assert lib.pg_gp_gemm_nt(p, 64, p, 64, p, 64, 8, n, 8, 0, 0, None) == ESHAPE
        assert lib.pg_gp_gemm_nt(p, 1 << 20, p, 1 << 20, p, 64, 8, 8, n, 0, 0, None) == ESHAPE
        assert lib.pg_gp_add_diag(p, 1 << 20, n, 1.0, None) == ESHAPE
        assert lib.pg_gp_trsm_diag(p, 64, p, 64, n, 8, 0, 0, None) == ESHAPE
    for d in (0, MAX_D + 1):
        assert lib.pg_gp_se_kernel(p, 1 << 20, 8, p, 1 << 20, 8, d, 1.0, 1.0, 0.0, p, 8, 0, 0, None) == ESHAPE
    assert lib.pg_gp_se_kernel(p, 65, 8, p, 65, 8, 65, 1.0, 1.0, 0.0, p, 8, 0, SE_DIRECT, None) == ESHAPE  # forced route 0 above d = 64
    assert lib.pg_gp_potrf(p, 64, 8, 9, p, None) == ESHAPE and lib.pg_gp_potrf(p, 64, 8, -1, p, None) == ESHAPE  # n_done outside 0 .. n
    assert lib.pg_gp_trsm_right(p, 64, 8, p, 64, 4, 9, 0, None) == ESHAPE
    for jb, done in ((0, 0), (65, 0), (8, 9), (8, -1)):
        assert lib.pg_gp_potrf_diag(p, 64, jb, done, 0, p, None) == ESHAPE
        assert lib.pg_gp_trsm_diag(p, 64, p, 64, 4, jb, done, 0, None) == ESHAPE
    assert lib.pg_gp_potrf_diag(p, 64, 8, 0, MAX_N - 7, p, None) == ESHAPE and lib.pg_gp_potrf_diag(p, 64, 8, 0, 2 ** 31 - 1, p, None) == ESHAPE
    # null pointers, row strides below the row length, flags
    assert lib.pg_gp_potrf(None, 64, 8, 0, p, None) == EINVAL and lib.pg_gp_potrf(p, 64, 8, 0, None, None) == EINVAL
    assert lib.pg_gp_potrf(p, 7, 8, 0, p, None) == EINVAL
    assert lib.pg_gp_trsm_right(p, 8, 8, p, 7, 4, 0, 0, None) == EINVAL and lib.pg_gp_trsm_right(p, 7, 8, p, 8, 4, 0, 0, None) == EINVAL
    assert lib.pg_gp_trsm_right(None, 8, 8, p, 8, 4, 0, 0, None) == EINVAL
    assert lib.pg_gp_trsm_right(p, 8, 8, p, 8, 4, 3, 1, None) == EINVAL  # the X L = B form completes no columns
    assert lib.pg_gp_trsm_diag(p, 8, p, 8, 4, 8, 3, 1, None) == EINVAL
    for k in range(3):
        args = [p, 8, p, 8, p, 8]
        args[2 * k] = None
        assert lib.pg_gp_gemm_nt(*args, 8, 8, 8, 0, 0, None) == EINVAL, k
        args = [p, 8, p, 8, p, 8]
        args[2 * k + 1] = 7
        assert lib.pg_gp_gemm_nt(*args, 8, 8, 8, 0, 0, None) == EINVAL, k
    assert lib.pg_gp_gemm_nt(p, 8, p, 8, p, 8, 8, 8, 8, 0, 128, None) == EINVAL  # unknown flag
    assert lib.pg_gp_gemm_nt(p, 8, p, 8, p, 8, 8, 8, 8, 0, MIRROR, None) == EINVAL  # the mirror needs lower
    assert lib.pg_gp_gemm_nt(p, 8, p, 8, p, 8, 8, 4, 8, 0, LOWER | MIRROR, None) == EINVAL  # and a square update
    assert lib.pg_gp_gemm_nt(p, 8, p, 4, p, 8, 8, 8, 4, 0, B_TRANS, None) == EINVAL  # b read as (K, C): its rows hold C floats
    assert lib.pg_gp_se_kernel(p, 2, 8, p, 2, 8, 2, 1.0, 0.0, 0.0, p, 8, 0, 0, None) == EINVAL and b"lengthscale" in lib.pg_last_error()
    assert lib.pg_gp_se_kernel(p, 2, 8, p, 2, 8, 2, 1.0, 1.0, 0.0, p, 7, 0, 0, None) == EINVAL
    assert lib.pg_gp_se_kernel(p, 2, 8, p, 2, 8, 2, 1.0, 1.0, 0.0, p, 8, 0, SE_DIRECT | SE_MFMA, None) == EINVAL
    assert lib.pg_gp_se_kernel(p, 2, 8, p + 64, 2, 8, 2, 1.0, 1.0, 0.0, p, 8, 0, LOWER | MIRROR, None) == EINVAL  # mirror: a is b
    assert lib.pg_gp_add_diag(None, 8, 8, 1.0, None) == EINVAL and lib.pg_gp_add_diag(p, 7, 8, 1.0, None) == EINVAL


def test_no_device_is_reported_only_for_accepted_problems(lib):
    """Every entry point over the sweep: a refused problem is PG_ESHAPE on any machine; an accepted one is called only where
    there is no device (the operands are host memory) and must then say hipErrorNoDevice, nothing else."""
    _keep, p = _buf()
    no_gpu = not torch.cuda.is_available()
    ld = 1 << 20
    calls = 0
    for n, m, d, _ in _sweep(seed=2, count=40) + [(8, 8, 2, 1)]:
        n_ok, m_ok, d_ok = 1 <= n <= MAX_N, 1 <= m <= MAX_N, 1 <= d <= MAX_D
        entries = (
            (n_ok and m_ok and d_ok, lambda: lib.pg_gp_se_kernel(p, ld, n, p, ld, m, d, 1.0, 1.0, 0.1, p, ld, 0, 0, None)),
            (n_ok and m_ok, lambda: lib.pg_gp_gemm_nt(p, ld, p, ld, p, ld, n, m, 8, 0, 0, None)),
            (n_ok and m_ok, lambda: lib.pg_gp_trsm_right(p, ld, n, p, ld, m, n // 2 if n_ok else 0, 0, None)),
            (n_ok, lambda: lib.pg_gp_potrf(p, ld, n, n // 3 if n_ok else 0, p, None)),
            (n_ok, lambda: lib.pg_gp_add_diag(p, ld, n, 0.5, None)),
            (m_ok, lambda: lib.pg_gp_trsm_diag(p, 64, p, 64, m, 64, 0, 1, None)),
        )
        for accepted, call in entries:
            if not accepted:
                assert call() == ESHAPE, (n, m, d)
            elif no_gpu:
                assert call() == NO_DEVICE and b"no HIP device" in lib.pg_last_error(), (n, m, d)
                calls += 1
    if no_gpu:
        assert calls > 200
        assert lib.pg_gp_potrf_diag(p, 64, 64, 3, 128, p, None) == NO_DEVICE


# ---------------------------------------------------------------------------------------------
# the float64 closed forms against the reference's recorded results
@pytest.mark.parametrize("name", sorted(load_cases()))
def test_closed_form_reproduces_the_fixture(name):
    """The maker asserted that the reference's float32 results lie within a quarter of the gate of these closed forms; the
    same quarter is asked here of the recorded tensors."""
    case = load_cases()[name]
    noise = float(torch.tensor(case["noise_var"], dtype=torch.float32))
    assert case["cond"] <= 1e3
    prior_max = float(gref.se(case["x"], case["x"], case["std"], case["lengthscale"]).abs().max())
    for tag, hi in (("", case["n1"]), ("2", case["n"])):
        mu, sig = gref.posterior(case["train_x"][:hi], case["train_y"][:hi], case["x"], case["std"], case["lengthscale"], case["value"],
                                 noise)
        assert mu.shape == (case["m"], case["p"]) and sig.shape == (case["m"], case["m"])
        e_mu = float((case["mu" + tag].double() - mu).abs().max() / mu.abs().max())
        e_sig = float((case["sig" + tag].double() - sig).abs().max()) / prior_max
        print(f"[gp] {name}{tag}: mu {e_mu:.2e}, sig {e_sig:.2e}")
        assert e_mu <= GATE / 4 and e_sig <= GATE / 4, (name, tag, e_mu, e_sig)


# ---------------------------------------------------------------------------------------------
# the public surface
def test_alias_serves_the_module():
    import pytorch_generative_amd as pg
    import pytorch_generative_amd.compat as compat

    compat.install_alias()
    import pytorch_generative.models.gaussian_process as aliased

    assert aliased is gp_mod() is pg.models.gaussian_process
    assert not hasattr(pg.models, "GaussianProcess")  # as in the reference: no top-level name
    for name in ("se_kernel", "cholesky_", "trsm_right_", "gemm_nt_", "gp_plan"):
        assert callable(getattr(pg.ops, name)), name


def test_constructor_state_and_routes():
    gp = gp_mod()
    model = gp.GaussianProcess(gp.Const(), gp.SquaredExponential(), 0.25)
    assert list(model.state_dict()) == ["noise_var", "mean.value", "kernel.std", "kernel.lengthscale"]
    assert model.noise_var.dtype == torch.float32 and float(model.noise_var) == 0.25
    assert float(gp.GaussianProcess(gp.Const(), gp.SquaredExponential()).noise_var) == 0.0
    assert model._kernel_route == "se" and model.incremental is True and model._factor_route is None
    assert gp.GaussianProcess(lambda x: x[:, :1] * 0, gp.SquaredExponential())._kernel_route == "callable"
    assert gp.GaussianProcess(gp.Const(), lambda a, b: a @ b.t())._kernel_route == "callable"
    kernel = gp.SquaredExponential(std=2.0, lengthscale=0.5)
    assert kernel.hyperparameters() == (2.0, 0.5) and list(kernel.state_dict()) == []
    assert gp.Const(3.0)(torch.zeros(4, 2)).tolist() == [[3.0]] * 4
    # a tensor hyperparameter is read again after an in-place change
    kernel = gp.SquaredExponential()
    assert kernel.hyperparameters() == (1.0, 1.0)
    with torch.no_grad():
        kernel.lengthscale.fill_(0.5)
    assert kernel.hyperparameters() == (1.0, 0.5)


def test_fit_appends_and_checks():
    gp = gp_mod()
    model = gp.GaussianProcess(gp.Const(), gp.SquaredExponential(), 0.1)
    model.fit(torch.zeros(3, 2), torch.zeros(3, 1))
    model.fit(torch.ones(2, 2), torch.ones(2, 1))
    assert model.train_x.shape == (5, 2) and model.train_y.shape == (5, 1) and model._n_factored == 0
    with pytest.raises(ValueError):
        model.fit(torch.zeros(3, 2), torch.zeros(4, 1))
    with pytest.raises(ValueError):
        model.fit(torch.zeros(3, 2, requires_grad=True), torch.zeros(3, 1))
    with pytest.raises(ValueError):
        model.predict(torch.zeros(3, 2, requires_grad=True))


def test_operators_have_no_cpu_fallback(lib):
    from pytorch_generative_amd import ops

    a = torch.eye(4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.cholesky_(a)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.se_kernel(a, a, 1.0, 1.0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.trsm_right_(a, a.clone())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.gemm_nt_(a.clone(), a, a)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        gp_mod().GaussianProcess(gp_mod().Const(), gp_mod().SquaredExponential()).predict(a)
    with pytest.raises(ValueError):
        ops.cholesky_(torch.zeros(4))
