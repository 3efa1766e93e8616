"""CPU: tests/_small_ref.py (the float64 references of the elementwise, LayerNorm, loss and resampling kernels) is
pinned against oracle/ops.py and torch.nn.functional in float64, and the inputs of tests/test_gpu_small_kernels.py are
shown to be fair: a float32 evaluation of every reference on every input set stays inside the bound the GPU tier
applies, with a factor 2 to spare (so a miss on the GPU is the kernel's). The largest absolute error of the float32
restatement of each transcendental kernel is measured on those inputs and pinned to the constants the GPU tier scales
its element-wise bound from. Three planted errors (unbiased variance, `s` for `1 - s` in the gate gradient, a dropped
last row of the broadcast sum) are shown to fall outside the bounds. The host-side refusals of the entry points return
their error code before any launch (dummy pointers, no device)."""

import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _small_ref as sref
import _util
from oracle import ops as oops
from test_cpu_gelu import gelu_parts

PIN = 1e-12
F32 = torch.float32
ACT_ALL_N = sref.ACT_N + (sref.ACT_N_BIG_ALIGNED, sref.ACT_N_BIG_UNALIGNED)
GATED_ALL = sref.GATED_VEC + sref.GATED_SCALAR + (sref.GATED_BIG,)


def _pin(got, want, what):
    assert got.dtype == torch.float64 and got.shape == want.shape, what
    assert float((got - want).abs().max()) <= PIN * max(float(want.abs().max()), 1.0), what


def _grad(fn, *leaves_and_dy):
    *leaves, dy = leaves_and_dy
    leaves = [t.double().clone().requires_grad_(True) for t in leaves]
    return torch.autograd.grad((fn(*leaves) * dy.double()).sum(), leaves)


# ---------------------------------------------------------------------------------------------
# the references are the functions they claim to be
def test_activation_references_are_torch_in_float64():
    x, dy = sref.act_inputs(4096)
    for name, fn in (("relu", F.relu), ("elu", F.elu), ("gelu", F.gelu)):
        _pin(sref.ACT_FWD[name](x), fn(x.double()), name)
        if name != "relu":                                    # relu'(0): torch's convention is 0 as well, but untested
            _pin(dy.double() * sref.ACT_GRAD[name](x), _grad(fn, x, dy)[0], name + " grad")
    nz = x != 0
    _pin((dy.double() * sref.relu_grad(x))[nz], _grad(F.relu, x, dy)[0][nz], "relu grad")
    assert float(sref.relu_grad(torch.zeros(1))) == 0.0 and float(sref.relu_grad_from_out(torch.zeros(1))) == 0.0
    # the derivative from the output is the derivative from the input (y - res recovers elu(pre) up to rounding)
    pre = x.double()
    res = dy.double()
    _pin(sref.elu_grad_from_out(sref.elu(pre) + res, res), sref.elu_grad(pre), "elu from out")
    assert torch.equal(sref.relu_grad_from_out(sref.relu(pre)), sref.relu_grad(pre))
    big = pre.abs() > 1e-3                                    # (a pre-activation of 1e-38 is absorbed by res)
    assert torch.equal(sref.relu_grad_from_out(sref.relu(pre) + res, res)[big], sref.relu_grad(pre)[big])


def test_gate_and_concat_elu_references_are_the_oracle_in_float64():
    x, dy, res = sref.gated_inputs(3, 5, 64)
    for kind, gate in sref.GATES.items():
        want = oops.gated_activation(x.double(), kind)
        _pin(sref.gated_fwd(x, gate), want, kind)
        _pin(sref.gated_fwd(x, gate, res), want + res.double(), kind + " + res")
        _pin(sref.gated_bwd(x, dy, gate), _grad(lambda t: oops.gated_activation(t, kind), x, dy)[0], kind + " grad")
    # the sigmoid keeps its digits at -30 (plain 1 - sigmoid(30) has lost three of them in float64)
    b = torch.tensor([30.0, -30.0], dtype=torch.float64)
    assert float((sref.sigmoid(-b)[0] / torch.exp(b[1]) - 1.0).abs()) < 1e-12
    assert bool(torch.isfinite(sref.sigmoid(torch.tensor([1000.0, -1000.0]).float())).all())
    xc, dyc = sref.rand(3, 7, 5), sref.rand(3, 14, 5, salt=1)
    cat = lambda t: F.elu(torch.cat((t, -t), dim=1))
    _pin(sref.concat_elu_fwd(xc), cat(xc.double()), "concat elu")
    _pin(sref.concat_elu_bwd(xc, dyc), _grad(cat, xc, dyc)[0], "concat elu grad")


def test_loss_references_are_the_oracle_in_float64():
    for fractional in (False, True):
        z, x = sref.bce_inputs(4, 784, fractional)
        _pin(sref.bce(z, x), oops.bce_sum_mean(z.double(), x.double()), "bce")
        zl = z.double().requires_grad_(True)
        (g,) = torch.autograd.grad(oops.bce_sum_mean(zl, x.double()) * 1.7, zl)
        _pin(sref.bce_grad(z, x, 1.7), g, "bce grad")
    a, b = sref.mse_inputs(1000)
    _pin(sref.mse(a, b), F.mse_loss(a.double(), b.double()), "mse")
    al, bl = a.double().requires_grad_(True), b.double().requires_grad_(True)
    ga, gb = torch.autograd.grad(F.mse_loss(al, bl) * -0.6, (al, bl))
    da, db = sref.mse_grad(a, b, -0.6)
    _pin(da, ga, "mse da")
    _pin(db, gb, "mse db")


@pytest.mark.parametrize("C", [1, 2, 17, 65])
def test_layernorm_reference_is_the_oracle_in_float64(C):
    x, gamma, beta, dy, dx_add = sref.ln_inputs(3, C, 49)
    r = sref.layernorm(x, gamma, beta, dy, dx_add)
    leaves = [t.double().clone().requires_grad_(True) for t in (x, gamma, beta)]
    y = oops.nchw_layernorm(leaves[0].unsqueeze(3), leaves[1], leaves[2], sref.LN_EPS).squeeze(3)
    dx, dg, db = torch.autograd.grad((y * dy.double()).sum(), leaves)
    _pin(r["y"], y.detach(), "y")
    _pin(r["dx"], dx, "dx")
    _pin(r["dgamma"], dg, "dgamma")
    _pin(r["dbeta"], db, "dbeta")
    _pin(r["dx_res"], dx + dx_add.double(), "dx + dx_add")
    _pin(r["mean"], x.double().mean(dim=1), "mean")
    _pin(r["rstd"], 1.0 / torch.sqrt(x.double().var(dim=1, unbiased=False) + sref.LN_EPS), "rstd")


def test_resampling_references_are_torch():
    x = sref.rand(6, 14, 6).double()
    _pin(sref.avgpool2_fwd(x), F.avg_pool2d(x[None], 2)[0], "avgpool")
    _pin(sref.upsample2_fwd(x), F.interpolate(x[None], scale_factor=2, mode="nearest")[0], "upsample")
    dy = sref.rand(6, 7, 3, salt=1)
    _pin(sref.avgpool2_bwd(dy.double()), _grad(lambda t: F.avg_pool2d(t[None], 2)[0], x, dy)[0], "avgpool bwd")
    dyu = sref.rand(6, 28, 12, salt=2)
    _pin(sref.upsample2_bwd(dyu.double()),
         _grad(lambda t: F.interpolate(t[None], scale_factor=2, mode="nearest")[0], x, dyu)[0], "upsample bwd")
    want = F.pixel_unshuffle(x[None], 2)[0].reshape(6, 4, 7, 3).transpose(0, 1)    # channel = plane * 4 + 2 pr + pc
    assert torch.equal(sref.phase_split(x), want)
    assert torch.equal(sref.col_zero_insert2(x.reshape(-1, 6))[:, 0::2], x.reshape(-1, 6))
    assert torch.equal(sref.col_subsample2(sref.col_zero_insert2(x.reshape(-1, 6))), x.reshape(-1, 6))
    assert float(sref.col_zero_insert2(x.reshape(-1, 6))[:, 1::2].abs().max()) == 0.0
    # the three same-order references are float32 and the stated order
    xf = sref.rand(3, 4, 10)
    assert sref.avgpool2_fwd(xf).dtype == F32 and sref.upsample2_bwd(xf).dtype == F32
    a, b, c, d = (float(v) for v in (xf[0, 0, 0], xf[0, 0, 1], xf[0, 1, 0], xf[0, 1, 1]))
    f = np.float32
    assert float(sref.upsample2_bwd(xf)[0, 0, 0]) == float((f(a) + f(b)) + (f(c) + f(d)))
    assert float(sref.avgpool2_fwd(xf)[0, 0, 0]) == float(f(0.25) * ((f(a) + f(b)) + (f(c) + f(d))))
    rows = [sref.rand(2, 5, salt=k) for k in range(3)]
    assert float(sref.sum_rows(rows)[1, 2]) == float(((f(0) + f(rows[0][1, 2])) + f(rows[1][1, 2])) + f(rows[2][1, 2]))
    src, dst = torch.arange(20.0), torch.full((16,), 100.0)
    got = sref.copy_rows(src, dst, 2, 3, 10, 5, 1)
    assert got.tolist() == [100, 101, 102, 100, 100, 110, 111, 112] + [100] * 8


# ---------------------------------------------------------------------------------------------
# float32 restatements on the GPU tier's inputs: inside the bounds with a factor 2, and the measured absolute figures
def _gelu_f32(x, dy):
    cdf, e = gelu_parts(x.numpy())
    f = np.float32
    fwd = (x.numpy() * cdf).astype(f)
    bwd = (dy.numpy() * (cdf + x.numpy() * f(0.39894228040143267794) * e).astype(f)).astype(f)
    return torch.from_numpy(fwd), torch.from_numpy(bwd)


def _abs_err(got, want):
    return float((got.double() - want).abs().max())


def _measure():
    """name -> (largest absolute error, largest max-normalised error) of the float32 restatement over every input set
    the GPU tier feeds that kernel."""
    worst = {}

    def note(name, got, want):
        a, r = worst.get(name, (0.0, 0.0))
        worst[name] = (max(a, _abs_err(got, want)), max(r, _util.rel_err(got, want)))

    for n in ACT_ALL_N:
        x, dy = sref.act_inputs(n)
        note("elu_fwd", sref.elu(x, F32), sref.elu(x))
        note("elu_bwd", dy * sref.elu_grad(x, F32), dy.double() * sref.elu_grad(x))
        gf, gb = _gelu_f32(x, dy)
        note("gelu_fwd", gf, sref.gelu(x))
        note("gelu_bwd", gb, dy.double() * sref.gelu_grad(x))
    for n in sref.FROM_OUT_N:
        for with_res in (False, True):
            y, res, dy = sref.from_out_inputs(n, sref.ACT_ELU, with_res)
            note("elu_bwd_out", dy * sref.elu_grad_from_out(y, res, F32), dy.double() * sref.elu_grad_from_out(y, res))
    for N, C, L in GATED_ALL:
        x, dy, res = sref.gated_inputs(N, C, L)
        for kind, gate in sref.GATES.items():
            note(f"gated_{kind}_fwd", sref.gated_fwd(x, gate, None, F32), sref.gated_fwd(x, gate))
            note(f"gated_{kind}_fwd_res", sref.gated_fwd(x, gate, res, F32), sref.gated_fwd(x, gate, res))
            note(f"gated_{kind}_bwd", sref.gated_bwd(x, dy, gate, F32), sref.gated_bwd(x, dy, gate))
    for N, CL in sref.CONCAT_ELU:
        x, dy = sref.rand(N, 1, CL, salt=3) * 2.5, sref.rand(N, 2, CL, salt=4)
        note("concat_elu_fwd", sref.concat_elu_fwd(x, F32), sref.concat_elu_fwd(x))
        note("concat_elu_bwd", sref.concat_elu_bwd(x, dy, F32), sref.concat_elu_bwd(x, dy))
    return worst


def test_fp32_restatements_within_bounds_and_absolute_figures_pinned():
    """Every transcendental kernel's inputs: the float32 restatement stays below half the project's 1e-5 max-normalised
    bound, and its largest absolute error is the constant of _small_ref.CPU_ABS_ERR (not above it, and not below half of
    it: the constant is the measurement, rounded up)."""
    worst = _measure()
    assert set(worst) == set(sref.CPU_ABS_ERR)
    for name, (a, r) in sorted(worst.items()):
        print(f"[small] {name}: float32 restatement abs err {a:.3e} (constant {sref.CPU_ABS_ERR[name]:.1e}), "
              f"max-normalised {r:.3e}")
    for name, (a, r) in worst.items():
        assert r <= 0.5e-5, f"{name}: max-normalised {r:.3e}"
        assert 0.5 * sref.CPU_ABS_ERR[name] <= a <= sref.CPU_ABS_ERR[name], f"{name}: measured {a:.3e}"


def test_fp32_losses_within_half_the_bound():
    for N, per in sref.BCE_CASES:
        for fractional in (False, True):
            z, x = sref.bce_inputs(N, per, fractional)
            _util.assert_close(sref.bce(z, x, F32), sref.bce(z, x), 0.5e-5, f"bce {N} x {per}")
            _util.assert_close(sref.bce_grad(z, x, 1.7, F32), sref.bce_grad(z, x, 1.7), 0.5e-5, f"bce grad {N} x {per}")
    for n in sref.MSE_N:
        a, b = sref.mse_inputs(n)
        _util.assert_close(sref.mse(a, b, F32), sref.mse(a, b), 0.5e-5, f"mse {n}")
        _util.assert_close(sref.mse_grad(a, b, -0.6, F32)[0], sref.mse_grad(a, b, -0.6)[0], 0.5e-5, f"mse grad {n}")


def _ln_cases():
    cases = [(N, C, L) for C in sref.LN_C for N, L in sref.LN_NL]
    return cases + [(N, 17, L) for N, L in sref.LN_G_CASES] + [(1, 2048, 5)]


def _ln_excess(got, want, tol, floor):
    """-> the largest of: max-normalised error / tol over y, mean, rstd, dx, dx_res, dgamma, dbeta, and GradReport's
    element-wise ratio over dx, dgamma, dbeta. <= 1 passes."""
    worst = 0.0
    for k in ("y", "mean", "rstd", "dx", "dx_res", "dgamma", "dbeta"):
        m = float(want[k].abs().max())
        d = (got[k].double() - want[k]).abs()
        if m == 0.0:                                         # C = 1: dx and dgamma are exactly 0
            assert float(d.max()) == 0.0, k
            continue
        worst = max(worst, float(d.max()) / m / tol)
        if k in ("dx", "dgamma", "dbeta"):
            worst = max(worst, float((d / (tol * want[k].abs() + floor * m)).max()))
    return worst


@pytest.mark.parametrize("case", _ln_cases(), ids=lambda c: "x".join(map(str, c)))
def test_fp32_layernorm_within_half_the_bound(case):
    N, C, L = case
    args = sref.ln_inputs(N, C, L)
    excess = _ln_excess(sref.layernorm(*args, dtype=F32), sref.layernorm(*args), _util.GRAD_TOL, _util.GRAD_FLOOR)
    assert excess <= 0.5, f"float32 LayerNorm at {excess:.3f} of the bound"


@pytest.mark.parametrize("C", sref.LN_ZERO_VAR_C)
def test_fp32_layernorm_zero_variance_pixel_within_half_the_bound(C):
    args = sref.ln_zero_variance_inputs(C)
    got, want = sref.layernorm(*args, dtype=F32), sref.layernorm(*args)
    assert _ln_excess(got, want, _util.GRAD_TOL, _util.GRAD_FLOOR) <= 0.5
    assert torch.equal(want["y"][1, :, 3], args[2].double()) and torch.equal(got["y"][1, :, 3], args[2])
    assert bool(torch.isfinite(want["dx"]).all())


def test_fp32_broadcast_sum_within_half_the_bound():
    for N, per in sref.BCAST_CASES:
        _, _, dy, start = sref.bcast_inputs(N, per)
        got = (start + sref.bcast_colsum(dy, F32)).double()
        want = start.double() + sref.bcast_colsum(dy)
        if N == 1:                                           # one rounding: the sum itself
            assert torch.equal(got, (start + dy[0]).double())
        assert bool(((got - want).abs() <= 0.5 * sref.bcast_bwd_bound(dy, start)).all()), (N, per)


# ---------------------------------------------------------------------------------------------
# the bounds can fail: one planted error each
def test_mutations_fall_outside_the_bounds():
    # LayerNorm with the unbiased variance: every C > 1 of the sweep (C = 1 would divide by zero)
    for N, C, L in ((3, 2, 49), (3, 17, 49), (1, 65, 513), (1, 2048, 5)):
        args = sref.ln_inputs(N, C, L)
        bad = sref.layernorm(*args, unbiased=True)
        assert _ln_excess(bad, sref.layernorm(*args), _util.GRAD_TOL, _util.GRAD_FLOOR) > 1.0, (N, C, L)
        assert _util.rel_err(bad["y"], sref.layernorm(*args)["y"]) > 1e-4, (N, C, L)
    # the gate gradient with s for 1 - s: beyond the absolute bound and the 1e-5 bound on every input set
    for N, C, L in GATED_ALL[:-1]:
        x, dy, _ = sref.gated_inputs(N, C, L)
        for kind, gate in sref.GATES.items():
            want, bad = sref.gated_bwd(x, dy, gate), sref.gated_bwd(x, dy, gate, mutate=True)
            assert _abs_err(bad, want) > sref.ABS_FACTOR * sref.CPU_ABS_ERR[f"gated_{kind}_bwd"], (N, C, L, kind)
            assert _util.rel_err(bad, want) > 1e-5, (N, C, L, kind)
    # the broadcast sum without its last row (N = 1 has no other row: the sum is then 0, still outside)
    for N, per in sref.BCAST_CASES:
        _, _, dy, start = sref.bcast_inputs(N, per)
        want = start.double() + sref.bcast_colsum(dy)
        bad = start.double() + sref.bcast_colsum(dy, drop_last=True)
        assert bool(((bad - want).abs() > sref.bcast_bwd_bound(dy, start)).any()), (N, per)
        doubled = want + dy[-1].double()
        assert bool(((doubled - want).abs() > sref.bcast_bwd_bound(dy, start)).any()), (N, per)


# ---------------------------------------------------------------------------------------------
# host-side refusals: error code before any launch
P = 4096                          # a non-null, 16-byte aligned address that is never dereferenced
EINVAL, ESHAPE = -1, -2


def test_host_side_refusals_need_no_device(lib):
    """Each call returns its error code from the argument checks in front of the launch (read from the entry points:
    every PG_REQUIRE named here precedes the first hip call of its function). The rows / strides arrays of pg_sum_rows
    are host arrays and are real; every device pointer is the dummy P."""
    from pytorch_generative_amd import _lib

    ws = lib.pg_nchw_layernorm_bwd_workspace_floats(3, 17, 600)
    assert ws == 4 * 2 * 17                                   # ceil(1800 / 512) = 4 blocks, one partial row of 2 C each
    assert lib.pg_nchw_layernorm_bwd(P, P, P, P, P, P, P, P, 1, 2049, 5, P, 1 << 30, 0) == ESHAPE
    assert lib.pg_nchw_layernorm_bwd_res(P, P, P, P, P, P, P, P, P, 1, 2049, 5, P, 1 << 30, 0) == ESHAPE
    assert lib.pg_nchw_layernorm_bwd(P, P, P, P, P, P, P, P, 3, 17, 600, P, ws - 1, 0) == EINVAL
    with pytest.raises(ValueError, match="workspace too small"):
        _lib.check(EINVAL, "pg_nchw_layernorm_bwd")
    assert lib.pg_nchw_layernorm_bwd_res(P, P, P, P, P, P, P, P, P, 3, 17, 600, P, ws - 1, 0) == EINVAL
    for n in (1, 2, 3, 1027):
        assert lib.pg_act_bwd_from_out(P, P, P, P, n, sref.ACT_ELU, 0) == ESHAPE
    assert lib.pg_act_bwd_from_out(P, 0, P, P, 6, sref.ACT_RELU, 0) == ESHAPE
    assert lib.pg_act_bwd_from_out(P, P, P, P, 8, sref.ACT_GELU, 0) == EINVAL
    assert lib.pg_act_bwd_from_out(P, P + 4, P, P, 8, sref.ACT_ELU, 0) == ESHAPE     # a misaligned residual
    rows = (ctypes.c_void_p * 33)(*([P] * 33))
    strides = (ctypes.c_long * 33)(*([50] * 33))
    assert lib.pg_sum_rows(rows, None, 0, P, 3, 50, 0) == ESHAPE
    assert lib.pg_sum_rows(rows, None, 33, P, 3, 50, 0) == ESHAPE
    strides[1] = 49
    assert lib.pg_sum_rows(rows, strides, 2, P, 3, 50, 0) == EINVAL
    with pytest.raises(ValueError, match="batch stride of row 1"):
        _lib.check(EINVAL, "pg_sum_rows")
    assert lib.pg_copy_rows(P, P, 3, 6, 5, 6, 0, 0) == EINVAL
    assert lib.pg_copy_rows(P, P, 3, 6, 6, 5, 1, 0) == EINVAL
    assert lib.pg_col_subsample2(P, P, 7, 5, 0) == ESHAPE
    assert lib.pg_col_subsample2(P, P, 7, 1, 0) == ESHAPE
    assert lib.pg_gated_fwd_res(P, P, P, 2, 3, 7, sref.GATE_TANH, 0) == ESHAPE
    assert lib.pg_gated_fwd_res(P, P, P, 2, 3, 6, sref.GATE_IDENTITY, 0) == ESHAPE
    assert lib.pg_gated_fwd_res(P, P + 4, P, 2, 3, 8, sref.GATE_TANH, 0) == ESHAPE    # L % 4 == 0, residual misaligned
    for act in (0, 4, 7, -1):
        assert lib.pg_act_fwd(P, P, 8, act, 0) == EINVAL
        assert lib.pg_act_bwd(P, P, P, 8, act, 0) == EINVAL
    for gate in (2, -1):
        assert lib.pg_gated_fwd(P, P, 2, 3, 8, gate, 0) == EINVAL
        assert lib.pg_gated_fwd_res(P, P, P, 2, 3, 8, gate, 0) == EINVAL
        assert lib.pg_gated_bwd(P, P, P, 2, 3, 8, gate, 0) == EINVAL
