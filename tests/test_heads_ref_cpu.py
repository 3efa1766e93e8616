"""CPU: tests/_heads_ref.py (the float64 references of the DMOL and Gaussian-head kernels) is pinned, and the inputs of
tests/test_gpu_dmol_kernels.py / tests/test_gpu_gauss_heads.py are shown to be fair: a float32 evaluation of the stable
formulation stays inside the project's bounds on every one of them (so a miss on the GPU is the kernel's), the tail
sweep tells the stable formulation from the plain difference of two sigmoids, and no input sits on the likelihood's
discontinuity at MASS_SWITCH.

Measured here (torch CPU, float32): the stable form's per-pixel log-likelihood is at most 0.14 of its bound
(1e-4 |want| + 2.3e-5; the edge-bin cases, through the absolute term) and 0.003 of it elsewhere; the plain form on the
tail sweep reaches 5.7 times the bound on the upper tail and 0.05 of it on the lower."""

import math

import pytest
import torch

import _heads_ref as href
import _util
from oracle import dmol as odmol
from oracle import ops as oops

FAMILIES = href.dmol_families()


# ---------------------------------------------------------------------------------------------
# DMOL
def test_reference_is_the_oracle_in_float64():
    """dmol_ref is oracle.dmol.dmol_log_likelihood on the upcast inputs, in the kernel's layout as well as row by row,
    and its gradient is the oracle loss's."""
    rows, x, K, _ = FAMILIES["mix3"]
    ll, g = href.dmol_ref(rows, x, K)
    assert ll.dtype == torch.float64 and g.shape == rows.shape
    for N in (1, 3):
        l, xx = href.to_kernel_layout(rows[:9], x[:9], N)
        leaf = l.double().unsqueeze(2).requires_grad_(True)           # (N, 10 K, 1, L)
        want = odmol.dmol_log_likelihood(leaf, xx.double().unsqueeze(2), K).detach()
        assert float((want.reshape(-1) - ll[:9]).abs().max()) <= 1e-12 * float(ll[:9].abs().max())
        odmol.dmol_loss_sum_mean(leaf, xx.double().unsqueeze(2), K).backward()
        got = href.from_kernel_layout(leaf.grad.squeeze(2)) * N        # the loss is a mean over the batch
        assert float((got - g[:9]).abs().max()) <= 1e-12 * float(g[:9].abs().max())


def test_plain_and_stable_forms_agree_in_float64():
    """The identity sigmoid(a) - sigmoid(b) = sigmoid(a) sigmoid(-b) (1 - exp(-(a - b))): in float64 the two forms are
    the same function on every input (both far from their float64 rounding)."""
    for name, (rows, x, K, _) in FAMILIES.items():
        a, ga = href.dmol_ref(rows, x, K, "stable")
        b, gb = href.dmol_ref(rows, x, K, "plain")
        assert float(((a - b).abs() / a.abs().clamp_min(1.0)).max()) <= 1e-9, name
        assert float((ga - gb).abs().max() / ga.abs().max()) <= 1e-9, name


@pytest.mark.parametrize("name", list(FAMILIES))
def test_fp32_stable_form_within_bounds(name):
    """The GPU tier's bounds hold for a correct float32 evaluation of the stable formulation, on the inputs and on
    their mirror images."""
    rows, x, K, _ = FAMILIES[name]
    rep = _util.GradReport(f"fp32 stable dmol {name}")
    for tag, (r, xx) in (("", (rows, x)), (" mirrored", href.mirror(rows, x, K))):
        want, gwant = href.dmol_ref(r, xx, K)
        got, ggot = href.dmol_ref(r, xx, K, "stable", torch.float32)
        href.assert_ll(got, want, f"fp32 stable {name}{tag}")
        href.add_rows(rep, f"{name}{tag}", ggot, gwant)
    rep.finish()


def test_mirror_is_exact_in_float64():
    """Exact up to the oracle's own float64 rounding — and torch's softplus, which returns z itself beyond z = 20 and so
    drops log1p(e^-20) = 2e-9 on one side of a mirrored pair in the density fallback: 1e-8 covers it. (For the same reason
    the gradient of a value-0 bin saturated at +60 scales is exactly 0 in this reference and e^-60 for its mirror image,
    the value-255 bin: the gradients are compared at the family's scale, and the GPU tier gives each side its own
    reference.)"""
    for name, (rows, x, K, _) in FAMILIES.items():
        ll, g = href.dmol_ref(rows, x, K)
        llm, gm = href.dmol_ref(*href.mirror(rows, x, K), K)
        assert float(((ll - llm).abs() / ll.abs().clamp_min(1.0)).max()) <= 1e-8, name
        assert float((g - gm * href.mean_sign(K)).abs().max() / g.abs().max()) <= 1e-8, name


def test_tail_sweep_discriminates_the_two_forms():
    """On the tail sweep the PLAIN difference of sigmoids, in float32, misses the 1e-4 bound on upper-tail points (among
    them the four named ones) and on no lower-tail point; the stable form passes on both (test above)."""
    rows, x, K, labels = FAMILIES["tail"]
    want = href.dmol_ll(rows, x, K)
    got = href.dmol_ll(rows, x, K, "plain", torch.float32)
    ratio = (got.double() - want).abs() / (href.LL_TOL * want.abs() + href.LL_ABS)
    upper = torch.tensor([lab[2] > 0 for lab in labels])
    grid = {(lab[0], lab[1]): i for i, lab in enumerate(labels) if lab[2] > 0 and not isinstance(lab[1], tuple)}
    print(f"[heads] plain fp32 on the tail sweep: upper tail worst {float(ratio[upper].max()):.2f} x bound, "
          f"lower tail worst {float(ratio[~upper].max()):.3f} x bound")
    assert float(ratio[~upper].max()) <= 1.0, "a lower-tail point misses the bound: the inputs are not fair"
    assert float(ratio[upper].max()) > 1.0, "no upper-tail point tells the two forms apart"
    named = [(math.log(0.01), 10.0), (math.log(0.01), 11.0), (-6.0, 12.0), (-6.0, 13.0)]
    assert sum(float(ratio[grid[p]]) > 1.0 for p in named) >= 2, [float(ratio[grid[p]]) for p in named]


def test_no_input_sits_on_the_discontinuity():
    """No float64 bin mass within [0.9e-5, 1.1e-5] and no log-scale of exactly -7.0 — asserted on every input, none
    filtered. The tail sweep's grid is fixed and ONE of its points, (log-scale -6, t = 13), has mass 1.053e-5: it is
    the only input in the band (asserted), and for it the float32 mass of BOTH forms is shown to lie on the float64
    side of the switch with 4 % to spare, which is what the band is for."""
    lo, hi = href.BAND
    for name, (rows, x, K, labels) in FAMILIES.items():
        for i in range(rows.shape[0]):
            assert not bool((rows[i, href.scale_channels(K)] == odmol.LOG_SCALE_MIN).any()), (name, labels[i])
            mass = href.bin_masses(rows[i:i + 1], x[i:i + 1], K)
            inside = bool(((mass >= lo) & (mass <= hi)).any())
            on_grid_point = name == "tail" and labels[i][:2] == href.BAND_GRID_POINT
            assert inside == on_grid_point, (name, labels[i], mass.tolist())
            if on_grid_point:
                assert float(mass.min()) >= 1.04e-5 and float(mass.max()) <= 1.06e-5
                r32 = rows[i:i + 1]
                l, xx = href._as_images(r32, x[i:i + 1], torch.float32)
                _, means, log_scales, coeffs = odmol.split_params(l, K)
                for clp in (odmol.component_log_probs, href.component_log_probs_plain):
                    m32 = clp(xx, means, log_scales, coeffs).exp()
                    assert float(m32.min()) > 1.04e-5 and float(m32.max()) < 1.06e-5


def test_index_pools_are_the_vetted_rows():
    for K in (1, 3):
        rows, x = href.index_pool(K)
        assert rows.shape[1] == 10 * K and rows.shape[0] == x.shape[0] >= 9
    n, L = href.GRID_STRIDE_NL
    assert n * L > 4096 * 256 and n * L < 4096 * 256 + 64
    idx = href.index_pick(1000, rows.shape[0])
    assert int(idx.min()) >= 0 and int(idx.max()) < rows.shape[0] and len(set(idx.tolist())) == rows.shape[0]


# ---------------------------------------------------------------------------------------------
# Gaussian heads
@pytest.mark.parametrize("extra", href.GAUSS_EXTRA)
def test_gauss_head_formulas_equal_the_oracle(extra):
    C, L, N = 3, 7, 2
    q, p, eps, dz, dkl = href.gauss_inputs(C, L, N, extra, extra, "moderate")
    qd, pd, ed = q.double(), p.double(), eps.double()
    z0, kl0 = href.gauss_head(q, None, eps, C, 0)
    z1, kl1 = href.gauss_head(q, p, eps, C, 1)
    z2, kl2 = href.gauss_head(None, p, eps, C, 2)
    want_z = oops.sample_from_gaussian(qd[:, :C], qd[:, C:2 * C], ed)
    assert float((z0 - want_z).abs().max()) <= 1e-14 and torch.equal(z0, z1)
    assert float((z2 - oops.sample_from_gaussian(pd[:, :C], pd[:, C:2 * C], ed)).abs().max()) <= 1e-14 and kl2 is None
    want0 = oops.unit_gaussian_kl_div(qd[:, :C], qd[:, C:2 * C]).sum(dim=(1, 2))
    want1 = oops.gaussian_kl_div(qd[:, :C], qd[:, C:2 * C], pd[:, :C], pd[:, C:2 * C]).sum(dim=(1, 2))
    assert float((kl0 - want0).abs().max()) <= 1e-13 * float(want0.abs().max())
    assert float((kl1 - want1).abs().max()) <= 1e-13 * float(want1.abs().max())
    # gradients: zero where an argument is absent, and those of the oracle's expression where present
    _, _, dq, dp = href.gauss_head_ref(q, p, eps, C, 1, dz, dkl)
    ql, pl = qd[:, :2 * C].clone().requires_grad_(True), pd[:, :2 * C].clone().requires_grad_(True)
    obj = (oops.sample_from_gaussian(ql[:, :C], ql[:, C:], ed) * dz.double()).sum() + (
        oops.gaussian_kl_div(ql[:, :C], ql[:, C:], pl[:, :C], pl[:, C:]).sum(dim=(1, 2)) * dkl.double()).sum()
    wq, wp = torch.autograd.grad(obj, (ql, pl))
    assert float((dq - wq).abs().max()) <= 1e-13 * float(wq.abs().max())
    assert float((dp - wp).abs().max()) <= 1e-13 * float(wp.abs().max())
    _, _, dq, dp = href.gauss_head_ref(None, p, eps, C, 2, dz, None)
    assert dq is None and torch.equal(dp[:, :C], dz.double())
    _, _, dq, _ = href.gauss_head_ref(q, None, eps, C, 0, None, None)
    assert float(dq.abs().max()) == 0.0


def _gauss_fp32_check(rep, what, q, p, eps, C, mode, dz, dkl):
    want = href.gauss_head_ref(q, p, eps, C, mode, dz, dkl)
    got = href.gauss_head_ref(q, p, eps, C, mode, dz, dkl, dtype=torch.float32)
    for name, g, w in zip(("z", "kl", "dq", "dp"), got, want):
        assert (g is None) == (w is None)
        if g is None:
            continue
        assert bool(torch.isfinite(g).all()), f"{what} {name}"
        _util.assert_close(g, w, 1e-5, f"{what} {name}")
        rep.add(f"{what} {name}", g, w)


@pytest.mark.parametrize("regime", ["moderate", "wide"])
@pytest.mark.parametrize("cl", list(href.GAUSS_CL))
def test_fp32_gauss_heads_within_bounds(cl, regime):
    C, L = href.GAUSS_CL[cl]
    rep = _util.GradReport(f"fp32 gauss heads C*L={cl} {regime}")
    for N in href.GAUSS_N:
        for q_extra, p_extra in ((0, 5), (5, 0)):          # the two layouts of the GPU tier (other seeds, other values)
            q, p, eps, dz, dkl = href.gauss_inputs(C, L, N, q_extra, p_extra, regime)
            for mode in (0, 1, 2):
                _gauss_fp32_check(rep, f"N={N} q+{q_extra} mode={mode}", q, p, eps, C, mode, dz, dkl)
                _gauss_fp32_check(rep, f"N={N} q+{q_extra} mode={mode} dz alone", q, p, eps, C, mode, dz, None)
    rep.finish()


def test_fp32_gauss_pairs_within_bounds():
    q, p, eps, dz, dkl = href.gauss_pair_inputs()
    rep = _util.GradReport("fp32 gauss pairs")
    for mode in (0, 1, 2):
        _gauss_fp32_check(rep, f"mode={mode}", q, p, eps, 1, mode, dz, dkl)
    rep.finish()


def test_fp32_vec_mean_within_bounds():
    for n in href.VEC_MEAN_N:
        v = href.vec_mean_inputs(n)
        _util.assert_close(v.mean(), v.double().mean(), 1e-5, f"mean n={n}")
