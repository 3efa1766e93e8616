"""GPU: the Gaussian-head kernels and the two small kernels of the ELBO (csrc/vae_ops.hip: pg_gauss_head_fwd,
pg_gauss_head_bwd, pg_vec_mean_accum, pg_fill_scaled), called through the C-ABI as ops/vae.py and ops/losses.py call
them, against the float64 reference of tests/_heads_ref.py (pinned against oracle/ops.py by
tests/test_heads_ref_cpu.py, which also shows that a float32 evaluation of these inputs stays inside the bounds).

Bounds: _util.assert_close at 1e-5 and _util.GradReport's defaults, as tests/test_gpu_models.py uses for these kernels;
everything stated as untouched, zero, or equal between two runs is torch.equal. Shapes: one element to 40000 per
sample — one wave, one block, 64 blocks exactly, and beyond (the grid-stride loop) — with one and three samples, batch
strides wider than [mean | log_std] on either argument, all three modes, every NULL the C-ABI allows."""

import pytest
import torch

import _heads_ref as href
import _util

pytestmark = pytest.mark.gpu

TOL = 1e-5
S = href.SENTINEL


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need the MI355X"
    from pytorch_generative_amd import _lib

    _lib.load()  # fail loudly if the extension is missing
    return torch.device("cuda:0")


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _ptr(t):
    return None if t is None else t.data_ptr()


def _fwd(q, p, eps, z, kl, C, mode):
    from pytorch_generative_amd import _lib

    N, _, L = eps.shape
    assert all(t is None or t.is_contiguous() for t in (q, p, eps, z, kl))
    _lib.check(_lib.load().pg_gauss_head_fwd(_ptr(q), _ptr(p), eps.data_ptr(), z.data_ptr(), _ptr(kl), N, C, L,
                                             0 if q is None else q.shape[1] * L, 0 if p is None else p.shape[1] * L,
                                             mode, _stream()), "pg_gauss_head_fwd")


def _bwd(q, p, eps, dz, dkl, dq, dp, C, mode):
    from pytorch_generative_amd import _lib

    N, _, L = eps.shape
    assert all(t is None or t.is_contiguous() for t in (q, p, eps, dz, dkl, dq, dp))
    _lib.check(_lib.load().pg_gauss_head_bwd(_ptr(q), _ptr(p), eps.data_ptr(), _ptr(dz), _ptr(dkl), _ptr(dq), _ptr(dp),
                                             N, C, L, 0 if q is None else q.shape[1] * L,
                                             0 if p is None else p.shape[1] * L, mode, _stream()), "pg_gauss_head_bwd")


def _compare(rep, name, got, want):
    assert bool(torch.isfinite(got).all()), f"{name}: not finite"
    _util.assert_close(got, want, TOL, name)
    rep.add(name, got, want)


def _run_mode(dev, rep, what, q, p, eps, dz, dkl, C, mode, kl0=1.5):
    """Forward (kl accumulated onto kl0, z surrounded by nothing the kernel may touch) and the three backward argument
    paths — dz and dkl, dz alone, dkl alone — against the reference; the channels of dq / dp beyond 2 C stay sentinels."""
    N, _, L = eps.shape
    qd = None if mode == 2 else q.to(dev)
    pd = None if mode == 0 else p.to(dev)
    ed, dzd, dkld = eps.to(dev), dz.to(dev), dkl.to(dev)
    z = torch.full((N, C, L), S, device=dev)
    kl = torch.full((N + 2,), kl0, device=dev)          # kl[0] and kl[N + 1] are not the kernel's
    _fwd(qd, pd, ed, z, None if mode == 2 else kl[1:N + 1], C, mode)
    want_z, want_kl, _, _ = href.gauss_head_ref(q, p, eps, C, mode, None, None)
    _compare(rep, f"{what} z", z.cpu(), want_z)
    kl = kl.cpu()
    assert float(kl[0]) == kl0 and float(kl[N + 1]) == kl0, "kl written outside its N elements"
    if mode == 2:
        assert torch.equal(kl, torch.full((N + 2,), kl0))
        kl_probe = torch.full((N,), S, device=dev)       # a kl pointer is ignored in mode 2 (and q may be NULL)
        z2 = torch.empty_like(z)
        _fwd(None, pd, ed, z2, kl_probe, C, mode)
        assert torch.equal(kl_probe.cpu(), torch.full((N,), S)) and torch.equal(z2, z), "mode 2 touched kl"
    else:
        _compare(rep, f"{what} kl (+ {kl0})", kl[1:N + 1], want_kl + kl0)
    for path, use_dz, use_dkl in (("dz+dkl", True, True), ("dz", True, False), ("dkl", False, True)):
        if mode == 2 and not use_dz:
            continue                                       # nothing to propagate: dkl is ignored in mode 2
        dq = None if mode == 2 else torch.full_like(qd, S)
        dp = None if mode == 0 else torch.full_like(pd, S)
        _bwd(qd, pd, ed, dzd if use_dz else None, dkld if use_dkl else None, dq, dp, C, mode)
        _, _, want_dq, want_dp = href.gauss_head_ref(q, p, eps, C, mode, dz if use_dz else None,
                                                     dkl if use_dkl else None)
        for name, got, want in (("dq", dq, want_dq), ("dp", dp, want_dp)):
            if got is None:
                continue
            got = got.cpu()
            rest = got[:, 2 * C:]
            assert torch.equal(rest, torch.full_like(rest, S)), f"{what} {path}: {name} written beyond 2 C channels"
            if float(want.abs().max()) == 0.0:             # mode 1 without dkl: dp is exactly 0
                assert torch.equal(got[:, :2 * C], torch.zeros_like(got[:, :2 * C])), f"{what} {path}: {name} != 0"
            else:
                _compare(rep, f"{what} {path} {name}", got[:, :2 * C], want)


@pytest.mark.parametrize("regime", ["moderate", "wide"])
@pytest.mark.parametrize("N", href.GAUSS_N)
@pytest.mark.parametrize("cl", list(href.GAUSS_CL))
def test_gauss_heads_all_modes(dev, cl, N, regime):
    """Modes 0, 1, 2 at every size class, q and p each with and without extra channels (the wider one is the other
    argument in turn, so a kernel reading p with q's batch stride — or the reverse — lands on the wrong sample)."""
    C, L = href.GAUSS_CL[cl]
    rep = _util.GradReport(f"gauss heads C*L={cl} N={N} {regime}")
    for q_extra, p_extra in ((0, 5), (5, 0)):
        q, p, eps, dz, dkl = href.gauss_inputs(C, L, N, q_extra, p_extra, regime)
        for mode in (0, 1, 2):
            _run_mode(dev, rep, f"q+{q_extra} p+{p_extra} mode={mode}", q, p, eps, dz, dkl, C, mode)
    rep.finish()


def test_gauss_heads_extreme_pairs(dev):
    """Log-std pairs (s_q, s_p) at +-20 with means 60 apart, one element per sample: finite and equal to float64."""
    q, p, eps, dz, dkl = href.gauss_pair_inputs()
    rep = _util.GradReport("gauss heads +-20 pairs")
    for mode in (0, 1, 2):
        _run_mode(dev, rep, f"mode={mode}", q, p, eps, dz, dkl, 1, mode, kl0=0.0)
    rep.finish()


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("cl", [257, 16385, 40000])
def test_gauss_kl_is_bit_reproducible_in_deterministic_mode(dev, cl, mode):
    """Under pg_attn_fused_bwd(0) the forward reduces each sample's KL in ONE block: two runs are bit-equal, and agree
    with the default multi-block (atomic) path within the bound. z does not depend on the mode."""
    from pytorch_generative_amd import _lib

    lib = _lib.load()
    C, L = href.GAUSS_CL[cl]
    N = 3
    q, p, eps, _, _ = href.gauss_inputs(C, L, N, 0, 5, "moderate", seed=1)
    qd, pd, ed = q.to(dev), (p.to(dev) if mode else None), eps.to(dev)
    _, want_kl, _, _ = href.gauss_head_ref(q, p, eps, C, mode, None, None)

    def run():
        z, kl = torch.empty(N, C, L, device=dev), torch.zeros(N, device=dev)
        _fwd(qd, pd, ed, z, kl, C, mode)
        return z.cpu(), kl.cpu()

    previous = lib.pg_attn_fused_bwd(1)
    try:
        z_default, kl_default = run()
        lib.pg_attn_fused_bwd(0)
        assert lib.pg_attn_fused_bwd(-1) == 0
        (z_a, kl_a), (z_b, kl_b) = run(), run()
    finally:
        lib.pg_attn_fused_bwd(previous)
    assert lib.pg_attn_fused_bwd(-1) == previous
    assert torch.equal(kl_a, kl_b), "deterministic mode: two runs differ"
    assert torch.equal(z_a, z_default) and torch.equal(z_b, z_default)
    _util.assert_close(kl_a, want_kl, TOL, "deterministic kl")
    _util.assert_close(kl_default, want_kl, TOL, "default kl")
    _util.assert_close(kl_a, kl_default, TOL, "deterministic against default kl")


@pytest.mark.parametrize("n", href.VEC_MEAN_N)
def test_vec_mean_accum(dev, n):
    """out[0] += mean(v): on either side of the single wave's 64 lanes, onto a non-zero out, neighbours untouched."""
    from pytorch_generative_amd import _lib

    v = href.vec_mean_inputs(n)
    out = torch.tensor([S, 2.0, S], device=dev)
    vd = v.to(dev)
    _lib.check(_lib.load().pg_vec_mean_accum(vd.data_ptr(), n, out.data_ptr() + 4, _stream()), "pg_vec_mean_accum")
    out = out.cpu()
    assert float(out[0]) == float(torch.tensor(S)) and float(out[2]) == float(torch.tensor(S))
    _util.assert_close(out[1], 2.0 + v.double().mean(), TOL, f"mean n={n}")


@pytest.mark.parametrize("n", href.FILL_N)
def test_fill_scaled(dev, n):
    """out[i] = g[0] * scale for i < n — the single float32 product, bit for bit — and nothing after n."""
    from pytorch_generative_amd import _lib

    g = torch.tensor([-1.7], device=dev)
    scale = 1.0 / n
    out = torch.full((n + 64,), S, device=dev)
    _lib.check(_lib.load().pg_fill_scaled(g.data_ptr(), scale, out.data_ptr(), n, _stream()), "pg_fill_scaled")
    out = out.cpu()
    want = torch.tensor([-1.7]) * torch.tensor([scale], dtype=torch.float32)
    assert torch.equal(out[:n], want.expand(n)), "fill value"
    assert torch.equal(out[n:], torch.full((64,), S)), "written beyond n"
