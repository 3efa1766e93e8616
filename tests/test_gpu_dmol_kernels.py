"""GPU: the discretized mixture-of-logistics kernels (csrc/dmol.hip: pg_dmol_fwd, pg_dmol_bwd), called through the
C-ABI as ops/losses.py calls them, against the float64 reference of tests/_heads_ref.py (oracle/dmol.py in float64;
tests/test_heads_ref_cpu.py shows that a float32 evaluation of these very inputs stays inside the bounds used here).

Bounds are the project's and are not tuned to the kernel: the per-pixel log-likelihood at 1e-4 relative (the TOL of
tests/test_gpu_f4.py; absolute term 2.3e-5, see _heads_ref.LL_ABS), gradients under _util.GradReport's defaults with
every pixel's 10 K gradient as a tensor of its own; everything stated as zero, untouched or exactly linear is
torch.equal. A per-pixel loss is read with one forward launch per pixel (N = 1, L = 1 on the pixel's own 10 K floats).

Measured on the MI355X: with the interior mass as sigmoid(pin) - sigmoid(nin), as subpixel() had it, the tail sweep's
worst per-pixel relative loss error was 5.7e-4 on the upper tail and 5.4e-6 on the lower, and 29 tests of this file
failed; with the stable form 8.1e-7 on both, gradient rows at most 4.2e-5 max-norm and 0.40 element-wise
(profiles/README.md)."""

import pytest
import torch

import _heads_ref as href
import _util

pytestmark = pytest.mark.gpu

PG_ESHAPE = -2


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need the MI355X"
    from pytorch_generative_amd import _lib

    _lib.load()  # fail loudly if the extension is missing
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def families():
    """name -> (rows, x, K, labels, ll64, grad64): the float64 reference once for all tests."""
    out = {}
    for name, (rows, x, K, labels) in href.dmol_families().items():
        out[name] = (rows, x, K, labels) + href.dmol_ref(rows, x, K)
    return out


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _fwd(l, x, loss, N, K, L):
    from pytorch_generative_amd import _lib

    assert l.is_contiguous() and x.is_contiguous() and l.numel() == N * 10 * K * L and x.numel() == N * 3 * L
    return _lib.load().pg_dmol_fwd(l.data_ptr(), x.data_ptr(), loss.data_ptr(), N, K, L, _stream())


def _bwd(l, x, gscale, dl_ptr, N, K, L):
    from pytorch_generative_amd import _lib

    assert l.is_contiguous() and x.is_contiguous() and l.numel() == N * 10 * K * L and x.numel() == N * 3 * L
    return _lib.load().pg_dmol_bwd(l.data_ptr(), x.data_ptr(), gscale.data_ptr(), dl_ptr, N, K, L, _stream())


def _per_pixel(dev, rows, x, K):
    """-> (ll (P,), grad (P, 10 K)) from the kernels: one forward launch per row (its 10 K floats ARE the (1, 10 K, 1)
    tensor), one backward launch over all rows in the kernel's layout with N = 1 and gscale = 1."""
    from pytorch_generative_amd import _lib

    P = rows.shape[0]
    rows_d, x_d = rows.to(dev).contiguous(), x.to(dev).contiguous()
    loss = torch.zeros(P, device=dev)
    lib, st = _lib.load(), _stream()
    for i in range(P):
        rc = lib.pg_dmol_fwd(rows_d.data_ptr() + 4 * 10 * K * i, x_d.data_ptr() + 4 * 3 * i, loss.data_ptr() + 4 * i,
                             1, K, 1, st)
        _lib.check(rc, "pg_dmol_fwd")
    l, xx = href.to_kernel_layout(rows, x, 1)
    l_d, xx_d = l.to(dev), xx.to(dev)
    dl = torch.full_like(l_d, float("nan"))
    _lib.check(_bwd(l_d, xx_d, torch.ones(1, device=dev), dl.data_ptr(), 1, K, P), "pg_dmol_bwd")
    return -loss.cpu(), href.from_kernel_layout(dl.cpu())


def _check(rep, what, got_ll, got_g, want_ll, want_g):
    href.assert_ll(got_ll, want_ll, what)
    href.add_rows(rep, what, got_g, want_g)


def test_tail_sweep(dev, families):
    """K = 1, interior pixel, log-scales from 0.5 to below the clamp, 0 to 60 scales above and below the mean (and a
    different distance per sub-pixel): per-pixel loss and gradient against float64. The upper tail — both sigmoids
    near 1 — is where a difference of sigmoids loses its digits; its points must meet the bounds of their mirrors."""
    rows, x, K, labels, ll, g = families["tail"]
    got_ll, got_g = _per_pixel(dev, rows, x, K)
    upper = torch.tensor([lab[2] > 0 for lab in labels])
    for name, sel in (("upper tail", upper), ("lower tail", ~upper)):
        ratio, rel = href.ll_excess(got_ll[sel], ll[sel])
        print(f"[heads] tail sweep, {name}: worst ll ratio {ratio:.3e}, worst relative {rel:.3e}")
    rep = _util.GradReport("dmol tail sweep")
    _check(rep, "tail", got_ll, got_g, ll, g)
    rep.finish()
    below = torch.tensor([lab[0] < -7.0 for lab in labels])
    sc = href.scale_channels(K)
    assert torch.equal(got_g[below][:, sc], torch.zeros(int(below.sum()), len(sc))), "gradient of a clamped log-scale"
    assert bool((got_g[~below][:, sc] != 0).all())


@pytest.mark.parametrize("name", ["tail", "branch"] + [f"mix{K}" for K in href.MIXTURE_KS])
def test_mirror_symmetry(dev, families, name):
    """x -> -x, means -> -means: the same loss per pixel; the mean gradients change sign, the others do not. The values
    0 and 255 swap, so the two edge-bin branches do. Each side is held to its own float64 reference (the two references
    are mirror images, tests/test_heads_ref_cpu.py), and the two losses the kernel gives to each other."""
    rows, x, K, _, ll, g = families[name]
    mrows, mx = href.mirror(rows, x, K)
    mll, mg = href.dmol_ref(mrows, mx, K)
    got_ll, got_g = _per_pixel(dev, rows, x, K)
    got_mll, got_mg = _per_pixel(dev, mrows, mx, K)
    rep = _util.GradReport(f"dmol mirror {name}")
    _check(rep, f"{name}", got_ll, got_g, ll, g)
    _check(rep, f"{name} mirrored", got_mll, got_mg, mll, mg)
    href.assert_ll(got_mll, got_ll.double(), f"{name}: the kernel's mirrored loss against its own")
    rep.finish()


def test_every_branch(dev, families):
    """Both edge bins with arguments around +-60 and +-100 (finite, and equal to float64), values 1 and 254 (interior),
    the density fallback on both tails, log-scales on either side of the clamp (gradient exactly 0 below it), raw
    coefficients at +-8 with x_r = +-1."""
    rows, x, K, labels, ll, g = families["branch"]
    got_ll, got_g = _per_pixel(dev, rows, x, K)
    assert bool(torch.isfinite(got_ll).all()) and bool(torch.isfinite(got_g).all())
    rep = _util.GradReport("dmol branches")
    _check(rep, "branch", got_ll, got_g, ll, g)
    rep.finish()
    sc = torch.tensor(href.scale_channels(K))
    clamped = rows[:, sc] < -7.0
    assert int(clamped.sum()) >= 10
    assert torch.equal(got_g[:, sc][clamped], torch.zeros(int(clamped.sum()))), "gradient of a clamped log-scale"
    assert bool((g[:, sc][clamped] == 0).all())


@pytest.mark.parametrize("K", href.MIXTURE_KS)
def test_mixtures(dev, families, K):
    """Random mixtures, logits spread by +-60, one component at -1e4, every component at a joint log-probability of
    about -200, one exact component among negligible ones."""
    rows, x, _, labels, ll, g = families[f"mix{K}"]
    far = labels.index("all components at -200")
    assert -215.0 < float(ll[far]) < -185.0
    got_ll, got_g = _per_pixel(dev, rows, x, K)
    rep = _util.GradReport(f"dmol mixtures K={K}")
    _check(rep, f"mix{K}", got_ll, got_g, ll, g)
    rep.finish()


@pytest.mark.parametrize("K", [0, 17])
def test_component_count_outside_1_to_16_is_a_shape_error(dev, K):
    """The host check answers before any launch: status PG_ESHAPE, loss and dl untouched."""
    l = torch.zeros(1, 170, 4, device=dev)
    x = torch.zeros(1, 3, 4, device=dev)
    loss = torch.full((1,), 3.25, device=dev)
    dl = torch.full_like(l, href.SENTINEL)
    from pytorch_generative_amd import _lib

    lib = _lib.load()
    assert lib.pg_dmol_fwd(l.data_ptr(), x.data_ptr(), loss.data_ptr(), 1, K, 4, _stream()) == PG_ESHAPE
    assert lib.pg_dmol_bwd(l.data_ptr(), x.data_ptr(), loss.data_ptr(), dl.data_ptr(), 1, K, 4, _stream()) == PG_ESHAPE
    with pytest.raises(ValueError):
        _lib.check(PG_ESHAPE, "pg_dmol_fwd")
    torch.cuda.synchronize()
    assert float(loss) == 3.25 and torch.equal(dl.cpu(), torch.full((1, 170, 4), href.SENTINEL))


PAD = 300  # floats of sentinel on either side of dl


def _index_case(dev, K, N, L, loss0, gscale):
    """Pixels drawn from the vetted pool; -> (got loss, want loss, got dl rows, want rows, pads ok, all written)."""
    from pytorch_generative_amd import _lib

    pool_rows, pool_x = href.index_pool(K)
    pll, pg = href.dmol_ref(pool_rows, pool_x, K)
    idx = href.index_pick(N * L, pool_rows.shape[0], salt=K + N + L)
    l, x = href.to_kernel_layout(pool_rows[idx], pool_x[idx], N)
    l_d, x_d = l.to(dev), x.to(dev)
    loss = torch.full((1,), loss0, device=dev)
    _lib.check(_fwd(l_d, x_d, loss, N, K, L), "pg_dmol_fwd")
    buf = torch.full((l.numel() + 2 * PAD,), float("nan"), device=dev)
    buf[:PAD] = href.SENTINEL
    buf[-PAD:] = href.SENTINEL
    gs = torch.full((1,), gscale, device=dev)
    _lib.check(_bwd(l_d, x_d, gs, buf.data_ptr() + 4 * PAD, N, K, L), "pg_dmol_bwd")
    buf = buf.cpu()
    pads_ok = torch.equal(buf[:PAD], torch.full((PAD,), href.SENTINEL)) and torch.equal(buf[-PAD:], buf[:PAD])
    dl = buf[PAD:-PAD].reshape(N, 10 * K, L)
    want_loss = loss0 - float(pll[idx].sum()) / N
    return float(loss), want_loss, dl, pg, idx, pads_ok


@pytest.mark.parametrize("N", href.INDEX_N)
@pytest.mark.parametrize("L", href.INDEX_L)
@pytest.mark.parametrize("K", [1, 3])
def test_indexing(dev, K, N, L):
    """Row lengths on either side of a wave and of a block, one and three samples: the loss is ADDED to what loss[0]
    held, every element of dl is written (it starts as NaN) and nothing outside it (sentinels on both sides), and the
    gradient carries gscale / N — gscale read from device memory."""
    gscale = -2.5
    got, want, dl, pg, idx, pads_ok = _index_case(dev, K, N, L, 3.25, gscale)
    assert pads_ok, "pg_dmol_bwd wrote outside dl"
    assert bool(torch.isfinite(dl).all()), "an element of dl was not written"
    assert abs(got - want) <= 1e-4 * abs(want), f"loss {got} != {want}"
    rep = _util.GradReport(f"dmol indexing K={K} N={N} L={L}")
    href.add_rows(rep, "dl", href.from_kernel_layout(dl), pg[idx] * (gscale / N))
    rep.finish()


def test_gradient_is_linear_in_gscale(dev):
    """gscale = 4 gives exactly 4 x the gradient of gscale = 1 (a power of two: no rounding), and -1 its negative."""
    K, N, L = 3, 3, 65
    runs = [_index_case(dev, K, N, L, 0.0, gs)[2] for gs in (1.0, 4.0, -1.0)]
    assert torch.equal(runs[1], 4.0 * runs[0]) and torch.equal(runs[2], -runs[0])
    assert float(runs[0].abs().max()) > 0


def test_grid_stride_loops(dev):
    """N * L = 1048581 pixels, just above 4096 * 256: the forward (2048 blocks at most) and the backward (4096) both go
    round their grid-stride loop; K = 1, pixels from the tail sweep and the branch cases."""
    N, L = href.GRID_STRIDE_NL
    got, want, dl, pg, idx, pads_ok = _index_case(dev, 1, N, L, 0.0, 1.0)
    assert pads_ok, "pg_dmol_bwd wrote outside dl"
    assert bool(torch.isfinite(dl).all()), "an element of dl was not written"
    assert abs(got - want) <= 1e-4 * abs(want), f"loss {got} != {want}"
    rep = _util.GradReport("dmol grid stride")
    href.add_rows(rep, "dl", href.from_kernel_layout(dl), pg[idx] / N)
    rep.finish()
