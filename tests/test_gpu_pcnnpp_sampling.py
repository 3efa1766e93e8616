"""GPU: PixelCNN++'s row-cached incremental sampler — the row step against one full forward (teacher forcing, on the graph
path and with capture refused), ops.dmol_sample against its float64 restatement, the single-row column resampling, and the
properties of the sampling procedure."""

import pytest
import torch

import _dmol_sample_ref as dref
import _util

pytestmark = pytest.mark.gpu

TOL = 1e-5  # the tolerance of test_row_cached_sampling_equals_full_forward


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need the MI355X"
    from pytorch_generative_amd import _lib

    _lib.load()  # fail loudly if the extension is missing
    return torch.device("cuda:0")


def _pp():
    from pytorch_generative_amd.models.autoregressive import pixel_cnn_pp

    return pixel_cnn_pp


# ---- teacher forcing ------------------------------------------------------------------------------------------------------------
class _Teacher:
    """sample_fn that hands out the pixels of `x` in raster order (every pixel is evaluated under return_params)."""

    def __init__(self):
        self.x, self.calls, self.seen = None, 0, []

    def start(self, x):
        self.x, self.calls, self.seen = x, 0, []

    def __call__(self, params):
        w = self.x.shape[3]
        r, c = divmod(self.calls, w)
        self.calls += 1
        self.seen.append(tuple(params.shape))
        return self.x[:, :, r, c]


def _teacher_forcing(model, teacher, x, what):
    n, _, h, w = x.shape
    teacher.start(x)
    out, params = model.sample(conditioned_on=torch.full_like(x, -2.0), return_params=True)
    assert teacher.calls == h * w and set(teacher.seen) == {(n, params.shape[1])}
    assert torch.equal(out, x), f"{what}: the canvas is not the teacher's image"
    with torch.no_grad():
        full = model._net(x)
    _util.assert_close(params, full, TOL, f"{what}: row-cached parameters vs one full forward")
    return out, params


TEACHER_CASES = [dict(n_filters=16, n_resnet=1, n_mix=5, hw=(8, 8)), dict(n_filters=16, n_resnet=1, n_mix=5, hw=(8, 12)),
                 dict(n_filters=8, n_resnet=2, n_mix=2, hw=(12, 8))]


@pytest.mark.parametrize("cfg", TEACHER_CASES, ids=["8x8", "8x12", "12x8-2resnets"])
def test_teacher_forcing_equals_full_forward(dev, cfg, monkeypatch):
    """With the teacher's pixels in place of the draws, the parameters of every pixel from the row steps equal one full
    forward on the finished image — all three row classes, both strided levels, a non-square image — once with the row
    steps replayed from their hipGraphs (H W step and H commit replays) and once with capture refused, bit for bit."""
    h, w = cfg["hw"]
    teacher = _Teacher()
    torch.manual_seed(0)
    model = _pp().PixelCNNpp(in_channels=3, n_filters=cfg["n_filters"], n_resnet=cfg["n_resnet"], n_mix=cfg["n_mix"],
                             sample_fn=teacher).to(dev)
    x = (torch.rand(3, 3, h, w, generator=torch.Generator().manual_seed(5)) * 2.0 - 1.0).to(dev)
    replays = []
    real_replay = torch.cuda.CUDAGraph.replay
    monkeypatch.setattr(torch.cuda.CUDAGraph, "replay", lambda self: (replays.append(1), real_replay(self))[1])
    out_g, params_g = _teacher_forcing(model, teacher, x, "graph path")
    assert len(replays) == h * w + h, "the graph path did not replay once per pixel and once per row"

    refused = []

    class Refused:
        def __init__(self, *a, **k):
            refused.append(1)
            raise RuntimeError("graph capture refused")

    monkeypatch.setattr(torch.cuda, "CUDAGraph", Refused)
    out_e, params_e = _teacher_forcing(model, teacher, x, "eager path")
    assert refused == [1] and len(replays) == h * w + h, "the eager fallback was not taken"
    assert torch.equal(out_e, out_g) and torch.equal(params_e, params_g)


# ---- the draw kernel --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", sorted(dref.KERNEL_SEEDS))
def test_dmol_sample_matches_float64(dev, k):
    """ops.dmol_sample against the float64 restatement given the same uniforms, K in {1, 5, 10} and, for the lanes past 16
    of the argmax butterfly and the kernel's bound, 17 and 32; N in {1, 3, 64, 65} (one image, a partial group block,
    exactly eight blocks, one more), each position once by host arguments and once through pos_dev: draws
    outside the near-tie band agree to 1e-5 max-norm (values and terms are bounded, fp32 round-off stays below it), every
    value lies in [-1, 1], known entries and every other canvas position are bit-unchanged, the row buffer holds the
    pixel as the canvas does afterwards (only that column), and at most 1 % of the draws fall inside the band."""
    from pytorch_generative_amd import ops

    h, w = 4, 8
    total = excluded = 0
    worst = 0.0
    for n in dref.KERNEL_BATCHES:
        params, uniforms, canvas, unknown = dref.kernel_case(dref.KERNEL_SEEDS[k], n, k, h, w)
        if n == 3:  # the parameters through their strides: a column window of a wider, taller tensor
            big = torch.full((n, 10 * k, 2, w + 3), float("nan"))
            big[:, :, 1:, 2:2 + w] = params
            params_d = big.to(dev)[:, :, 1:, 2:2 + w]
            assert not params_d.is_contiguous()
        else:
            params_d = params.to(dev)
        uniforms_d, unknown_d = uniforms.to(dev), unknown.to(dev)
        pos_dev = torch.zeros(1, dtype=torch.int32, device=dev)
        for r, c in dref.KERNEL_POSITIONS:
            want, gap = dref.apply(params, uniforms, canvas, unknown, k, r, c)
            keep = gap >= dref.NEAR_TIE
            results = []
            for by_device in (False, True):
                got = canvas.to(dev)
                row_buf = torch.full((n, 3, 1, w), 5.0, device=dev)
                if by_device:
                    pos_dev.fill_(r * w + c)
                    ops.dmol_sample(params_d, uniforms_d, got, unknown_d, k, row_buf=row_buf, pos_dev=pos_dev)
                else:
                    ops.dmol_sample(params_d, uniforms_d, got, unknown_d, k, r, c, row_buf=row_buf)
                got_c, buf = got.cpu(), row_buf.cpu()
                results.append(got_c)
                assert float(got_c.min()) >= -1.0 and float(got_c.max()) <= 1.0
                untouched = ~unknown.clone()
                untouched[:, :, :r] = True
                untouched[:, :, r + 1:] = True
                untouched[:, :, r, :c] = True
                untouched[:, :, r, c + 1:] = True
                assert torch.equal(got_c[untouched], canvas[untouched]), "a known entry or another position changed"
                assert torch.equal(buf[:, :, 0, c], got_c[:, :, r, c]), "row buffer != canvas at the pixel"
                others = torch.ones(w, dtype=torch.bool)
                others[c] = False
                assert bool((buf[:, :, 0, others] == 5.0).all()), "the row buffer changed outside the pixel's column"
                err = (got_c[:, :, r, c].double() - want[:, :, r, c]).abs()[keep]
                if err.numel():
                    worst = max(worst, float(err.max()))
                total += n
                excluded += int((~keep).sum())
            assert torch.equal(results[0], results[1]), "host (r, c) != device pos_dev"
            # a draw without a row buffer leaves the same canvas
            bare = canvas.to(dev)
            ops.dmol_sample(params_d, uniforms_d, bare, unknown_d, k, r, c)
            assert torch.equal(bare.cpu(), results[0])
    print(f"dmol_sample K={k}: worst |fp32 - fp64| {worst:.3e} over {total - excluded} draws, {excluded} inside the near-tie band")
    assert excluded <= 0.01 * total, (excluded, total)
    assert worst <= 1e-5, f"K={k}: max-norm error {worst:.3e} > 1e-5"


def test_dmol_sample_rejects_what_it_does_not_take(dev):
    from pytorch_generative_amd import ops

    params, uniforms, canvas, unknown = (t.to(dev) for t in dref.kernel_case(1, 2, 5))
    with pytest.raises(ValueError):
        ops.dmol_sample(params, uniforms[:-1], canvas, unknown, 5)
    with pytest.raises(ValueError):
        ops.dmol_sample(params, uniforms, canvas, unknown, 5, 4, 0)  # a row outside the image
    with pytest.raises(ValueError):
        ops.dmol_sample(params, uniforms, canvas, unknown, 4)
    with pytest.raises(TypeError):
        ops.dmol_sample(params, uniforms, canvas, unknown.float(), 5)
    with pytest.raises(RuntimeError):
        ops.dmol_sample(params.cpu(), uniforms, canvas, unknown, 5)


# ---- column resampling ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w", [4, 12, 32])
def test_column_resampling_of_one_row(dev, w):
    from pytorch_generative_amd import ops

    x = torch.randn(3, 5, 1, w, generator=torch.Generator().manual_seed(w)).to(dev)
    assert torch.equal(ops.col_subsample2(x), x[..., ::2])
    stuffed = torch.zeros(3, 5, 1, 2 * w, device=dev)
    stuffed[..., ::2] = x
    up = ops.col_zero_insert2(x)
    assert torch.equal(up, stuffed) and not bool(torch.signbit(up[..., 1::2]).any())
    assert torch.equal(ops.col_subsample2(up), x)
    with pytest.raises(RuntimeError):
        ops.col_subsample2(x.clone().requires_grad_(True))


# ---- the procedure ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small_model(dev):
    torch.manual_seed(0)
    return _pp().PixelCNNpp(in_channels=3, n_filters=16, n_resnet=1, n_mix=5).to(dev)


@pytest.fixture(scope="module")
def seeded_sample(small_model):
    torch.manual_seed(11)
    return small_model.sample(n_samples=2, image_size=(8, 8))


def test_sampler_is_reproducible_and_in_range(small_model, seeded_sample):
    a = seeded_sample
    assert a.shape == (2, 3, 8, 8) and float(a.min()) >= -1.0 and float(a.max()) <= 1.0
    assert float(a.std()) > 0.0
    torch.manual_seed(11)
    assert torch.equal(small_model.sample(n_samples=2, image_size=(8, 8)), a)
    torch.manual_seed(12)
    assert not torch.equal(small_model.sample(n_samples=2, image_size=(8, 8)), a)


def test_sampler_keeps_what_is_given(dev, small_model, seeded_sample):
    a = seeded_sample
    cond = torch.full((2, 3, 8, 8), -2.0, device=dev)
    cond[:, :, :4] = a[:, :, :4]  # the upper half given
    before = cond.clone()
    torch.manual_seed(5)
    c = small_model.sample(conditioned_on=cond)
    assert torch.equal(cond, before), "conditioned_on was modified"
    assert torch.equal(c[:, :, :4], a[:, :, :4])
    assert float(c[:, :, 4:].min()) >= -1.0 and float(c[:, :, 4:].max()) <= 1.0
    assert torch.equal(small_model.sample(conditioned_on=a), a), "a fully known image did not come back unchanged"
    # single known entries inside unknown pixels, and an image of the batch that is fully known
    mixed = torch.full((2, 3, 8, 8), -2.0, device=dev)
    mixed[0] = a[0]
    mixed[1, 1, 2, 3] = 0.25
    torch.manual_seed(5)
    d = small_model.sample(conditioned_on=mixed)
    assert torch.equal(d[0], a[0]) and float(d[1, 1, 2, 3]) == 0.25 and float(d.min()) >= -1.0


def test_same_uniforms_same_draw_as_the_float64_restatement(dev, small_model):
    """The draws of a whole call follow its parameters: with return_params, every pixel equals the float64 restatement's
    draw from the returned parameters and the call's own uniforms (the one torch.rand the seed fixes)."""
    n, k, h, w = 2, 5, 8, 8
    torch.manual_seed(21)
    out, params = small_model.sample(n_samples=n, image_size=(h, w), return_params=True)
    torch.manual_seed(21)
    uniforms = torch.rand((h * w, n, k + 3), device=dev).cpu()
    out, params = out.cpu(), params.cpu()
    worst, skipped = 0.0, 0
    for r in range(h):
        for c in range(w):
            u = uniforms[r * w + c]
            want, gap = dref.draw(params[:, :, r, c], u[:, :k], u[:, k:], k)
            keep = gap >= dref.NEAR_TIE
            skipped += int((~keep).sum())
            if bool(keep.any()):
                worst = max(worst, float((out[:, :, r, c].double() - want)[keep].abs().max()))
    assert skipped <= 1 and worst <= 1e-5, (skipped, worst)


def test_unit_range_model_follows_the_plain_one(dev, small_model, seeded_sample):
    unit = _pp().PixelCNNppUnitRange(in_channels=3, n_filters=16, n_resnet=1, n_mix=5).to(dev)
    unit.load_state_dict(small_model.state_dict())
    torch.manual_seed(11)
    b = unit.sample(n_samples=2, image_size=(8, 8))
    assert float(b.min()) >= 0.0 and float(b.max()) <= 1.0
    assert torch.equal(b, (seeded_sample + 1.0) * 0.5)
    torch.manual_seed(11)
    b2, params = unit.sample(n_samples=2, image_size=(8, 8), return_params=True)
    assert torch.equal(b2, b) and params.shape == (2, 50, 8, 8)
    with pytest.raises(ValueError):
        unit.sample(n_samples=2, image_size=(8, 8), incremental=False, return_params=True)


def test_full_forward_procedure_is_still_there(dev, small_model):
    torch.manual_seed(3)
    a = small_model.sample(n_samples=1, image_size=(4, 4), incremental=False)
    torch.manual_seed(3)
    b = small_model.sample(n_samples=1, image_size=(4, 4), incremental=False)
    assert torch.equal(a, b) and a.shape == (1, 3, 4, 4) and float(a.min()) >= -1.0 and float(a.max()) <= 1.0


def test_nothing_leaks_from_one_call_into_the_next(dev):
    """Bands, constants and the draw's static buffers (uniforms, row buffer, position) belong to one call: a sample at
    8 x 8 and one at 8 x 12 with another batch size, both drawn by ops.dmol_sample, then teacher forcing at 8 x 8 on the
    same model still equals the full forward."""
    teacher = _Teacher()
    torch.manual_seed(0)
    model = _pp().PixelCNNpp(in_channels=3, n_filters=16, n_resnet=1, n_mix=5, sample_fn=teacher).to(dev)
    model._pixel_sample_fn = None  # the first two calls draw from the mixture, as a model built without sample_fn does
    torch.manual_seed(1)
    a = model.sample(n_samples=2, image_size=(8, 8))
    b = model.sample(n_samples=3, image_size=(8, 12))
    assert teacher.calls == 0
    assert a.shape == (2, 3, 8, 8) and b.shape == (3, 3, 8, 12) and float(b.min()) >= -1.0 and float(b.max()) <= 1.0
    assert float(a.std()) > 0.0 and float(b.std()) > 0.0
    model._pixel_sample_fn = teacher
    x = (torch.rand(3, 3, 8, 8, generator=torch.Generator().manual_seed(9)) * 2.0 - 1.0).to(dev)
    _teacher_forcing(model, teacher, x, "after two other calls")
