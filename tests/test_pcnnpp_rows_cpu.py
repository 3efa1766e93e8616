"""CPU: the pieces of PixelCNN++'s row-cached sampler that need no GPU — the row schedule, the row-by-row restatement of the
network against the oracle's full forward (float64), the float64 restatement of the mixture draw against
PixelCNNpp.sample_from_mixture, the inputs of the GPU kernel test, and the new entry points' argument checks."""

import pytest
import torch

import _dmol_sample_ref as dref
import _pcnnpp_rows


def _pp():
    from pytorch_generative_amd.models.autoregressive import pixel_cnn_pp

    return pixel_cnn_pp


# ---- the schedule ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h", [4, 8, 12])
def test_row_schedule_follows_the_rule(h):
    sched = _pp().row_schedule(h)
    assert len(sched) == h
    for y, entry in enumerate(sched):
        assert [s for s, _ in entry] == [s for s in range(3) if y % 2 ** s == 0], (y, entry)
        assert all(r == y >> s for s, r in entry)
        assert entry[0] == (0, y), "level 0 is evaluated at every row, first"
    for s in range(3):  # every row of every level once, in order
        visited = [r for entry in sched for lvl, r in entry if lvl == s]
        assert visited == list(range(h >> s)), (s, visited)


@pytest.mark.parametrize("h", [0, -4, 2, 6, 9])
def test_row_schedule_rejects_heights_the_network_does_not_take(h):
    with pytest.raises(ValueError):
        _pp().row_schedule(h)


# ---- the network, row by row ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_resnet", [1, 2])
@pytest.mark.parametrize("hw", [(4, 4), (8, 8), (8, 12)])
def test_row_by_row_network_equals_full_forward(hw, n_resnet):
    """Every row's parameters from the banded row-by-row evaluation equal the oracle's full forward to 1e-12 (float64), the
    evaluate-only pass leaves no trace (it can be repeated), and only the commit pass moves the bands."""
    from oracle import pixelcnnpp as opp

    h, w = hw
    torch.manual_seed(0)
    model = _pp().PixelCNNpp(in_channels=3, n_filters=6, n_resnet=n_resnet, n_mix=2)
    g = torch.Generator().manual_seed(1)
    state = {k: (v.detach().double() + 0.05 * torch.randn(v.shape, generator=g, dtype=torch.float64))
             for k, v in model.state_dict().items()}  # random weights AND biases
    x = torch.rand(2, 3, h, w, generator=g, dtype=torch.float64) * 2.0 - 1.0
    want = opp.pixel_cnn_pp(state, x, n_resnet)
    net = _pcnnpp_rows.RowNet(state, n_resnet, h)
    for y in range(h):
        row = x[:, :, y:y + 1, :]
        garbage = row.clone()
        garbage[..., w // 2:] = 7.0  # an evaluate-only pass on an unfinished row must leave no trace
        net.row(y, garbage, commit=False)
        first = net.row(y, row, commit=False)
        again = net.row(y, row, commit=False)
        assert torch.equal(first, again)
        got = net.row(y, row, commit=True)
        assert torch.equal(got, first)
        err = float((got[:, :, 0] - want[:, :, y]).abs().max())
        assert err <= 1e-12, f"row {y}: {err:.3e}"


# ---- the draw --------------------------------------------------------------------------------------------------------------------
def _mixture_with_uniforms(params, u_mix, u_pix, k, monkeypatch):
    """PixelCNNpp.sample_from_mixture with torch.rand_like handing out the given uniforms (first the K, then the 3)."""
    queue = [u_mix.clone(), u_pix.clone()]
    monkeypatch.setattr(torch, "rand_like", lambda t, **kw: queue.pop(0).to(t.dtype))
    out = _pp().PixelCNNpp.sample_from_mixture(params, k)
    assert not queue
    return out


@pytest.mark.parametrize("k", [1, 5, 10])
def test_draw_restatement_equals_sample_from_mixture(k, monkeypatch):
    g = torch.Generator().manual_seed(k)
    n = 257
    params = torch.randn(n, 10 * k, generator=g, dtype=torch.float64) * 2.0
    params[:, 2 * k:3 * k] -= 6.0  # red log-scales around the floor
    u_mix = torch.rand(n, k, generator=g, dtype=torch.float64)
    u_pix = torch.rand(n, 3, generator=g, dtype=torch.float64)
    u_mix[0], u_pix[0] = 0.0, 1.0  # both clamps
    u_mix[1], u_pix[1] = 1.0, 0.0
    want = _mixture_with_uniforms(params, u_mix, u_pix, k, monkeypatch)
    got, gap = dref.draw(params, u_mix, u_pix, k)
    assert torch.equal(got, want)
    assert got.min() >= -1.0 and got.max() <= 1.0 and (gap >= 0).all()


def _one_component(mean, log_scale, coeff):
    """(1, 10) parameters of a single component: logits [0], then per sub-pixel mean, log-scale, coefficient."""
    p = torch.zeros(1, 10, dtype=torch.float64)
    for j in range(3):
        p[0, 1 + 3 * j], p[0, 2 + 3 * j], p[0, 3 + 3 * j] = mean[j], log_scale[j], coeff[j]
    return p


def test_draw_restatement_hand_built_cases():
    half = torch.full((1, 3), 0.5, dtype=torch.float64)  # v = 1/2: the logistic variate is 0, the draw is the mean
    one = torch.full((1, 1), 0.3, dtype=torch.float64)
    # one component, median draw: x = (m0, m1 + tanh(c0) m0, m2 + tanh(c1) x0 + tanh(c2) x1)
    x, gap = dref.draw(_one_component((0.25, -0.5, 0.1), (0.0, 0.0, 0.0), (0.5, -1.0, 2.0)), one, half, 1)
    t = torch.tanh(torch.tensor([0.5, -1.0, 2.0], dtype=torch.float64))
    x1 = -0.5 + t[0] * 0.25
    want = torch.stack((torch.tensor(0.25, dtype=torch.float64), x1, 0.1 + t[1] * 0.25 + t[2] * x1))
    assert torch.allclose(x[0], want, atol=1e-15, rtol=0) and gap[0] == float("inf")
    # uniforms at both clamps: the variate is +-log((1 - 1e-5) / 1e-5) times the scale
    lim = torch.log(torch.tensor((1.0 - 1e-5) / 1e-5, dtype=torch.float64))
    for v, sign in ((0.0, -1.0), (1.0, 1.0), (1e-9, -1.0)):
        x, _ = dref.draw(_one_component((0.0, 0.0, 0.0), (-3.0, -3.0, -3.0), (0.0, 0.0, 0.0)), one,
                         torch.full((1, 3), v, dtype=torch.float64), 1)
        assert torch.allclose(x[0], sign * torch.exp(torch.tensor(-3.0, dtype=torch.float64)) * lim.expand(3), atol=1e-12, rtol=0)
    # log-scale below the floor: -20 draws as -7
    a, _ = dref.draw(_one_component((0.0, 0.0, 0.0), (-20.0, -7.0, -6.0), (0.0, 0.0, 0.0)), one,
                     torch.full((1, 3), 0.9, dtype=torch.float64), 1)
    assert a[0, 0] == a[0, 1] and a[0, 2] > a[0, 1] > 0
    # means that clamp at +-1, and G / B following the CLAMPED R / G
    x, _ = dref.draw(_one_component((3.0, -3.0, 0.0), (0.0, 0.0, 0.0), (0.0, 0.0, 20.0)), one, half, 1)
    assert x[0].tolist() == [1.0, -1.0, -1.0]
    # the component choice: the largest perturbed logit wins, the gap is the margin to the runner-up
    p = torch.zeros(1, 20, dtype=torch.float64)
    p[0, 0], p[0, 1] = 0.0, 1.0
    p[0, 2], p[0, 3] = -0.5, 0.5  # red means of components 0 / 1
    same = torch.full((1, 2), 0.5, dtype=torch.float64)
    x, gap = dref.draw(p, same, half, 2)
    assert x[0, 0] == 0.5 and abs(float(gap[0]) - 1.0) < 1e-12
    tilt = torch.tensor([[1.0 - 1e-5, 1e-5]], dtype=torch.float64)  # Gumbel noise +11.5 on component 0, -2.4 on component 1
    x, _ = dref.draw(p, tilt, half, 2)
    assert x[0, 0] == -0.5


@pytest.mark.parametrize("k", sorted(dref.KERNEL_SEEDS))
def test_kernel_test_inputs_meet_their_conditions(k):
    """The inputs of tests/test_gpu_pcnnpp_sampling.py's kernel test: ranges as stated, and at most 1 % of the draws inside
    the near-tie band (a condition on the seeds, checked here; the expected share is of order 1e-4)."""
    total = excluded = 0
    for n in dref.KERNEL_BATCHES:
        params, uniforms, canvas, unknown = dref.kernel_case(dref.KERNEL_SEEDS[k], n, k)
        assert params.shape == (n, 10 * k, 1, 8) and uniforms.shape == (32, n, k + 3)
        sub = params[:, k:].reshape(n, 3, 3, k, 1, 8)
        assert float(sub[:, :, 0].abs().max()) <= 2.0
        assert -8.0 <= float(sub[:, :, 1].min()) and float(sub[:, :, 1].max()) <= 1.0
        if n >= 3:
            assert float(sub[:, :, 1].min()) < -7.0, "the floor is never crossed"
            assert float(params[:, :k].std()) > 1.0 or k == 1
        assert float(canvas.abs().max()) <= 1.0 and 0 < int(unknown.sum()) < unknown.numel()
        for r, c in dref.KERNEL_POSITIONS:
            want, gap = dref.apply(params, uniforms, canvas, unknown, k, r, c)
            assert float(want.abs().max()) <= 1.0
            total += n
            excluded += int((gap < dref.NEAR_TIE).sum())
    assert excluded <= 0.01 * total, (excluded, total)


# ---- the C-ABI without a device ----------------------------------------------------------------------------------------------------
def _dmol_sample(lib, n=2, k=5, h=4, w=8, r=0, c=0, params=16, uniforms=16, canvas=16, unknown=16, strides=(80, 8, 1)):
    return lib.pg_dmol_sample(params, *strides, uniforms, canvas, unknown, 0, n, k, h, w, r, c, 0, 0)


def test_entry_points_reject_bad_arguments(lib):
    from pytorch_generative_amd import _lib, ops

    assert ops.DMOL_SAMPLE_MAX_K >= 32
    for bad in (dict(n=0), dict(n=-1), dict(k=0), dict(k=-3), dict(h=0), dict(w=0), dict(h=-4), dict(w=-8),
                dict(h=6), dict(w=10), dict(h=3), dict(w=7), dict(k=ops.DMOL_SAMPLE_MAX_K + 1)):
        rc = _dmol_sample(lib, **bad)
        assert rc == -2, (bad, rc)
        with pytest.raises(ValueError):
            _lib.check(rc, "pg_dmol_sample")
    for bad in (dict(params=0), dict(uniforms=0), dict(canvas=0), dict(unknown=0), dict(r=4), dict(c=8), dict(r=-1),
                dict(strides=(80, 0, 1)), dict(strides=(0, 8, 1)), dict(strides=(80, 8, 0)), dict(strides=(-80, 8, 1))):
        assert _dmol_sample(lib, **bad) == -1, bad
    for fn in (lib.pg_col_subsample2, lib.pg_col_zero_insert2):
        assert fn(16, 16, 0, 8, 0) == -2 and fn(16, 16, -1, 8, 0) == -2
        assert fn(16, 16, 4, 0, 0) == -2 and fn(16, 16, 4, -2, 0) == -2
        assert fn(0, 16, 4, 8, 0) == -1 and fn(16, 0, 4, 8, 0) == -1
    assert lib.pg_col_subsample2(16, 16, 4, 7, 0) == -2  # an odd width has no even-column half


def test_return_params_needs_the_incremental_path():
    pp = _pp()
    for cls in (pp.PixelCNNpp, pp.PixelCNNppUnitRange):
        model = cls(in_channels=3, n_filters=4, n_resnet=1, n_mix=2)
        with pytest.raises(ValueError):
            model.sample(n_samples=1, image_size=(4, 4), incremental=False, return_params=True)
