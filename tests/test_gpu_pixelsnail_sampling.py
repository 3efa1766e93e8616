"""GPU: PixelSNAIL.sample() on the cached row attention (ops.attention_row) with its row step captured into hipGraphs.

Teacher forcing, as tests/test_gpu_trainer.py does it: a known image is fed pixel by pixel through the sampler (the 'draw' is
the teacher's pixel), so every logit the sampler produced has a full forward to be compared with — at the project's bound for
the samplers, _util.assert_close at 1e-5; two routes that run the same kernels are compared with torch.equal."""

import pytest
import torch

import _util

pytestmark = pytest.mark.gpu

TOL = 1e-5
CASES = [(1, 6, 6), (3, 5, 7)]  # (in_channels, H, W)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need the MI355X"
    from pytorch_generative_amd import _lib

    _lib.load()
    return torch.device("cuda:0")


@pytest.fixture(scope="module", params=CASES, ids=lambda c: f"c{c[0]}-{c[1]}x{c[2]}")
def setup(request, dev):
    """(model, image, logits of one full forward), shared by the tests of a case."""
    import pytorch_generative_amd as pg

    c, h, w = request.param
    torch.manual_seed(0)
    model = pg.models.PixelSNAIL(in_channels=c, out_channels=c, n_channels=16, n_pixel_snail_blocks=2, n_residual_blocks=2,
                                 attention_key_channels=4, attention_value_channels=16).to(dev)
    x = torch.bernoulli(torch.full((2, c, h, w), 0.4)).to(dev)
    with torch.no_grad():
        full = model(x).detach()
    return model, x, full


def _teacher_forced(model, x, *, row_attention="decode", graph=True, conditioned_on=None):
    """sample(return_logits=True) with the teacher's pixels as draws; (canvas, logits, model._row_step_captured)."""
    import pytorch_generative_amd as pg

    h, w = x.shape[2:]
    pos = iter([(r, q) for r in range(h) for q in range(w)])

    def teacher(_logits):
        r, q = next(pos)
        return x[:, :, r, q]

    saved = model._sample_fn, pg.nn.CausalAttention.row_attention
    model._sample_fn = teacher
    pg.nn.CausalAttention.row_attention = row_attention
    model._row_graph = graph  # instance attribute over the class's
    try:
        start = torch.full_like(x, -1.0) if conditioned_on is None else conditioned_on
        canvas, logits = model.sample(conditioned_on=start, return_logits=True)
    finally:
        model._sample_fn, pg.nn.CausalAttention.row_attention = saved
        del model._row_graph
    return canvas, logits, model._row_step_captured


def test_defaults():
    import pytorch_generative_amd as pg

    assert pg.nn.CausalAttention.row_attention == "decode"
    assert pg.models.PixelSNAIL._row_graph is True and pg.models.PixelSNAIL._row_decode is True


def test_graphed_decode_route_equals_the_full_forward(setup):
    model, x, full = setup
    canvas, logits, captured = _teacher_forced(model, x)
    assert captured is True, "the row step of the decode route must be captured"
    assert torch.equal(canvas, x)
    print(f"[pixelsnail] decode graphed vs full forward: rel err {_util.rel_err(logits, full):.3e}")
    _util.assert_close(logits, full, TOL, "decode route, graphed: logits vs full forward")


def test_prefix_route_refuses_the_capture(setup):
    model, x, full = setup
    canvas, logits, captured = _teacher_forced(model, x, row_attention="prefix")
    assert captured is False, "the prefix route depends on the row index: its capture must be refused"
    assert torch.equal(canvas, x)
    _util.assert_close(logits, full, TOL, "prefix route, eager: logits vs full forward")


def test_graphed_equals_eager(setup):
    model, x, _ = setup
    canvas_g, logits_g, captured_g = _teacher_forced(model, x, graph=True)
    canvas_e, logits_e, captured_e = _teacher_forced(model, x, graph=False)
    assert captured_g is True and captured_e is False
    assert torch.equal(canvas_g, canvas_e) and torch.equal(logits_g, logits_e)


def test_given_pixels_are_kept(setup):
    """Entries >= 0 of conditioned_on survive whatever is drawn (here: the complement of the image)."""
    model, x, _ = setup
    given = torch.rand(x.shape, device=x.device) < 0.5
    start = torch.where(given, x, torch.full_like(x, -1.0))
    canvas, _, captured = _teacher_forced(model, 1.0 - x, conditioned_on=start)
    assert captured is True
    assert torch.equal(canvas[given], x[given]) and torch.equal(canvas[~given], (1.0 - x)[~given])


def test_unknown_route_is_an_error(setup):
    model, x, _ = setup
    with pytest.raises(ValueError):
        _teacher_forced(model, x, row_attention="nope", graph=False)
