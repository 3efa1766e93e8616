"""GPU: models that read code images (`input_codes`) against the oracle on one_hot(codes) with the same parameters, their
samplers, and the VQ-VAE's code I/O, prior hook and recipe.

Gates: _util.assert_close at 1e-4 for logits, 1e-5 for losses and sampler logits (the existing teacher-forcing tests'),
_util.GradReport (1e-4 / 5e-6) for gradients."""

import pytest
import torch
import torch.nn.functional as F

import _categorical_ref as cref
import _util
from oracle import models as omodels
from oracle import train as otrain

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
K = 8


def _gpt(in_size=4, blocks=2, heads=2, channels=8, sample_fn=None, seed=0, k=K):
    import pytorch_generative_amd as pg

    torch.manual_seed(seed)
    model = pg.models.ImageGPT(in_channels=k, out_channels=k, in_size=in_size, n_transformer_blocks=blocks,
                               n_attention_heads=heads, n_embedding_channels=channels, sample_fn=sample_fn)
    with torch.no_grad():
        model._pos.normal_(0, 0.1)
    model.input_codes = k
    return model.to(DEV)


def _pcnn(sample_fn=None, seed=0):
    import pytorch_generative_amd as pg

    torch.manual_seed(seed)
    model = pg.models.PixelCNN(in_channels=K, out_channels=K, n_residual=1, residual_channels=4, head_channels=8,
                               sample_fn=sample_fn)
    model.input_codes = K
    return model.to(DEV)


def _codes(n, h, w, seed=1, k=K):
    return torch.randint(0, k, (n, 1, h, w), generator=torch.Generator().manual_seed(seed))


def _one_hot(codes, k=K):
    return F.one_hot(codes[:, 0], k).permute(0, 3, 1, 2).double()


def _step(model, levels):
    from pytorch_generative_amd import ops

    model.zero_grad(set_to_none=True)
    logits = model(levels)
    loss = ops.categorical_nll_sum_mean(logits, levels, model.input_codes)
    loss.backward()
    torch.cuda.synchronize()
    dense = logits.dense() if isinstance(logits, ops.DeferredLogits) else logits
    return dense.detach(), loss.detach(), {k: p.grad.clone() for k, p in model.named_parameters()}


def _oracle_step(state, fwd, codes, k=K, **kw):
    leaves = {n: v.detach().double().cpu().clone().requires_grad_(otrain.is_param(n)) for n, v in state.items()}
    logits = fwd(leaves, _one_hot(codes, k), **kw)
    loss = cref.nll_per_sample(logits, cref.to_level(codes, k), k).mean()
    loss.backward()
    return logits.detach(), loss.detach(), {n: v.grad for n, v in leaves.items() if v.requires_grad}


def _against_oracle(what, model, fwd, codes, **kw):
    state = {n: v.clone() for n, v in model.state_dict().items()}
    logits, loss, grads = _step(model, cref.to_level(codes, model.input_codes).to(DEV))
    o_logits, o_loss, o_grads = _oracle_step(state, fwd, codes, model.input_codes, **kw)
    print(f"[code_prior] {what}: logits rel err {_util.rel_err(logits, o_logits):.3e}, loss {_util.rel_err(loss, o_loss):.3e}")
    _util.assert_close(logits, o_logits, 1e-4, f"{what} logits")
    _util.assert_close(loss, o_loss, 1e-5, f"{what} loss")
    assert set(grads) == set(o_grads)
    rep = _util.GradReport(what)
    for n in grads:
        rep.add(n, grads[n], o_grads[n])
    rep.finish()
    # the state_dict is the reference model's: same keys and shapes as on one-hot input (+ the lazily registered shape)
    assert {n: tuple(v.shape) for n, v in model.state_dict().items() if n not in ("_c", "_h", "_w")} == \
        {n: tuple(v.shape) for n, v in state.items()}


def test_image_gpt_matches_the_oracle_on_one_hot_input():
    model = _gpt()
    assert model._input.weight.shape == (8, K, 3, 3) and model._pos.shape == (1, K, 4, 4)
    _against_oracle("ImageGPT", model, omodels.image_gpt, _codes(3, 4, 4), n_heads=2)


def test_pixel_cnn_matches_the_oracle_on_one_hot_input():
    _against_oracle("PixelCNN", _pcnn(), omodels.pixel_cnn, _codes(3, 5, 5))


def _fused_gpt(**kw):
    """16 channels, 4 heads at the smallest in_size whose blocks take the fused kernels."""
    for size in range(2, 17):
        model = _gpt(in_size=size, heads=4, channels=16, **kw)
        probe = torch.empty(1, 16, size, size, device="meta")
        if all(b._fused_ok(probe) for b in model._transformer):
            return model, size
    pytest.fail("no in_size up to 16 takes the fused block kernels")


def test_image_gpt_on_the_fused_block_kernels_and_flat_adam():
    from pytorch_generative_amd import optim

    model, size = _fused_gpt()
    codes = _codes(3, size, size, seed=2)
    _against_oracle(f"ImageGPT fused {size}x{size}", model, omodels.image_gpt, codes, n_heads=4)
    # FlatAdam: the gradients land in the flat buffer (sinks) and match the no-sink run; a step trains
    levels = cref.to_level(codes, K).to(DEV)
    _, loss0, want = _step(model, levels)
    opt = optim.FlatAdam(model.parameters(), lr=1e-2)
    probe = torch.empty(1, 16, size, size, device="meta")
    assert all(b._fused_ok(probe) for b in model._transformer)
    opt.zero_grad()
    from pytorch_generative_amd import ops

    loss = ops.categorical_nll_sum_mean(model(levels), levels, K)
    loss.backward()
    torch.cuda.synchronize()
    rep = _util.GradReport("flat_grad vs no-sink run")
    for n, p in model.named_parameters():
        sink = ops._sink(p)
        assert sink is not None, n
        rep.add(n, sink.view_as(p), want[n])
    rep.finish()
    opt.step()
    with torch.no_grad():
        loss1 = ops.categorical_nll_sum_mean(model(levels), levels, K)
    assert float(loss1) < float(loss0), (float(loss0), float(loss1))


@pytest.mark.parametrize("name", ["ImageGPT", "PixelCNN"])
def test_causality(name):
    model, hw = (_gpt(), 4) if name == "ImageGPT" else (_pcnn(), 5)
    codes = _codes(2, hw, hw, seed=3)
    with torch.no_grad():
        base = model(cref.to_level(codes, K).to(DEV))
        for p in (0, hw + 1, hw * hw - 2):
            changed = codes.clone()
            changed.view(2, -1)[:, p] = (changed.view(2, -1)[:, p] + 3) % K
            out = model(cref.to_level(changed, K).to(DEV))
            a, b = out.flatten(2), base.flatten(2)
            assert torch.equal(a[:, :, :p + 1], b[:, :, :p + 1]), f"{name}: position {p} reaches the logits at or before it"
            assert not torch.equal(a[:, :, p + 1:], b[:, :, p + 1:]), f"{name}: position {p} reaches nothing"


class _Recorder:
    """sample_fn that records the logits it is shown and 'draws' the teacher's codes."""

    def __init__(self, levels):
        self.levels, self.seen = levels, []

    def __call__(self, logits):
        p = len(self.seen)
        self.seen.append(logits.clone())
        return self.levels.flatten(1)[:, p:p + 1]


@pytest.mark.parametrize("name", ["ImageGPT", "PixelCNN"])
def test_samplers_equal_the_full_forward(name):
    if name == "ImageGPT":
        model, hw = _fused_gpt()
        assert model._incremental_ok(3)
    else:
        model, hw = _pcnn(), 5
        assert model._row_decode and model._row_graph
    levels = cref.to_level(_codes(3, hw, hw, seed=4), K).to(DEV)
    with torch.no_grad():
        full = model(levels)  # also registers the (1, H, W) canvas shape
    want = full.flatten(2).permute(2, 0, 1)  # (H W, N, K)
    for canvas in (levels, torch.full_like(levels, -1.0)):  # fully known, and teacher forcing from an empty canvas
        rec = _Recorder(levels)
        model._sample_fn = rec
        out = model.sample(conditioned_on=canvas)
        assert torch.equal(out, levels)
        assert len(rec.seen) == hw * hw
        if name == "PixelCNN":  # the row step with the band of levels was captured: no host synchronisation in it
            assert model._row_step_captured is True
        _util.assert_close(torch.stack(rec.seen), want, 1e-5, f"{name}: incremental sampler logits vs the full forward")
    rec = _Recorder(levels)
    model._sample_fn = rec
    out = model.sample(conditioned_on=levels, incremental=False)
    assert torch.equal(out, levels)
    _util.assert_close(torch.stack(rec.seen), want, 1e-5, f"{name}: per-pixel full forwards vs one full forward")


def test_defer_head_with_input_codes():
    model, size = _fused_gpt()
    levels = cref.to_level(_codes(4, size, size, seed=5), K).to(DEV)
    model.defer_head = False
    _, want_loss, want = _step(model, levels)
    model.defer_head = True
    from pytorch_generative_amd import ops

    assert isinstance(model(levels), ops.DeferredLogits)
    _, loss, got = _step(model, levels)
    _util.assert_close(loss, want_loss, 1e-5, "defer_head loss")
    rep = _util.GradReport("defer_head with input_codes")
    for n in want:
        rep.add(n, got[n], want[n])
    rep.finish()


# ---- VQ-VAE -------------------------------------------------------------------------------------------------------------------
def _vqvae(seed=0):
    import pytorch_generative_amd as pg

    torch.manual_seed(seed)
    return pg.models.VectorQuantizedVAE(in_channels=1, out_channels=1, hidden_channels=8, n_residual_blocks=1,
                                        residual_channels=4, n_embeddings=4, embedding_dim=4).to(DEV)


def _images(n, seed=6):
    return torch.rand(n, 1, 8, 8, generator=torch.Generator().manual_seed(seed))


def test_vq_vae_code_io():
    vq = _vqvae()
    x = _images(3).to(DEV)
    vq.eval()
    with torch.no_grad():
        recon, _ = vq(x)
    idx = vq._quantizer._net[1].last_indices.clone()
    got = vq.encode_codes(x, return_indices=True)
    assert got.dtype == torch.int64 and got.shape == (3, 2, 2)
    assert torch.equal(got.flatten(), idx.to(torch.int64))
    levels = vq.encode_codes(x)
    assert levels.shape == (3, 1, 2, 2) and levels.dtype == torch.float32
    assert torch.equal(levels, cref.to_level(got, 4).unsqueeze(1))
    _util.assert_close(vq.decode_codes(levels), recon, 1e-4, "decode_codes(encode_codes(x)) vs forward")
    # training mode: the EMA buffers stay bit-identical
    vq.train()
    before = {n: b.clone() for n, b in vq.named_buffers()}
    vq.encode_codes(x)
    torch.cuda.synchronize()
    assert vq.training
    for n, b in vq.named_buffers():
        assert torch.equal(b, before[n]), n


def test_vq_vae_samples_through_a_prior():
    from pytorch_generative_amd import nn as pg_nn

    vq = _vqvae()
    x = _images(2).to(DEV)
    with pytest.raises(NotImplementedError, match="VQ-VAE does not support sampling"):
        vq.sample(2)
    prior = _gpt(in_size=2, blocks=1, heads=2, channels=4, sample_fn=pg_nn.CategoricalSampler(4), k=4)
    with torch.no_grad():
        prior(vq.encode_codes(x))
    vq.set_prior(prior)
    codes = vq.sample_codes(5)
    assert codes.shape == (5, 1, 2, 2)
    assert bool(torch.isin(codes, cref.levels(4).to(DEV)).all()), "sample_codes values are not levels of K"
    vq._sample_fn = lambda out: out  # the decoder's output itself
    out = vq.sample(2)
    assert out.shape == x.shape and bool(torch.isfinite(out).all())


def test_reproduce_prior_runs_two_batches(tmp_path):
    from pytorch_generative_amd.models.vae import vq_vae

    vq = _vqvae()
    loader = [(_images(4, seed=s), torch.zeros(4)) for s in (7, 8)]
    t = vq_vae.reproduce_prior(vq, n_epochs=1, batch_size=4, log_dir=str(tmp_path), debug_loader=loader)
    assert t._epoch == 1 and t._step == 2
    prior = vq._prior
    assert prior is t.model and prior.input_codes == 4
    assert prior._input.weight.shape == (64, 4, 3, 3) and len(prior._transformer) == 8
    assert all(bool(torch.isfinite(p).all()) for p in prior.parameters())
    out = vq.sample(2)
    assert out.shape == (2, 1, 8, 8) and bool(torch.isfinite(out).all())
