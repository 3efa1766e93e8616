"""GPU: an ImageGPT that takes a coarser code image as context (set_condition / nn.CodeUpsample) against the float64
restatement (tests/_code_up_ref.py: image_gpt_cond), its samplers on every route, its captured training step, and VQ-VAE-2's
code I/O, priors and recipe.

Gates: _util.assert_close at 1e-4 for logits, 1e-5 for losses and sampler logits, _util.GradReport (1e-4 / 5e-6) for
gradients, torch.equal where the contract is "same bits" (a zero `_cond.weight`, locality, graph replays against eager steps
under ops.set_deterministic(True), as the existing capture-vs-eager tests)."""

import pytest
import torch

import _categorical_ref as cref
import _code_up_ref as ref
import _util
from oracle import train as otrain

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
K, F = 6, 2
# (in_size, blocks, heads, channels, the route the cached sampler takes): 16 channels at 16 positions are the fused block kernels
MODELS = {"blocks": (4, 2, 4, 16, "blocks"), "step": (6, 1, 2, 8, "step")}


def _gpt(name, *, cond=True, zero=False, sample_fn=None, seed=0):
    import pytorch_generative_amd as pg
    from pytorch_generative_amd import nn as pg_nn

    size, blocks, heads, channels, _ = MODELS[name]
    torch.manual_seed(seed)
    model = pg.models.ImageGPT(in_channels=K, out_channels=K, in_size=size, n_transformer_blocks=blocks,
                               n_attention_heads=heads, n_embedding_channels=channels, sample_fn=sample_fn)
    with torch.no_grad():
        model._pos.normal_(0, 0.1)
    model.input_codes = K
    if cond:
        up = pg_nn.CodeUpsample(K, channels, F)
        if not zero:
            with torch.no_grad():
                up.weight.normal_(0, 0.5)
        model.set_condition(up)
    return model.to(DEV)


def _codes(n, size, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, K, (n, 1, size, size), generator=g), torch.randint(0, K, (n, 1, size // F, size // F), generator=g)


def _levels(codes):
    return cref.to_level(codes, K).to(DEV)


@pytest.mark.parametrize("name", list(MODELS))
def test_forward_loss_and_gradients_match_float64(name):
    from pytorch_generative_amd import ops

    model, (size, _, heads, _, _) = _gpt(name), MODELS[name]
    probe = torch.empty(1, model._input.weight.shape[0], size, size, device="meta")
    assert all(b._fused_ok(probe) for b in model._transformer) == (name == "blocks")
    codes, cond = _codes(3, size, seed=1)
    state = {n: v.clone() for n, v in model.state_dict().items()}
    assert "_cond.weight" in state
    x, c = _levels(codes), _levels(cond)
    logits = model(x, cond=c)
    loss = ops.categorical_nll_sum_mean(logits, x, K)
    loss.backward()
    torch.cuda.synchronize()
    leaves = {n: v.detach().double().cpu().clone().requires_grad_(otrain.is_param(n)) for n, v in state.items()}
    assert leaves["_cond.weight"].requires_grad
    o_logits = ref.image_gpt_cond(leaves, ref.one_hot(codes, K), cond, heads, F)
    o_loss = cref.nll_per_sample(o_logits, cref.to_level(codes, K), K).mean()
    o_loss.backward()
    print(f"[code_cond] {name}: logits rel err {_util.rel_err(logits, o_logits):.3e}, loss {_util.rel_err(loss, o_loss):.3e}")
    _util.assert_close(logits, o_logits, 1e-4, f"{name} logits")
    _util.assert_close(loss, o_loss, 1e-5, f"{name} loss")
    rep = _util.GradReport(f"conditional ImageGPT {name}")
    grads = {n: p.grad for n, p in model.named_parameters()}
    assert set(grads) == {n for n, v in leaves.items() if v.requires_grad}
    for n, g in grads.items():
        rep.add(n, g, leaves[n].grad)
    rep.finish()


@pytest.mark.parametrize("name", list(MODELS))
def test_zero_condition_weight_has_the_bits_of_the_unconditional_model(name):
    size = MODELS[name][0]
    plain, model = _gpt(name, cond=False), _gpt(name, zero=True)
    codes, cond = _codes(3, size, seed=2)
    with torch.no_grad():
        assert torch.equal(model(_levels(codes), cond=_levels(cond)), plain(_levels(codes)))
    with pytest.raises(ValueError, match="needs `cond`"):
        model(_levels(codes))
    with pytest.raises(ValueError, match="condition module"):
        plain(_levels(codes), cond=_levels(cond))
    with pytest.raises(ValueError, match="image size"):
        model(_levels(codes), cond=_levels(codes))


def test_graph_replays_of_the_conditional_step_equal_eager_steps(tmp_path):
    """Four replays of the step ConditionalTrainer captures equal four eager steps bit for bit under
    ops.set_deterministic(True)."""
    from pytorch_generative_amd import ops, optim, recipes, trainer

    size = MODELS["blocks"][0]
    batches = [tuple(_levels(t) for t in _codes(4, size, seed=10 + i)) for i in range(4)]
    was = ops.set_deterministic(True)
    try:
        m1, m2 = _gpt("blocks"), _gpt("blocks")  # twins from one seed: the same flat layout
        cond0 = m1._cond.weight.detach().clone()
        runs = []
        for model, graph, sub in ((m1, False, "eager"), (m2, True, "graph")):
            opt = optim.FlatAdam(model.parameters(), lr=1e-3)
            assert ops._sink(model._cond.weight) is not None
            t = trainer.ConditionalTrainer(model=model, loss_fn=recipes.categorical_loss(K), optimizer=opt,
                                           train_loader=batches, eval_loader=batches, log_dir=str(tmp_path / sub), n_gpus=1,
                                           graph=graph)
            assert t._use_graph == graph
            losses = [t._train_one_batch(x, y)["loss"] for x, y in batches]
            runs.append((opt, t, losses))
        torch.cuda.synchronize()
        (o1, _, l1), (o2, t2, l2) = runs
        assert t2._use_graph and len(t2._graphs) == 1, "the conditional step was not captured"
        assert torch.equal(o1.flat_param, o2.flat_param), "graph replays differ from eager steps"
        assert torch.equal(o1.exp_avg, o2.exp_avg) and torch.equal(o1.exp_avg_sq, o2.exp_avg_sq)
        assert l1 == l2
        assert not torch.equal(m2._cond.weight, cond0), "four steps left the condition weight as it was"
    finally:
        ops.set_deterministic(was)


class _Recorder:
    """sample_fn that 'draws' the teacher's codes."""

    def __init__(self, levels):
        self.levels, self.n = levels, 0

    def __call__(self, logits):
        p, self.n = self.n, self.n + 1
        return self.levels.flatten(1)[:, p:p + 1]


def _routes(name):
    return ("blocks", "step", "full") if name == "blocks" else ("step", "full")


@pytest.mark.parametrize("name", list(MODELS))
def test_samplers_equal_the_full_forward_under_teacher_forcing(name):
    size, want_route = MODELS[name][0], MODELS[name][4]
    model = _gpt(name)
    codes, cond = _codes(3, size, seed=3)
    x, c = _levels(codes), _levels(cond)
    with torch.no_grad():
        full = model(x, cond=c)  # also registers the canvas shape
    want = full.flatten(2).permute(2, 0, 1)  # (H W, N, K)
    assert model._decode_route(3) == want_route
    for route in _routes(name):
        if route == "full":
            # the per-pixel loop: return_logits belongs to the cached sampler, so the logits are recorded by the sample_fn
            seen = []
            rec = _Recorder(x)
            model._sample_fn = lambda lg: (seen.append(lg.clone()), rec(lg))[1]
            out = model.sample(conditioned_on=torch.full_like(x, -1.0), cond=c, incremental=False)
            got = torch.stack(seen)
        else:
            model._sample_fn = _Recorder(x)
            out, got = model.sample(conditioned_on=x, cond=c, return_logits=True, route=None if route == want_route else route)
        assert model._sample_route == route
        assert torch.equal(out, x)
        assert got.shape == want.shape
        print(f"[code_cond] {name} route {route}: sampler logits rel err {_util.rel_err(got, want):.3e}")
        _util.assert_close(got, want, 1e-5, f"{name}: route {route} vs one full forward")
    # n comes from cond when nothing else says it; an empty canvas under teacher forcing reproduces the codes
    model._sample_fn = _Recorder(x)
    assert torch.equal(model.sample(cond=c), x)
    with pytest.raises(ValueError, match="needs `cond`"):
        model.sample(3)
    with pytest.raises(ValueError, match="cond holds"):
        model.sample(2, cond=c)


@pytest.mark.parametrize("name", list(MODELS))
def test_a_top_code_reaches_only_its_own_block(name):
    size = MODELS[name][0]
    model = _gpt(name)
    codes, cond = _codes(2, size, seed=5)
    x = _levels(codes)
    with torch.no_grad():
        base = model(x, cond=_levels(cond))
        far = cond.clone()
        far[:, 0, -1, -1] = (far[:, 0, -1, -1] + 1) % K    # its 2 x 2 block holds the last raster positions only
        out = model(x, cond=_levels(far))
        last_block_start = (size - F) * size + (size - F)
        assert torch.equal(out.flatten(2)[:, :, :last_block_start], base.flatten(2)[:, :, :last_block_start])
        assert not torch.equal(out, base)
        near = cond.clone()
        near[:, 0, 0, 0] = (near[:, 0, 0, 0] + 1) % K
        out = model(x, cond=_levels(near))
        assert not torch.equal(out[:, :, 0, 0], base[:, :, 0, 0]), "the code at (0, 0) does not reach position 0"
    # the same through the cached sampler's first position
    model._sample_fn = _Recorder(x)
    _, l_base = model.sample(conditioned_on=x, cond=_levels(cond), return_logits=True)
    model._sample_fn = _Recorder(x)
    _, l_far = model.sample(conditioned_on=x, cond=_levels(far), return_logits=True)
    model._sample_fn = _Recorder(x)
    _, l_near = model.sample(conditioned_on=x, cond=_levels(near), return_logits=True)
    assert torch.equal(l_far[0], l_base[0]) and not torch.equal(l_near[0], l_base[0])


# ---- VQ-VAE-2 -----------------------------------------------------------------------------------------------------------------
def _vqvae2(seed=0):
    import pytorch_generative_amd as pg

    g = _util.load_golden("vq_vae_2_small")
    torch.manual_seed(seed)
    model = pg.models.VectorQuantizedVAE2(**g["kwargs"]).to(DEV)
    model.load_state_dict(g["state0"])
    return model, g["x"].to(DEV)


def test_vq_vae_2_code_io():
    vq, x = _vqvae2()
    k = vq._quantizer_b._net[1].n_embeddings
    vq.eval()
    with torch.no_grad():
        recon, _ = vq(x)
    idx_t, idx_b = vq._quantizer_t._net[1].last_indices.clone(), vq._quantizer_b._net[1].last_indices.clone()
    top_i, bottom_i = vq.encode_codes(x, return_indices=True)
    n, h = x.shape[0], x.shape[2]
    assert top_i.dtype == bottom_i.dtype == torch.int64
    assert top_i.shape == (n, h // 4, h // 4) and bottom_i.shape == (n, h // 2, h // 2)
    assert torch.equal(top_i.flatten(), idx_t.to(torch.int64)) and torch.equal(bottom_i.flatten(), idx_b.to(torch.int64))
    top, bottom = vq.encode_codes(x)
    assert top.shape == (n, 1, h // 4, h // 4) and bottom.shape == (n, 1, h // 2, h // 2) and top.dtype == torch.float32
    assert torch.equal(top, cref.to_level(top_i, k).unsqueeze(1)) and torch.equal(bottom, cref.to_level(bottom_i, k).unsqueeze(1))
    _util.assert_close(vq.decode_codes(top, bottom), recon, 1e-4, "decode_codes(encode_codes(x)) vs forward")
    vq.train()  # training mode: the EMA buffers stay bit-identical
    before = {n_: b.clone() for n_, b in vq.named_buffers()}
    vq.encode_codes(x)
    torch.cuda.synchronize()
    assert vq.training
    for n_, b in vq.named_buffers():
        assert torch.equal(b, before[n_]), n_


def _prior(k, size, channels=8, cond=False, seed=0):
    import pytorch_generative_amd as pg
    from pytorch_generative_amd import nn as pg_nn

    torch.manual_seed(seed)
    model = pg.models.ImageGPT(in_channels=k, out_channels=k, in_size=size, n_transformer_blocks=1, n_attention_heads=2,
                               n_embedding_channels=channels, sample_fn=pg_nn.CategoricalSampler(k))
    model.input_codes = k
    if cond:
        model.set_condition(pg_nn.CodeUpsample(k, channels, 2))
        with torch.no_grad():
            model._cond.weight.normal_(0, 0.5)
    return model.to(DEV)


def test_vq_vae_2_samples_through_priors():
    vq, x = _vqvae2()
    k = vq._quantizer_b._net[1].n_embeddings
    with pytest.raises(NotImplementedError, match="VQ-VAE-2 does not support sampling."):
        vq.sample(2)
    top, bottom = vq.encode_codes(x)
    p_top, p_bottom = _prior(k, top.shape[2]), _prior(k, bottom.shape[2], cond=True)
    with torch.no_grad():  # registers the canvas shapes
        p_top(top)
        p_bottom(bottom, cond=top)
    vq.set_priors(p_top, p_bottom)
    s_top, s_bottom = vq.sample_codes(5)
    assert s_top.shape == (5,) + tuple(top.shape[1:]) and s_bottom.shape == (5,) + tuple(bottom.shape[1:])
    lv = cref.levels(k).to(DEV)
    assert bool(torch.isin(s_top, lv).all()) and bool(torch.isin(s_bottom, lv).all()), "sampled values are not levels of K"
    vq._sample_fn = lambda out: out  # the decoder's output itself
    out = vq.sample(2)
    assert out.shape == (2,) + tuple(x.shape[1:]) and bool(torch.isfinite(out).all())


def test_reproduce_priors_runs_two_batches(tmp_path):
    from pytorch_generative_amd import nn as pg_nn
    from pytorch_generative_amd.models.vae import vq_vae_2

    vq, x = _vqvae2()
    k = vq._quantizer_b._net[1].n_embeddings
    g = torch.Generator().manual_seed(7)
    loader = [(torch.rand(tuple(x.shape), generator=g), torch.zeros(x.shape[0])) for _ in range(2)]
    t_top, t_bottom = vq_vae_2.reproduce_priors(vq, n_epochs=1, batch_size=x.shape[0], log_dir=str(tmp_path),
                                                debug_loader=loader)
    for t in (t_top, t_bottom):
        assert t._epoch == 1 and t._step == 2
        assert all(bool(torch.isfinite(p).all()) for p in t.model.parameters())
    top, bottom = vq._priors
    assert top is t_top.model and bottom is t_bottom.model and top.input_codes == bottom.input_codes == k
    assert not hasattr(top, "_cond") and isinstance(bottom._cond, pg_nn.CodeUpsample)
    assert bottom._cond.weight.shape == (k, 64, 2, 2) and bool(bottom._cond.weight.any()), "the condition weight did not train"
    assert bottom._input.weight.shape == (64, k, 3, 3) and len(bottom._transformer) == len(top._transformer) == 8
    assert t_bottom._use_graph and len(t_bottom._graphs) == 1, "the conditional step was not captured"
    vq._sample_fn = lambda out: out
    out = vq.sample(2)
    assert out.shape == (2,) + tuple(x.shape[1:]) and bool(torch.isfinite(out).all())
