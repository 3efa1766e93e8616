"""CPU tier of the upsampling code lookup: the float64 helper (tests/_code_up_ref.py) against index-by-index loops; the
conditional ImageGPT restatement with a zero `_cond.weight` against oracle.models.image_gpt; the host-side validation of the
entry points of csrc/code_up.hip through the built library (no device: every check runs before the first device call); the
Python surface of set_condition, nn.CodeUpsample and VectorQuantizedVAE2.set_priors."""

import ctypes

import pytest
import torch

import _code_up_ref as ref
from oracle import models as omodels

CASES = [
    # (N, K, Cout, h, w, f, with -1 entries)
    (1, 2, 1, 1, 1, 1, False),
    (2, 7, 5, 3, 5, 2, True),
    (2, 4, 3, 2, 3, 3, True),
    (1, 5, 2, 2, 2, 4, False),
]


def _case(n, k, cout, h, w, f, neg, seed=0):
    g = torch.Generator().manual_seed(seed)
    codes = torch.randint(0, k, (n, 1, h, w), generator=g)
    if neg:
        codes[torch.rand(codes.shape, generator=g) < 0.3] = -1
    weight = torch.randn(k, cout, f, f, generator=g, dtype=torch.float64)
    base = torch.randn(n, cout, h * f, w * f, generator=g, dtype=torch.float64)
    return codes, weight, base


@pytest.mark.parametrize("n,k,cout,h,w,f,neg", CASES)
def test_helper_equals_the_loops(n, k, cout, h, w, f, neg):
    codes, weight, base = _case(n, k, cout, h, w, f, neg)
    for b in (None, base):
        got, want = ref.code_upsample_ref(codes, weight, f, b), ref.code_upsample_loop(codes, weight, f, b)
        assert got.shape == want.shape == (n, cout, h * f, w * f)
        assert torch.allclose(got, want, rtol=0, atol=1e-12)
    dy = torch.randn(base.shape, generator=torch.Generator().manual_seed(1), dtype=torch.float64)
    dw, dw_loop = ref.code_upsample_wgrad_ref(codes, dy, k, f), ref.code_upsample_wgrad_loop(codes, dy, k, f)
    assert torch.allclose(dw, dw_loop, rtol=0, atol=1e-12)
    used = set(codes[codes >= 0].tolist())
    for c in range(k):
        if c not in used:
            assert not dw[c].any() and not dw_loop[c].any()
    # the levels decode to the codes they were made from, -1 included
    assert torch.equal(ref.to_codes(ref.to_levels(codes, k), k), codes)


def _gpt_params(k, channels, size, blocks, heads, seed=0):
    import pytorch_generative_amd as pg

    torch.manual_seed(seed)
    model = pg.models.ImageGPT(in_channels=k, out_channels=k, in_size=size, n_transformer_blocks=blocks,
                               n_attention_heads=heads, n_embedding_channels=channels)
    with torch.no_grad():
        model._pos.normal_(0, 0.1)
    return {n: v.detach().double().clone() for n, v in model.state_dict().items()}


def test_zero_condition_weight_is_the_unconditional_oracle():
    k, f = 6, 2
    p = _gpt_params(k, 8, 4, 2, 2)
    g = torch.Generator().manual_seed(3)
    codes = torch.randint(0, k, (2, 1, 4, 4), generator=g)
    cond = torch.randint(0, k, (2, 1, 2, 2), generator=g)
    x = ref.one_hot(codes, k)
    want = omodels.image_gpt(p, x, n_heads=2)
    p["_cond.weight"] = torch.zeros(k, 8, f, f, dtype=torch.float64)
    assert torch.equal(ref.image_gpt_cond(p, x, cond, 2, f), want)
    p["_cond.weight"] = torch.randn(k, 8, f, f, generator=g, dtype=torch.float64)
    assert not torch.equal(ref.image_gpt_cond(p, x, cond, 2, f), want)


# ---- host-side validation through the built library (no device needed) ---------------------------------------------------------
PG_EINVAL, PG_ESHAPE = -1, -2
P = 4096  # a non-null address that is never dereferenced: every check precedes the first device call


def _fwd(lib, *, levels=P, w=P, out=P, ws=P, k=8, f=2, ws_floats=None):
    need = lib.pg_code_up_fwd_workspace_floats(max(min(k, 4096), 2), 4, max(min(f, 4), 1))
    return lib.pg_code_up_fwd(levels, w, 0, out, 2, k, 4, 4, 4, f, ws, need if ws_floats is None else ws_floats, 0)


def _wgrad(lib, *, levels=P, dy=P, dw=P, ws=P, k=8, f=2, ws_floats=None):
    need = lib.pg_code_up_wgrad_workspace_floats(2, max(min(k, 4096), 2), 4, 4, 4, max(min(f, 4), 1))
    return lib.pg_code_up_wgrad(levels, dy, dw, 0, 2, k, 4, 4, 4, f, ws, need if ws_floats is None else ws_floats, 0)


def _cond(lib, *, cond=P, w=P, x=P, n=2, k=8, h=4, f=2, r=0, c=0, ld=16):
    return lib.pg_sample_cond_codes(cond, w, x, n, k, h, 4, 4, f, r, c, ld, 0, 0)


def _plan(lib, n, k, h, w):
    a, b = ctypes.c_int(-7), ctypes.c_int(-7)
    return lib.pg_code_up_plan(n, k, h, w, ctypes.byref(a), ctypes.byref(b)), a.value, b.value


@pytest.mark.parametrize("k", [1, 2, 4096, 4097])
def test_n_codes_range(lib, k):
    want = 0 if 2 <= k <= 4096 else PG_ESHAPE
    if want:  # (an accepted shape would launch: only the refusals are swept through the launching entry points)
        assert _fwd(lib, k=k) == want and _wgrad(lib, k=k) == want and _cond(lib, k=k) == want
    assert _plan(lib, 2, k, 4, 4)[0] == want
    assert (lib.pg_code_up_fwd_workspace_floats(k, 4, 2) == 0) == bool(want)
    assert (lib.pg_code_up_wgrad_workspace_floats(2, k, 4, 4, 4, 2) == 0) == bool(want)
    if not want:
        assert lib.pg_code_up_fwd_workspace_floats(k, 4, 2) == 4 * k * 4


@pytest.mark.parametrize("f", [0, 1, 4, 5])
def test_factor_range(lib, f):
    want = 0 if 1 <= f <= 4 else PG_ESHAPE
    if want:
        assert _fwd(lib, f=f) == want and _wgrad(lib, f=f) == want and _cond(lib, f=f) == want
        assert b"factor" in lib.pg_last_error()
    assert (lib.pg_code_up_fwd_workspace_floats(8, 4, f) == 0) == bool(want)
    assert (lib.pg_code_up_wgrad_workspace_floats(2, 8, 4, 4, 4, f) == 0) == bool(want)
    if not want:
        assert lib.pg_code_up_fwd_workspace_floats(8, 4, f) == f * f * 8 * 4


def test_null_operands_and_bad_dimensions_are_rejected(lib):
    for name in ("levels", "w", "out", "ws"):
        assert _fwd(lib, **{name: 0}) == PG_EINVAL, name
    for name in ("levels", "dy", "dw", "ws"):
        assert _wgrad(lib, **{name: 0}) == PG_EINVAL, name
    for name in ("cond", "w", "x"):
        assert _cond(lib, **{name: 0}) == PG_EINVAL, name
    assert b"null" in lib.pg_last_error()
    assert lib.pg_code_up_plan(2, 8, 4, 4, None, None) == PG_EINVAL
    assert _cond(lib, r=8) == PG_EINVAL and _cond(lib, c=8) == PG_EINVAL and _cond(lib, r=-1) == PG_EINVAL  # an 8 x 8 image
    assert _cond(lib, n=32) == PG_ESHAPE  # ld < N
    assert _cond(lib, h=0) == PG_ESHAPE
    assert lib.pg_code_up_fwd(P, P, 0, P, 0, 8, 4, 4, 4, 2, P, 1 << 20, 0) == PG_ESHAPE
    assert lib.pg_code_up_wgrad(P, P, P, 0, 2, 8, 4, 4, 0, 2, P, 1 << 20, 0) == PG_ESHAPE
    assert lib.pg_code_up_fwd(P, P, 0, P, 1 << 20, 8, 1 << 10, 1 << 10, 4, 2, P, 1 << 20, 0) == PG_ESHAPE  # 2^32 positions
    assert _plan(lib, 1 << 20, 8, 1 << 10, 1 << 10)[0] == PG_ESHAPE
    assert lib.pg_code_up_wgrad_workspace_floats(1 << 20, 8, 1 << 10, 1 << 10, 4, 2) == 0


def test_short_workspace_is_rejected(lib):
    need = lib.pg_code_up_fwd_workspace_floats(8, 4, 2)
    assert need == 4 * 8 * 4
    assert _fwd(lib, ws_floats=need - 1) == PG_EINVAL
    need = lib.pg_code_up_wgrad_workspace_floats(2, 8, 4, 4, 4, 2)
    assert need > 0
    assert _wgrad(lib, ws_floats=need - 1) == PG_EINVAL
    assert b"workspace" in lib.pg_last_error()


def test_plan(lib):
    rc, chunks, items = _plan(lib, 3, 2, 16, 16)
    assert rc == 0 and chunks >= 2 and (chunks, items) == (2, 2 + 1)  # 768 top positions: the chunk merge can run
    seen = []
    for n, h, w in [(1, 1, 1), (1, 8, 8), (2, 16, 16), (128, 8, 8), (64, 16, 16), (256, 32, 32)]:
        rc, a, b = _plan(lib, n, 32, h, w)
        assert rc == 0 and a == -(-n * h * w // 512) and b == 32 + n * h * w // 512
        seen.append((a, b, lib.pg_code_up_wgrad_workspace_floats(n, 32, h, w, 8, 2)))
    assert seen == sorted(seen) and seen[0][0] == 1


# ---- Python surface -------------------------------------------------------------------------------------------------------------
def _small_gpt(k=4, size=4, input_codes=True):
    import pytorch_generative_amd as pg

    model = pg.models.ImageGPT(in_channels=k, out_channels=k, in_size=size, n_transformer_blocks=1, n_attention_heads=2,
                               n_embedding_channels=4)
    if input_codes:
        model.input_codes = k
    return model


def test_set_condition_adds_exactly_one_key():
    from pytorch_generative_amd import nn as pg_nn

    model = _small_gpt()
    keys = list(model.state_dict().keys())
    assert not any(k.startswith("_cond") for k in keys) and not hasattr(model, "_cond")
    up = pg_nn.CodeUpsample(4, 4, 2)
    assert up.weight.shape == (4, 4, 2, 2) and not up.weight.any() and [n for n, _ in up.named_parameters()] == ["weight"]
    model.set_condition(up)
    assert model._cond is up
    assert list(model.state_dict().keys()) == keys + ["_cond.weight"]
    assert any(p is up.weight for p in model.parameters())
    model.set_condition(None)
    assert list(model.state_dict().keys()) == keys and not hasattr(model, "_cond")
    assert not any(p is up.weight for p in model.parameters())
    model.set_condition(None)  # nothing to remove: no error


def test_only_image_gpt_with_input_codes_takes_a_condition():
    import pytorch_generative_amd as pg
    from pytorch_generative_amd import nn as pg_nn

    m = pg.models
    up = pg_nn.CodeUpsample(4, 4, 2)
    for model in (m.PixelCNN(in_channels=4, out_channels=4, n_residual=1, residual_channels=4, head_channels=4),
                  m.GatedPixelCNN(in_channels=4, out_channels=4, n_gated=1, gated_channels=4, head_channels=4),
                  m.PixelSNAIL(in_channels=4, out_channels=4, n_channels=8, n_pixel_snail_blocks=1, n_residual_blocks=1,
                               attention_key_channels=2, attention_value_channels=4),
                  m.PixelCNNpp(in_channels=3, n_filters=4, n_resnet=1, n_mix=2),
                  m.MADE(input_dim=16, hidden_dims=[8], n_masks=1)):
        model.input_codes = 4
        with pytest.raises(ValueError, match="condition"):
            model.set_condition(up)
        assert "_cond.weight" not in model.state_dict()
    with pytest.raises(ValueError, match="input_codes"):
        _small_gpt(input_codes=False).set_condition(up)
    # forward: a cond without a module, a module without a cond, a cond of the wrong size — before any kernel is reached
    model = _small_gpt()
    x, cond = torch.zeros(1, 1, 4, 4), torch.zeros(1, 1, 2, 2)
    with pytest.raises(ValueError, match="condition module"):
        model(x, cond=cond)
    with pytest.raises(ValueError, match="condition module"):
        _small_gpt(input_codes=False)(torch.zeros(1, 4, 4, 4), cond=cond)
    model.set_condition(up)
    with pytest.raises(ValueError, match="needs `cond`"):
        model(x)
    with pytest.raises(ValueError, match="image size"):
        model(x, cond=torch.zeros(1, 1, 4, 4))
    with pytest.raises(ValueError, match="image size"):
        model.sample(cond=torch.zeros(2, 1, 3, 3), conditioned_on=torch.full((2, 1, 4, 4), -1.0))
    with pytest.raises(RuntimeError, match="cuda"):
        model(x, cond=cond)


def test_cpu_tensors_and_bad_arguments_raise():
    from pytorch_generative_amd import nn as pg_nn
    from pytorch_generative_amd import ops

    lv, w = torch.zeros(1, 1, 2, 2), torch.zeros(4, 3, 2, 2)
    with pytest.raises(RuntimeError, match="cuda"):
        ops.code_upsample(lv, w, 2)
    with pytest.raises(RuntimeError, match="cuda"):
        ops.code_upsample(lv, w, 2, base=torch.zeros(1, 3, 4, 4))
    with pytest.raises(RuntimeError, match="cuda"):
        ops.code_upsample_(torch.zeros(1, 3, 4, 4), lv, w, 2)
    with pytest.raises(RuntimeError, match="cuda"):
        pg_nn.CodeUpsample(4, 3, 2)(lv)
    with pytest.raises(RuntimeError, match="cuda"):
        pg_nn.CodeUpsample(4, 3, 2).add_position_(torch.zeros(3, 16), lv, None, 16)
    with pytest.raises(ValueError, match="factor"):
        ops.code_upsample(lv, torch.zeros(4, 3, 5, 5), 5)
    with pytest.raises(ValueError, match="weight"):
        ops.code_upsample(lv, torch.zeros(4, 3, 3, 3), 2)
    with pytest.raises(ValueError, match="base"):
        ops.code_upsample(lv, w, 2, base=torch.zeros(1, 3, 2, 2))
    with pytest.raises(ValueError, match="level image"):
        ops.code_upsample(torch.zeros(1, 2, 2, 2), w, 2)
    with pytest.raises(ValueError, match="n_codes"):
        pg_nn.CodeUpsample(4097, 3, 2)
    with pytest.raises(ValueError, match="factor"):
        pg_nn.CodeUpsample(4, 3, 5)
    assert ops.code_up_plan(3, 2, 16, 16)[0] >= 2


def _vqvae2():
    import pytorch_generative_amd as pg

    return pg.models.VectorQuantizedVAE2(in_channels=1, out_channels=1, hidden_channels=8, n_residual_blocks=1,
                                         residual_channels=4, n_embeddings=4, embedding_dim=4)


def test_set_priors_leaves_the_vq_vae_2_as_it_is():
    from pytorch_generative_amd import nn as pg_nn

    vq = _vqvae2()
    for call in (lambda: vq.sample(1), lambda: vq.sample_codes(1)):
        with pytest.raises(NotImplementedError, match="VQ-VAE-2 does not support sampling."):
            call()
    keys, params, mods = list(vq.state_dict().keys()), [id(p) for p in vq.parameters()], [id(m) for m in vq.modules()]
    top, bottom = _small_gpt(size=2), _small_gpt(size=4)
    bottom.set_condition(pg_nn.CodeUpsample(4, 4, 2))
    vq.set_priors(top, bottom)
    assert vq._priors == (top, bottom)
    assert list(vq.state_dict().keys()) == keys and [id(p) for p in vq.parameters()] == params
    assert [id(m) for m in vq.modules()] == mods
    with pytest.raises(ValueError, match="both"):
        vq.set_priors(top, None)
    vq.set_priors(None, None)
    for call in (lambda: vq.sample(1), lambda: vq.sample_codes(1)):
        with pytest.raises(NotImplementedError, match="VQ-VAE-2 does not support sampling."):
            call()


def test_conditional_trainer_and_recipe_surface():
    import inspect

    from pytorch_generative_amd import recipes, trainer
    from pytorch_generative_amd.models.vae import vq_vae_2

    assert issubclass(trainer.ConditionalTrainer, trainer.Trainer)
    assert trainer.ConditionalTrainer.train_one_batch is not trainer.Trainer.train_one_batch
    assert trainer.ConditionalTrainer.eval_one_batch is not trainer.Trainer.eval_one_batch
    assert inspect.signature(recipes.run).parameters["trainer_cls"].default is None
    assert callable(vq_vae_2.reproduce_priors)
    with pytest.raises(ValueError, match="level"):
        recipes.code_loaders_2(_vqvae2(), ([], []), "middle")
