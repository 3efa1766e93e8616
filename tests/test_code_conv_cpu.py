"""CPU tier of the code-index convolution: the float64 reference (tests/_code_conv_ref.py) against F.conv2d on one-hot
input and its autograd; the host-side validation of the four entry points through the built library (no device: every
check runs before the first device call); the Python surface of `input_codes` and of the VQ-VAE prior hook."""

import ctypes
import os

import pytest
import torch
import torch.nn.functional as F

import _code_conv_ref as ref
import _ref

CASES = [
    # (N, K, Cout, H, W, kernel, mask_center or None, with -1 entries)
    (2, 5, 6, 3, 5, 7, True, False),   # an image smaller than the kernel
    (2, 4, 3, 4, 4, 3, True, True),
    (1, 7, 1, 1, 9, 3, False, True),
    (2, 3, 2, 5, 4, 3, None, False),
]


def _case(n, k, cout, h, w, ks, neg, seed=0):
    g = torch.Generator().manual_seed(seed)
    codes = torch.randint(0, k, (n, 1, h, w), generator=g)
    if neg:
        codes[torch.rand(codes.shape, generator=g) < 0.3] = -1
    weight = torch.randn(cout, k, ks, ks, generator=g, dtype=torch.float64)
    bias = torch.randn(cout, generator=g, dtype=torch.float64)
    return codes, weight, bias


@pytest.mark.parametrize("n,k,cout,h,w,ks,mc,neg", CASES)
def test_reference_equals_conv_on_one_hot(n, k, cout, h, w, ks, mc, neg):
    codes, weight, bias = _case(n, k, cout, h, w, ks, neg)
    mask = None if mc is None else ref.causal_mask(ks, ks, mc)
    pad = (ks // 2, ks // 2)
    got = ref.forward(codes, weight, bias, pad, mask)
    want = ref.dense(codes, weight, bias, pad, mask)
    assert got.shape == want.shape == (n, cout, h, w)
    assert torch.allclose(got, want, rtol=0, atol=1e-12)
    # the weight gradient is the unmasked one: autograd with respect to the PRODUCT weight * mask
    prod = (weight if mask is None else weight * mask).clone().requires_grad_(True)
    b = bias.clone().requires_grad_(True)
    out = F.conv2d(ref.one_hot(codes, k), prod, b, padding=pad)
    dy = torch.randn(out.shape, generator=torch.Generator().manual_seed(1), dtype=torch.float64)
    out.backward(dy)
    dw, db = ref.wgrad(codes, dy, k, (ks, ks), pad)
    assert torch.allclose(dw, prod.grad, rtol=0, atol=1e-12)
    assert torch.allclose(db, b.grad, rtol=0, atol=1e-12)
    dw2, db2 = ref.dense_wgrad(codes, dy, k, (ks, ks), pad)
    assert torch.allclose(dw, dw2, rtol=0, atol=1e-12) and torch.allclose(db, db2, rtol=0, atol=1e-12)
    # codes that never occur: exact zeros
    used = set(codes[codes >= 0].tolist())
    for c in range(k):
        if c not in used:
            assert not dw[:, c].any()


def test_level_round_trip_and_band():
    for k in (2, 3, 5, 255, 256, 257, 512, 1000, 4095, 4096):
        j = torch.arange(k)
        assert torch.equal(ref.to_codes(ref.to_levels(j, k), k), j)
    codes = torch.tensor([[[[-1, 0, 2]]]])
    assert torch.equal(ref.to_codes(ref.to_levels(codes, 3), 3), codes)
    # a row band (padding reduced by the upward reach, one output row) equals the matching row of the full call
    codes, weight, bias = _case(2, 4, 3, 5, 6, 3, False)
    mask = ref.causal_mask(3, 3, True)
    full = ref.forward(codes, weight, bias, (1, 1), mask)
    for row in range(5):
        band = torch.full((2, 1, 2, 6), -1, dtype=torch.long)
        band[:, :, 1] = codes[:, :, row]
        if row:
            band[:, :, 0] = codes[:, :, row - 1]
        got = ref.forward(band, weight, bias, (0, 1), mask, out_hw=(1, 6))
        assert torch.equal(got[:, :, 0], full[:, :, row])


def test_reference_equals_the_reference_modules():
    """Where the checkout of the reference exists (tests/_ref.py), its own CausalConv2d on one-hot input."""
    if not _ref.available():
        pytest.skip("no checkout of the reference on this machine")
    root = _ref.REF_ROOT
    import importlib.util

    # the one file, not the package: the package's __init__ imports its datasets and their dependencies
    path = os.path.join(root, "pytorch_generative", "nn", "convolution.py")
    spec = importlib.util.spec_from_file_location("_reference_convolution", path)
    rconv = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(rconv)
    codes, weight, bias = _case(2, 5, 4, 6, 6, 3, False)
    conv = rconv.CausalConv2d(True, in_channels=5, out_channels=4, kernel_size=3, padding=1).double()
    with torch.no_grad():
        conv.weight.copy_(weight)
        conv.bias.copy_(bias)
    want = conv(ref.one_hot(codes, 5))
    got = ref.forward(codes, weight, bias, (1, 1), ref.causal_mask(3, 3, True))
    assert torch.allclose(got, want.detach(), rtol=0, atol=1e-12)
    dy = torch.randn(want.shape, generator=torch.Generator().manual_seed(1), dtype=torch.float64)
    want.backward(dy)
    dw, db = ref.wgrad(codes, dy, 5, (3, 3), (1, 1))
    assert torch.allclose(dw, conv.weight.grad, rtol=0, atol=1e-12)
    assert torch.allclose(db, conv.bias.grad, rtol=0, atol=1e-12)


# ---- host-side validation through the built library (no device needed) ---------------------------------------------------------
PG_EINVAL, PG_ESHAPE = -1, -2
P = 4096  # a non-null address that is never dereferenced: every check precedes the first device call


def _taps(ks):
    from pytorch_generative_amd import _lib

    t = [(u, v) for u in range(ks) for v in range(ks)]
    return len(t), _lib.int_array([u for u, _ in t]), _lib.int_array([v for _, v in t])


def _fwd(lib, *, levels=P, w=P, out=P, ws=P, k=8, ws_floats=None, taps=None):
    nt, u, v = taps or _taps(3)
    need = lib.pg_code_conv_fwd_workspace_floats(4, max(min(k, 4096), 2), nt)
    return lib.pg_code_conv_fwd(levels, w, 0, out, 2, k, 4, 4, 4, 3, 3, 4, 4, nt, u, v, 1, 1, ws,
                                need if ws_floats is None else ws_floats, 0)


def _wgrad(lib, *, levels=P, dy=P, dw=P, ws=P, k=8, ws_floats=None):
    need = lib.pg_code_conv_wgrad_workspace_floats(2, max(min(k, 4096), 2), 4, 4, 4, 3, 3)
    return lib.pg_code_conv_wgrad(levels, dy, dw, 0, 0, 2, k, 4, 4, 4, 3, 3, 4, 4, 1, 1, ws,
                                  need if ws_floats is None else ws_floats, 0)


@pytest.mark.parametrize("k", [-1, 0, 1, 4097, 1 << 20])
def test_n_codes_outside_range_is_rejected(lib, k):
    assert _fwd(lib, k=k) == PG_ESHAPE
    assert _wgrad(lib, k=k) == PG_ESHAPE
    assert lib.pg_sample_embed_codes(P, P, P, P, P, 2, k, 4, 4, 4, 3, 3, 0, 0, 16, 0, 0) == PG_ESHAPE
    assert lib.pg_vq_lookup(P, P, P, 2, 4, 16, k, 0) == PG_ESHAPE
    a, b = ctypes.c_int(), ctypes.c_int()
    assert lib.pg_code_conv_wgrad_plan(2, k, 4, 4, ctypes.byref(a), ctypes.byref(b)) == PG_ESHAPE
    assert lib.pg_code_conv_fwd_workspace_floats(4, k, 9) == 0
    assert lib.pg_code_conv_wgrad_workspace_floats(2, k, 4, 4, 4, 3, 3) == 0


def test_null_operands_are_rejected(lib):
    for name in ("levels", "w", "out", "ws"):
        assert _fwd(lib, **{name: 0}) == PG_EINVAL, name
    for name in ("levels", "dy", "ws"):
        assert _wgrad(lib, **{name: 0}) == PG_EINVAL, name
    assert lib.pg_code_conv_wgrad(P, P, 0, 0, 0, 2, 8, 4, 4, 4, 3, 3, 4, 4, 1, 1, P, 1 << 30, 0) == PG_EINVAL  # neither dw nor db
    assert lib.pg_sample_embed_codes(0, P, P, P, P, 2, 8, 4, 4, 4, 3, 3, 0, 0, 16, 0, 0) == PG_EINVAL
    assert lib.pg_sample_embed_codes(P, P, P, P, 0, 2, 8, 4, 4, 4, 3, 3, 0, 0, 16, 0, 0) == PG_EINVAL
    assert lib.pg_sample_embed_codes(P, P, P, P, P, 2, 8, 4, 4, 4, 3, 3, 4, 0, 16, 0, 0) == PG_EINVAL  # row outside the image
    assert lib.pg_vq_lookup(P, 0, P, 2, 4, 16, 8, 0) == PG_EINVAL
    assert b"null" in lib.pg_last_error()
    # dimensions outside the range are shape errors on every entry point
    assert lib.pg_sample_embed_codes(P, P, P, P, P, 32, 8, 4, 4, 4, 3, 3, 0, 0, 16, 0, 0) == PG_ESHAPE  # ld < N
    assert lib.pg_sample_embed_codes(P, P, P, P, P, 2, 8, 0, 4, 4, 3, 3, 0, 0, 16, 0, 0) == PG_ESHAPE
    assert lib.pg_vq_lookup(P, P, P, 0, 4, 16, 8, 0) == PG_ESHAPE


def test_short_workspace_and_bad_taps_are_rejected(lib):
    from pytorch_generative_amd import _lib

    need = lib.pg_code_conv_fwd_workspace_floats(4, 8, 9)
    assert need == 9 * 8 * 4
    assert _fwd(lib, ws_floats=need - 1) == PG_EINVAL
    need = lib.pg_code_conv_wgrad_workspace_floats(2, 8, 4, 4, 4, 3, 3)
    assert need > 0
    assert _wgrad(lib, ws_floats=need - 1) == PG_EINVAL
    assert b"workspace" in lib.pg_last_error()
    # a tap list must be ascending (the summation order) and inside the kernel
    assert _fwd(lib, taps=(2, _lib.int_array([1, 0]), _lib.int_array([0, 0]))) == PG_EINVAL
    assert _fwd(lib, taps=(1, _lib.int_array([3]), _lib.int_array([0]))) == PG_EINVAL


def test_plan_is_monotone_in_positions(lib):
    a, b = ctypes.c_int(), ctypes.c_int()
    seen = []
    for n, h, w in [(1, 1, 1), (1, 8, 8), (2, 16, 16), (64, 16, 16), (64, 32, 32), (128, 32, 32), (256, 64, 64)]:
        assert lib.pg_code_conv_wgrad_plan(n, 32, h, w, ctypes.byref(a), ctypes.byref(b)) == 0
        assert a.value == -(-n * h * w // 512) and b.value == 32 + n * h * w // 512
        seen.append((a.value, b.value, lib.pg_code_conv_wgrad_workspace_floats(n, 32, h, w, 8, 3, 3)))
    assert seen == sorted(seen) and seen[0][0] == 1
    assert seen[3][0] >= 2  # (64, 32, ., 16, 16): the shape the GPU test merges chunks at


# ---- Python surface -------------------------------------------------------------------------------------------------------------
def test_input_codes_defaults_to_none_and_unsupported_models_raise():
    import pytorch_generative_amd as pg

    m = pg.models
    assert m.base.AutoregressiveModel.input_codes is None
    gpt = m.ImageGPT(in_channels=4, out_channels=4, in_size=4, n_transformer_blocks=1, n_attention_heads=2,
                     n_embedding_channels=4)
    assert gpt.input_codes is None and "input_codes" not in gpt.state_dict()
    for model in (m.GatedPixelCNN(in_channels=4, out_channels=4, n_gated=1, gated_channels=4, head_channels=4),
                  m.PixelSNAIL(in_channels=4, out_channels=4, n_channels=8, n_pixel_snail_blocks=1, n_residual_blocks=1,
                               attention_key_channels=2, attention_value_channels=4),
                  m.PixelCNNpp(in_channels=3, n_filters=4, n_resnet=1, n_mix=2),
                  m.MADE(input_dim=16, hidden_dims=[8], n_masks=1)):
        model.input_codes = 4
        shape = (1, 3, 4, 4) if isinstance(model, m.PixelCNNpp) else (1, 1, 4, 4)
        with pytest.raises(ValueError, match="input_codes"):
            model(torch.zeros(shape))
        if isinstance(model, (m.PixelCNNpp, m.MADE)):  # their samplers do not go through forward()
            with pytest.raises(ValueError, match="input_codes"):
                model.sample(conditioned_on=torch.full(shape, -2.0))


def test_cpu_tensors_and_wrong_code_counts_raise():
    import pytorch_generative_amd as pg
    from pytorch_generative_amd import nn as pg_nn
    from pytorch_generative_amd import ops

    conv = pg_nn.CausalConv2d(True, in_channels=4, out_channels=3, kernel_size=3, padding=1)
    before = conv.weight.detach().clone()
    with pytest.raises(ValueError, match="n_codes"):
        conv.forward_codes(torch.zeros(1, 1, 4, 4), 5)
    assert torch.equal(conv.weight, before)  # rejected before the in-place masking
    spec = ops.ConvSpec(3, 3, 1, 1)
    with pytest.raises(ValueError, match="n_codes"):
        ops.code_conv2d(torch.zeros(1, 1, 4, 4), torch.zeros(3, 4, 3, 3), None, spec, 5)
    with pytest.raises(ValueError, match="n_codes"):
        ops.code_conv2d(torch.zeros(1, 1, 4, 4), torch.zeros(3, 4097, 3, 3), None, spec, 4097)
    with pytest.raises(RuntimeError, match="cuda"):
        ops.code_conv2d(torch.zeros(1, 1, 4, 4), torch.zeros(3, 4, 3, 3), None, spec, 4)
    with pytest.raises(RuntimeError, match="cuda"):
        ops.vq_lookup(torch.zeros(1, 1, 2, 2), torch.zeros(4, 3))
    plain = pg_nn.Conv2d(4, 3, kernel_size=3, padding=1)
    with pytest.raises(RuntimeError, match="cuda"):
        plain.forward_codes(torch.zeros(1, 1, 4, 4), 4)
    assert pg.ops.code_conv_wgrad_plan(64, 32, 16, 16)[0] >= 2


def test_set_prior_leaves_the_vq_vae_as_it_is():
    import pytorch_generative_amd as pg

    m = pg.models
    vq = m.VectorQuantizedVAE(in_channels=1, out_channels=1, hidden_channels=8, n_residual_blocks=1, residual_channels=4,
                              n_embeddings=4, embedding_dim=4)
    with pytest.raises(NotImplementedError, match="VQ-VAE does not support sampling"):
        vq.sample(1)
    keys, params = list(vq.state_dict().keys()), [id(p) for p in vq.parameters()]
    prior = m.ImageGPT(in_channels=4, out_channels=4, in_size=2, n_transformer_blocks=1, n_attention_heads=2,
                       n_embedding_channels=4)
    vq.set_prior(prior)
    assert vq._prior is prior
    assert list(vq.state_dict().keys()) == keys and [id(p) for p in vq.parameters()] == params
    assert prior not in list(vq.modules())
    vq.set_prior(None)
    with pytest.raises(NotImplementedError, match="VQ-VAE does not support sampling"):
        vq.sample(1)
    with pytest.raises(NotImplementedError):
        vq.sample_codes(1)
