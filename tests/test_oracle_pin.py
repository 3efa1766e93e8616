"""Pins the CPU oracle against the REAL reference, op by op, model by model and for a full train step.

The reference's own tests hold no numeric vectors for this path. What the reference modules were
given and what they returned, case by case, is stored in tests/golden/oracle_pin/ (written from the reference itself by
tests/golden/make_pin_golden.py); these tests run the oracle on the same inputs and compare."""

import numpy as np
import pytest
import torch

import _util
from oracle import models as omodels
from oracle import ops as oops
from oracle import train as otrain

_GOLD = {}


def gold(name):
    """The cases of tests/golden/oracle_pin/<name>.pt (loaded once per session)."""
    if name not in _GOLD:
        _GOLD[name] = _util.load_golden(f"oracle_pin/{name}")["cases"]
    return _GOLD[name]


def unpack_mask(m):
    """Inverse of make_pin_golden.pack_mask: the reference's 0 / 1 mask, same shape and dtype."""
    n = int(np.prod(m["shape"]))
    flat = np.unpackbits(m["bits"].numpy())[:n]
    return torch.from_numpy(flat.copy()).to(getattr(torch, m["dtype"])).reshape(m["shape"])


@pytest.mark.parametrize("k,mc", [(3, True), (3, False), (7, True), (5, False)])
def test_causal_mask_bit_exact(k, mc):
    mask = unpack_mask(gold("masks")["causal_mask"][(k, mc)])  # CausalConv2d(mc, 2, 3, kernel_size=k).mask
    assert torch.equal(mask[0, 0], oops.causal_mask(k, k, mc))
    assert torch.equal(mask, oops.causal_mask(k, k, mc).expand_as(mask))


@pytest.mark.parametrize("size,mc", [(16, True), (16, False), (784, False), (1024, True)])
def test_attention_mask_bit_exact(size, mc):
    assert torch.equal(unpack_mask(gold("masks")["attention_mask"][(size, mc)]), oops.attention_mask(size, mc))


@pytest.mark.parametrize("shape", [(2, 3, 32, 32), (1, 1, 28, 28), (2, 3, 8, 8), (1, 3, 64, 64)])
def test_posenc_bit_exact(shape):
    assert torch.equal(gold("masks")["posenc"][shape], oops.image_positional_encoding(shape))


def test_causal_conv_and_ln_and_gate():
    g = gold("layers")
    x = g["x"]
    assert torch.allclose(g["conv_out"], oops.causal_conv2d(x, g["conv_weight"], g["conv_bias"], True, 1), atol=1e-6)
    assert torch.allclose(g["ln_out"], oops.nchw_layernorm(x, g["ln_weight"], g["ln_bias"]), atol=1e-6)
    assert torch.allclose(g["gate_tanh_out"], oops.gated_activation(x, "tanh"), atol=1e-7)
    assert torch.allclose(g["gate_identity_out"], oops.gated_activation(x, "identity"), atol=1e-7)


@pytest.mark.parametrize("mc,heads,extra", [(False, 2, 0), (True, 1, 3)])
def test_attention_module(mc, heads, extra):
    g = gold("layers")["attention_module"][(mc, heads, extra)]
    got = oops.causal_attention(g["x"], g["extra"], g["params"], "", heads, 4, mc)
    assert torch.allclose(g["out"], got, atol=1e-6)


@pytest.mark.parametrize("name", ["image_gpt", "pixel_cnn", "gated_pixel_cnn", "pixel_snail"])
def test_model_forward_loss_grads_and_adam_step(name):
    """One reference train step (trainer.py:173-193 semantics: torch.optim.Adam, lr 1e-3) of a small model against the
    oracle's step on the same initial state: logits, loss, every gradient, the grad norm and the parameters after Adam."""
    g = gold("models")[name]
    state = {k: v.clone() for k, v in g["state0"].items()}
    o_logits, o_loss, o_grads = otrain.loss_and_grads(omodels.FORWARDS[name], state, g["x"], **g["oracle_kwargs"])
    assert torch.allclose(o_logits, g["logits"], rtol=1e-5, atol=1e-5)
    assert abs(float(o_loss) - float(g["loss"])) <= 1e-5 * abs(float(g["loss"]))
    for k, g_ref in g["grads"].items():
        if g_ref is None:
            assert o_grads[k] is None, k
        else:
            assert torch.allclose(o_grads[k], g_ref, rtol=1e-4, atol=1e-5), k
    o_norm = otrain.adam_step_(state, o_grads, otrain.new_opt_state(), lr=g["lr"])
    assert abs(o_norm - g["grad_norm"]) <= 1e-5 * g["grad_norm"]
    for k, p in g["params1"].items():
        assert torch.allclose(state[k], p, rtol=1e-5, atol=1e-6), k


def _vae_grads_match(g, grads):
    """The oracle's gradients (keyed by parameter name) against the reference's; a parameter the reference's ELBO does
    not reach must get no or an all-zero gradient from the oracle."""
    assert set(grads) == set(g["grads"])
    for k, want in g["grads"].items():
        go = grads[k]
        if want is None:
            assert go is None or float(go.abs().max()) == 0.0, k
        else:
            assert torch.allclose(go, want, rtol=1e-4, atol=1e-5), k


def test_vd_vae_forward_elbo_and_grads():
    """VD-VAE (vd_vae.py) with the reference's noise replayed: the reference ran with vaes.sample_from_gaussian patched
    to consume the pre-drawn eps the oracle is given here."""
    g = gold("vaes")["vd_vae"]
    x = g["x"]
    leaves = {k: v.clone().requires_grad_(True) for k, v in g["state0"].items() if otrain.is_param(k)}
    o_logits, o_kl = omodels.vd_vae(leaves, x, g["eps"])
    _, _, o_elbo = omodels.elbo_terms(o_logits, x, o_kl)
    grads = torch.autograd.grad(o_elbo, list(leaves.values()), allow_unused=True)
    assert torch.allclose(o_logits, g["logits"], rtol=1e-5, atol=1e-5)
    assert torch.allclose(o_kl, g["kl"], rtol=1e-5, atol=1e-4)
    _vae_grads_match(g, dict(zip(leaves, grads)))


def test_beta_vae_forward_elbo_and_grads():
    g = gold("vaes")["beta_vae"]
    x = g["x"]
    leaves = {k: v.clone().requires_grad_(True) for k, v in g["state0"].items() if otrain.is_param(k)}
    o_logits, o_kl = omodels.vae(leaves, x, g["eps"], beta=g["beta"])
    _, _, o_elbo = omodels.elbo_terms(o_logits, x, o_kl)
    grads = torch.autograd.grad(o_elbo, list(leaves.values()), allow_unused=True)
    assert torch.allclose(o_logits, g["logits"], rtol=1e-5, atol=1e-5)
    assert torch.allclose(o_kl, g["kl"], rtol=1e-5, atol=1e-4)
    assert all(v is not None for v in g["grads"].values())
    _vae_grads_match(g, dict(zip(leaves, grads)))


@pytest.mark.parametrize("use_ema,training", [(True, True), (True, False), (False, True)])
def test_vector_quantizer_live(use_ema, training):
    """oracle.ops.vector_quantize against the reference's VectorQuantizer (nn/utils.py:53-96), fresh seeds."""
    g = gold("vector_quantizer")[(use_ema, training)]
    before = g["before"]
    out = oops.vector_quantize(g["x"], before["_embedding"], before.get("_cluster_size"),
                               before.get("_embedding_avg"), use_ema=use_ema, training=training)
    assert torch.equal(out["quantized"], g["quantized"])
    assert torch.allclose(out["loss"], g["loss"], rtol=1e-6, atol=0)
    after = g["after"]
    for key in ("_embedding", "_cluster_size", "_embedding_avg"):
        if key in after:
            assert torch.allclose(out[key[1:]], after[key], rtol=1e-6, atol=1e-7), key


@pytest.mark.parametrize("heads,embed,out", [(1, 4, 32), (1, 4, 16), (2, 8, 64), (1, 16, 16), (1, 32, 32), (2, 64, 32),
                                              (1, 64, 64), (2, 16, 40), (1, 8, 20)],
                         ids=lambda v: str(v))
@pytest.mark.parametrize("mc", [False, True], ids=["incl_centre", "strict"])
def test_attention_module_head_dims_forward_and_gradients(heads, embed, out, mc):
    """The head dimensions the GPU tier exercises (d_k = embed / heads in {4, 8, 16, 32, 64}, d_v = out / heads in
    {16, 20, 32, 64}; tests/test_gpu_ops.py ATTN_CASES compare the HIP kernels with `oracle.ops.causal_attention_core`):
    the oracle against the reference module — output, input gradient and every parameter gradient."""
    g = gold("attention_head_dims")[(heads, embed, out, mc)]
    p = {k: v.clone().requires_grad_(True) for k, v in g["params"].items()}
    xo = g["x"].clone().requires_grad_(True)
    got = oops.causal_attention(xo, None, p, "", heads, embed, mc)
    got.backward(g["d_out"])
    assert torch.allclose(g["out"], got.detach(), atol=2e-6, rtol=1e-5)
    assert torch.allclose(g["x_grad"], xo.grad, atol=2e-6, rtol=1e-5)
    assert set(g["grads"]) <= set(p) and g["grads"]
    for k, v in g["grads"].items():
        assert torch.allclose(v, p[k].grad, atol=5e-6, rtol=1e-5), k
