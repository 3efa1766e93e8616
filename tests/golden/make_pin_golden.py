"""Generates tests/golden/oracle_pin/*.pt from the REAL reference (run in the build container only):

    python tests/golden/make_pin_golden.py

tests/test_oracle_pin.py pins the CPU oracle op by op, model by model and for a full train step against the reference.
Each file holds, for every case of one test, what the reference module was given (state, inputs, the noise it drew) and
what it returned (outputs, loss, gradients, state after the step), computed exactly as the test used to compute them
against the live modules. The test then runs only the oracle, so it needs nothing outside the repository.

Masks (0 / 1 float planes) are stored bit-packed: the 1024 x 1024 attention mask is 4 MB as float32.
"""

import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "oracle_pin")
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import _ref  # noqa: E402
from oracle import models as omodels  # noqa: E402
from oracle import ops as oops  # noqa: E402

# the parametrisations of tests/test_oracle_pin.py
CAUSAL_MASKS = [(3, True), (3, False), (7, True), (5, False)]
ATTN_MASKS = [(16, True), (16, False), (784, False), (1024, True)]
POSENC = [(2, 3, 32, 32), (1, 1, 28, 28), (2, 3, 8, 8), (1, 3, 64, 64)]
ATTN_MODULES = [(False, 2, 0), (True, 1, 3)]
MODELS = ["image_gpt", "pixel_cnn", "gated_pixel_cnn", "pixel_snail"]
VQ = [(True, True), (True, False), (False, True)]
HEAD_DIMS = [(1, 4, 32), (1, 4, 16), (2, 8, 64), (1, 16, 16), (1, 32, 32), (2, 64, 32), (1, 64, 64), (2, 16, 40), (1, 8, 20)]


def pack_mask(m):
    """0 / 1 tensor -> {bits, shape, dtype}; tests/test_oracle_pin.py's unpack_mask restores it exactly."""
    flat = m.reshape(-1)
    assert bool(((flat == 0) | (flat == 1)).all())
    return {"bits": torch.from_numpy(np.packbits(flat.numpy().astype(np.uint8))), "shape": tuple(m.shape),
            "dtype": str(m.dtype).replace("torch.", "")}


def grads_of(module):
    return {k: (p.grad.clone() if p.grad is not None else None) for k, p in module.named_parameters()}


def masks(ref):
    from pytorch_generative.nn import attention

    causal = {}
    for k, mc in CAUSAL_MASKS:
        conv = ref.nn.CausalConv2d(mc, 2, 3, kernel_size=k, padding=k // 2)
        causal[(k, mc)] = pack_mask(conv.mask)
    attn = {(size, mc): pack_mask(attention._get_causal_mask(size, mc)) for size, mc in ATTN_MASKS}
    posenc = {shape: ref.nn.image_positional_encoding(shape) for shape in POSENC}
    return {"causal_mask": causal, "attention_mask": attn, "posenc": posenc}


def layers(ref):
    torch.manual_seed(0)
    x = torch.randn(2, 4, 9, 9)
    conv = ref.nn.CausalConv2d(True, 4, 6, kernel_size=3, padding=1)
    w0 = conv.weight.detach().clone()
    y = conv(x).detach()
    ln = ref.nn.NCHWLayerNorm(4)
    with torch.no_grad():
        ln.weight.uniform_(0.5, 1.5)
        ln.bias.uniform_(-1, 1)
    ga = ref.nn.GatedActivation(activation_fn=torch.nn.Identity())
    out = {"x": x, "conv_weight": w0, "conv_bias": conv.bias.detach().clone(), "conv_out": y,
           "ln_weight": ln.weight.detach().clone(), "ln_bias": ln.bias.detach().clone(), "ln_out": ln(x).detach(),
           "gate_tanh_out": ref.nn.GatedActivation()(x).detach(), "gate_identity_out": ga(x).detach()}
    modules = {}
    for mc, heads, extra in ATTN_MODULES:
        torch.manual_seed(1)
        attn = ref.nn.CausalAttention(6, n_heads=heads, embed_channels=4, out_channels=8,
                                      mask_center=mc, extra_input_channels=extra)
        xa = torch.randn(2, 6, 5, 5)
        ex = torch.randn(2, extra, 5, 5) if extra else None
        p = {k: v.detach().clone() for k, v in attn.state_dict().items()}
        modules[(mc, heads, extra)] = {"x": xa, "extra": ex, "params": p, "out": attn(xa, ex).detach()}
    out["attention_module"] = modules
    return out


def build_model(ref, name):
    """tests/test_oracle_pin.py's former _build: the same seeds, the same constructors."""
    torch.manual_seed(0)
    m = ref.models
    if name == "image_gpt":
        return m.ImageGPT(1, 1, in_size=8, n_transformer_blocks=2, n_attention_heads=2,
                          n_embedding_channels=8), (2, 1, 8, 8), {"n_heads": 2}
    if name == "pixel_cnn":
        return m.PixelCNN(1, 1, n_residual=2, residual_channels=4, head_channels=4), (2, 1, 9, 9), {}
    if name == "gated_pixel_cnn":
        return m.GatedPixelCNN(3, 3, n_gated=2, gated_channels=4, head_channels=4), (2, 3, 9, 9), {}
    return m.PixelSNAIL(3, 3, n_channels=8, n_pixel_snail_blocks=2, n_residual_blocks=2,
                        attention_key_channels=2, attention_value_channels=4), (2, 3, 8, 8), {}


def models(ref):
    out = {}
    for name in MODELS:
        model, shape, kw = build_model(ref, name)
        if name == "image_gpt":  # _pos is zero-initialised; make it matter
            with torch.no_grad():
                model._pos.normal_(0, 0.1)
        g = torch.Generator().manual_seed(7)
        x = torch.rand(shape, generator=g)
        state = _ref.clone_state(model)
        # reference step (trainer.py:173-193 semantics)
        opt = torch.optim.Adam(model.parameters(), lr=1e-3)
        opt.zero_grad()
        logits = model(x)
        loss = oops.bce_sum_mean(logits, x)  # same formula as every reproduce().loss_fn
        loss.backward()
        norm = torch.nn.utils.clip_grad_norm_(model.parameters(), 1e50)
        grads = grads_of(model)
        opt.step()
        out[name] = {"state0": state, "x": x, "oracle_kwargs": kw, "lr": 1e-3, "logits": logits.detach(),
                     "loss": loss.detach(), "grad_norm": float(norm), "grads": grads,
                     "params1": {k: p.detach().clone() for k, p in model.named_parameters()}}
    return out


def vaes(ref):
    from pytorch_generative.models.vae import vaes as rvaes
    from pytorch_generative.models.vae import vd_vae as rvd

    orig = rvaes.sample_from_gaussian
    # VD-VAE (vd_vae.py) with the noise replayed: vaes.sample_from_gaussian is resolved by attribute lookup at call time
    torch.manual_seed(0)
    cfg = [rvd.StackConfig(2, 2), rvd.StackConfig(1, 2), rvd.StackConfig(1, 1)]
    model = ref.models.VeryDeepVAE(3, 3, input_resolution=8, stack_configs=cfg, latent_channels=4,
                                   hidden_channels=8, bottleneck_channels=4)
    with torch.no_grad():
        for b in model._biases:
            b.normal_(0, 0.1)
    x = torch.rand(2, 3, 8, 8, generator=torch.Generator().manual_seed(3))
    state = _ref.clone_state(model)
    eg = torch.Generator().manual_seed(4321)
    eps = [torch.randn(s, generator=eg) for s in omodels.vd_vae_noise_shapes(state, 2, 8)]
    it = iter(eps)
    rvaes.sample_from_gaussian = lambda mu, log_sig: mu + log_sig.exp() * next(it)
    try:
        logits, kl = model(x)
    finally:
        rvaes.sample_from_gaussian = orig
    _, _, elbo = omodels.elbo_terms(logits, x, kl)
    elbo.backward()
    vd = {"state0": state, "x": x, "eps": eps, "logits": logits.detach(), "kl": kl.detach(), "grads": grads_of(model)}

    torch.manual_seed(0)
    model = ref.models.BetaVAE(3, 3, beta=4.0, latent_channels=4, strides=[2, 4], hidden_channels=8,
                               residual_channels=4)
    x = torch.rand(2, 3, 16, 16, generator=torch.Generator().manual_seed(3))
    state = _ref.clone_state(model)
    eps = torch.randn(2, 4, 2, 2, generator=torch.Generator().manual_seed(4321))
    rvaes.sample_from_gaussian = lambda mu, log_sig: mu + log_sig.exp() * eps
    try:
        logits, kl = model(x)
    finally:
        rvaes.sample_from_gaussian = orig
    _, _, elbo = omodels.elbo_terms(logits, x, kl)
    elbo.backward()
    beta = {"state0": state, "x": x, "eps": eps, "beta": 4.0, "logits": logits.detach(), "kl": kl.detach(),
            "grads": grads_of(model)}
    return {"vd_vae": vd, "beta_vae": beta}


def vector_quantizer(ref):
    out = {}
    for use_ema, training in VQ:
        torch.manual_seed(11)
        vq = ref.nn.VectorQuantizer(n_embeddings=32, embedding_dim=6, use_ema=use_ema)
        vq.train(training)
        before = _ref.clone_state(vq)
        x = torch.randn(4, 6, 7, 5)
        q, loss = vq(x)
        out[(use_ema, training)] = {"before": before, "x": x, "quantized": q.detach(), "loss": loss.detach(),
                                    "after": _ref.clone_state(vq)}
    return out


def attention_head_dims(ref):
    out = {}
    for heads, embed, cout in HEAD_DIMS:
        for mc in (False, True):
            torch.manual_seed(3)
            cin = 6
            attn = ref.nn.CausalAttention(cin, n_heads=heads, embed_channels=embed, out_channels=cout, mask_center=mc)
            x = torch.randn(2, cin, 4, 5)
            d_o = torch.randn(2, cout, 4, 5)
            p = {k: v.detach().clone() for k, v in attn.state_dict().items()}
            xr = x.clone().requires_grad_(True)
            attn(xr).backward(d_o)
            out[(heads, embed, cout, mc)] = {"x": x, "d_out": d_o, "params": p, "out": attn(x).detach(),
                                              "x_grad": xr.grad.clone(), "grads": grads_of(attn)}
    return out


def main():
    ref = _ref.load()
    os.makedirs(OUT, exist_ok=True)
    meta = {"torch_version": torch.__version__, "cpu_capability": torch.backends.cpu.get_cpu_capability()}
    for name, fn in [("masks", masks), ("layers", layers), ("models", models), ("vaes", vaes),
                     ("vector_quantizer", vector_quantizer), ("attention_head_dims", attention_head_dims)]:
        path = os.path.join(OUT, name + ".pt")
        torch.save({**meta, "cases": fn(ref)}, path)
        print(f"wrote {path} ({os.path.getsize(path) / 1e3:.0f} kB)")


if __name__ == "__main__":
    main()
