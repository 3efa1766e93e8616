"""VQ-VAE-2 on the MI355X operator path (reference models/vae/vq_vae_2.py:21-110), plus what the reference leaves out, as
for VQ-VAE (vq_vae.py): code I/O at both levels, hooks for a prior over the top codes and a prior over the bottom codes given
the top codes, and the recipe that trains the two, so that sample() works once they are set. A code image is (N, 1, h, w)
float32 at the levels j / (n_embeddings - 1); the top one is half the bottom one's size."""

import torch

from pytorch_generative_amd import nn as pg_nn
from pytorch_generative_amd import ops
from pytorch_generative_amd.models.vae import vaes
from pytorch_generative_amd.nn import utils as nn_utils


class VectorQuantizedVAE2(vaes.VariationalAutoEncoder):
    """vq_vae_2.py:21-110."""

    def __init__(self, in_channels=1, out_channels=1, hidden_channels=128, n_residual_blocks=2,
                 residual_channels=32, n_embeddings=128, embedding_dim=16, sample_fn=None):
        super().__init__(sample_fn)
        enc = dict(hidden_channels=hidden_channels, n_residual_blocks=n_residual_blocks,
                   residual_channels=residual_channels, stride=2)
        self._encoder_b = vaes.Encoder(in_channels=in_channels, out_channels=hidden_channels, **enc)
        self._encoder_t = vaes.Encoder(in_channels=hidden_channels, out_channels=hidden_channels, **enc)
        self._quantizer_t = vaes.Quantizer(hidden_channels, n_embeddings, embedding_dim)
        self._quantizer_b = vaes.Quantizer(hidden_channels, n_embeddings, embedding_dim)
        self._decoder_t = vaes.Decoder(in_channels=embedding_dim, out_channels=hidden_channels, **enc)
        self._conv = pg_nn.Conv2d(in_channels=hidden_channels, out_channels=embedding_dim, kernel_size=1)
        self._decoder_b = vaes.Decoder(in_channels=2 * embedding_dim, out_channels=out_channels, **enc)

    def forward(self, x):
        encoded_b = self._encoder_b(x)
        encoded_t = self._encoder_t(encoded_b)
        quantized_t, vq_loss_t = self._quantizer_t(encoded_t)
        quantized_b, vq_loss_b = self._quantizer_b(encoded_b)
        decoded_t = self._decoder_t(quantized_t)
        xhat = self._decoder_b(torch.cat((self._conv(decoded_t), quantized_b), dim=1))
        # 0.5 * (vq_b + vq_t) + mse(decoded_t, encoded_b), vq_vae_2.py:110 (gradients to both arguments)
        return xhat, (vq_loss_b + vq_loss_t) * 0.5 + nn_utils.mse_loss(decoded_t, encoded_b)

    # ---- code I/O and the priors (extensions) ---------------------------------------------------
    @staticmethod
    def _assign(quantizer, encoded, return_indices):
        conv, vq = quantizer._net[0], quantizer._net[1]
        z = conv(encoded)
        if vq._use_ema:
            _, _, idx = nn_utils._VectorQuantize.apply(z, vq._embedding, vq._cluster_size, vq._embedding_avg, vq._decay,
                                                       False, True, None)
        else:
            _, _, idx = nn_utils._VectorQuantize.apply(z, vq._embedding, None, None, vq._decay, False, False, None)
        idx = idx.view(z.shape[0], z.shape[2], z.shape[3])
        if return_indices:
            return idx.to(torch.int64)
        return ops.codes_to_levels(idx, vq.n_embeddings).unsqueeze(1)

    @torch.no_grad()
    def encode_codes(self, x, *, return_indices=False):
        """(top, bottom): the code images of x, (N, 1, h, w) levels j / (n_embeddings - 1) each, or the int64 indices
        (N, h, w). The assignment only: the EMA buffers are never updated, whatever self.training is."""
        encoded_b = self._encoder_b(x)
        encoded_t = self._encoder_t(encoded_b)
        return (self._assign(self._quantizer_t, encoded_t, return_indices),
                self._assign(self._quantizer_b, encoded_b, return_indices))

    @torch.no_grad()
    def decode_codes(self, top, bottom):
        """The decoder's output for the two code images: the codebook rows by index (ops.vq_lookup) decoded as in forward."""
        quantized_t = ops.vq_lookup(top, self._quantizer_t._net[1]._embedding)
        quantized_b = ops.vq_lookup(bottom, self._quantizer_b._net[1]._embedding)
        decoded_t = self._decoder_t(quantized_t)
        return self._decoder_b(torch.cat((self._conv(decoded_t), quantized_b), dim=1))

    def set_priors(self, top, bottom):
        """Stores an autoregressive model over the top code images and one over the bottom code images that takes the top
        ones as `cond` (None, None removes them). They are NOT submodules: state_dict(), parameters() and modules() of the
        VQ-VAE-2 do not change."""
        if (top is None) != (bottom is None):
            raise ValueError("set_priors: both priors or neither")
        object.__setattr__(self, "_priors", None if top is None else (top, bottom))

    @torch.no_grad()
    def sample_codes(self, n_samples):
        priors = getattr(self, "_priors", None)
        if priors is None:
            raise NotImplementedError("VQ-VAE-2 does not support sampling.")
        top = priors[0].sample(n_samples)
        return top, priors[1].sample(cond=top)

    def _sample(self, n_samples):
        if getattr(self, "_priors", None) is None:
            raise NotImplementedError("VQ-VAE-2 does not support sampling.")
        return self.decode_codes(*self.sample_codes(n_samples))


def reproduce(n_epochs=457, batch_size=128, log_dir="/tmp/run", n_gpus=1, device_id=0,
              debug_loader=None):
    """The reference's training recipe for this model (vq_vae_2.py:117-186: as VQ-VAE with 64 residual
    channels and loss = MSE + 0.25 * quantization loss) on the MI355X path. Returns the Trainer."""
    from pytorch_generative_amd import recipes

    return recipes.run(
        lambda: VectorQuantizedVAE2(in_channels=3, out_channels=3, hidden_channels=128,
                                    n_residual_blocks=2, residual_channels=64, n_embeddings=512,
                                    embedding_dim=64),
        loaders=recipes.cifar10, loss_fn=recipes.vq_loss(0.25), lr=2e-4, lr_decay=0.999977,
        n_epochs=n_epochs, batch_size=batch_size, log_dir=log_dir, n_gpus=n_gpus,
        device_id=device_id, debug_loader=debug_loader)


def reproduce_priors(vqvae2, n_epochs=457, batch_size=128, log_dir="/tmp/run", n_gpus=1, device_id=0, debug_loader=None,
                     defer_head=False):
    """Second stage (the reference has NO such recipe: its VQ-VAE-2 cannot sample): trains two ImageGPT priors of
    vq_vae.reproduce_prior's size on the code images of the frozen `vqvae2` — 8 blocks, 2 heads, 64 channels, K-way softmax
    head and code-index stem (`input_codes`), Adam lr 5e-3 with the 0.999977 decay — one over the top codes, and one over the
    bottom codes that takes the top codes as context through nn.CodeUpsample(K, 64, 2) (trainer.ConditionalTrainer), and
    installs them with vqvae2.set_priors: vqvae2.sample(n) then returns images. `debug_loader` yields (x, y) IMAGE batches.
    Returns the two Trainers (top, bottom); their logs go to log_dir/top and log_dir/bottom."""
    import os

    from pytorch_generative_amd import recipes, trainer
    from pytorch_generative_amd.models.autoregressive import image_gpt

    k = vqvae2._quantizer_b._net[1].n_embeddings
    if vqvae2._quantizer_t._net[1].n_embeddings != k:
        raise ValueError("reproduce_priors: the two codebooks differ in size")
    device = recipes._device(n_gpus, device_id)
    vqvae2.to(device)
    image_loaders = (debug_loader, debug_loader) if debug_loader is not None else recipes.cifar10(batch_size)
    # the latent sizes, from one batch of the eval loader (a one-shot iterator as debug_loader loses that batch)
    top, bottom = vqvae2.encode_codes(next(iter(image_loaders[1]))[0][:1].to(device))
    sizes = {"top": int(top.shape[2]), "bottom": int(bottom.shape[2])}
    factor = sizes["bottom"] // sizes["top"]
    priors = {}

    def build(level):
        def fn():
            model = image_gpt.ImageGPT(in_channels=k, out_channels=k, in_size=sizes[level], n_transformer_blocks=8,
                                       n_attention_heads=2, n_embedding_channels=64,
                                       sample_fn=nn_utils.CategoricalSampler(k))
            model.input_codes = k
            if level == "bottom":
                model.set_condition(pg_nn.CodeUpsample(k, 64, factor))
            priors[level] = model
            return model

        return fn

    trainers = []
    for level, cls in (("top", None), ("bottom", trainer.ConditionalTrainer)):
        code_loaders = recipes.code_loaders_2(vqvae2, image_loaders, level)
        trainers.append(recipes.run(build(level), loaders=lambda _batch_size, cl=code_loaders: cl,
                                    loss_fn=recipes.categorical_loss(k), lr=5e-3, lr_decay=0.999977, n_epochs=n_epochs,
                                    batch_size=batch_size, log_dir=os.path.join(log_dir, level), n_gpus=n_gpus,
                                    device_id=device_id, debug_loader=None, defer_head=defer_head, trainer_cls=cls))
    vqvae2.set_priors(priors["top"], priors["bottom"])
    return tuple(trainers)
