"""VQ-VAE on the MI355X operator path (reference models/vae/vq_vae.py:19-81), plus what the reference leaves out: code
I/O (encode_codes / decode_codes), a hook for an autoregressive prior over the codes and the recipe that trains one, so
that sample() works once a prior is set. A code image is (N, 1, h, w) float32 at the levels j / (n_embeddings - 1)."""

import torch

from pytorch_generative_amd import ops
from pytorch_generative_amd.models.vae import vaes
from pytorch_generative_amd.nn import utils as nn_utils


class VectorQuantizedVAE(vaes.VariationalAutoEncoder):
    """vq_vae.py:19-81."""

    def __init__(self, in_channels=1, out_channels=1, hidden_channels=128, n_residual_blocks=2,
                 residual_channels=32, n_embeddings=128, embedding_dim=16, sample_fn=None):
        super().__init__(sample_fn)
        self._encoder = vaes.Encoder(in_channels, hidden_channels, hidden_channels, n_residual_blocks,
                                     residual_channels, stride=4)
        self._quantizer = vaes.Quantizer(hidden_channels, n_embeddings, embedding_dim)
        self._decoder = vaes.Decoder(embedding_dim, out_channels, hidden_channels, n_residual_blocks,
                                     residual_channels, stride=4)

    def forward(self, x):
        quantized, quantization_loss = self._quantizer(self._encoder(x))
        return self._decoder(quantized), quantization_loss

    # ---- code I/O and the prior (extensions) ----------------------------------------------------
    @torch.no_grad()
    def encode_codes(self, x, *, return_indices=False):
        """The code image of x: (N, 1, h, w) levels j / (n_embeddings - 1), or the int64 indices (N, h, w). The assignment
        only: the EMA buffers are never updated, whatever self.training is."""
        conv, vq = self._quantizer._net[0], self._quantizer._net[1]
        z = conv(self._encoder(x))
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
    def decode_codes(self, levels):
        """The decoder's output for a code image (N, 1, h, w): the codebook rows by index (ops.vq_lookup), decoded."""
        vq = self._quantizer._net[1]
        return self._decoder(ops.vq_lookup(levels, vq._embedding))

    def set_prior(self, prior):
        """Stores an autoregressive model over the code images (None removes it). It is NOT a submodule: state_dict()
        and parameters() of the VQ-VAE do not change."""
        object.__setattr__(self, "_prior", prior)

    @torch.no_grad()
    def sample_codes(self, n_samples):
        prior = getattr(self, "_prior", None)
        if prior is None:
            raise NotImplementedError("VQ-VAE does not support sampling.")
        return prior.sample(n_samples)

    def _sample(self, n_samples):
        if getattr(self, "_prior", None) is None:
            raise NotImplementedError("VQ-VAE does not support sampling.")
        return self.decode_codes(self.sample_codes(n_samples))


def reproduce(n_epochs=457, batch_size=128, log_dir="/tmp/run", n_gpus=1, device_id=0,
              debug_loader=None):
    """The reference's training recipe for this model (vq_vae.py:84-153: CIFAR-10 shaped data, 128 hidden
    channels, 512 codes of width 64, Adam lr 2e-4 with the per-batch 0.999977 decay, loss = MSE +
    quantization loss) on the MI355X path. Arguments as the reference; returns the Trainer."""
    from pytorch_generative_amd import recipes

    return recipes.run(
        lambda: VectorQuantizedVAE(in_channels=3, out_channels=3, hidden_channels=128,
                                   residual_channels=32, n_residual_blocks=2, n_embeddings=512,
                                   embedding_dim=64),
        loaders=recipes.cifar10, loss_fn=recipes.vq_loss(1.0), lr=2e-4, lr_decay=0.999977,
        n_epochs=n_epochs, batch_size=batch_size, log_dir=log_dir, n_gpus=n_gpus,
        device_id=device_id, debug_loader=debug_loader)


def reproduce_prior(vqvae, n_epochs=457, batch_size=128, log_dir="/tmp/run", n_gpus=1, device_id=0, debug_loader=None,
                    defer_head=False):
    """Second stage (the reference has NO such recipe: its VQ-VAE cannot sample): trains an ImageGPT prior on the code
    images of the frozen `vqvae` — 8 blocks, 2 heads, 64 channels, K-way softmax head and code-index stem (`input_codes`),
    Adam lr 5e-3 with the 0.999977 decay of the ImageGPT recipe, on the data of the VQ-VAE recipe — and installs it with
    vqvae.set_prior: vqvae.sample(n) then returns images. `debug_loader` yields (x, y) IMAGE batches. Returns the Trainer."""
    from pytorch_generative_amd import recipes
    from pytorch_generative_amd.models.autoregressive import image_gpt

    vq = vqvae._quantizer._net[1]
    k = vq.n_embeddings
    device = recipes._device(n_gpus, device_id)
    vqvae.to(device)
    image_loaders = (debug_loader, debug_loader) if debug_loader is not None else recipes.cifar10(batch_size)
    # the latent size, from one batch of the eval loader (a one-shot iterator as debug_loader loses that batch)
    h = int(vqvae.encode_codes(next(iter(image_loaders[1]))[0][:1].to(device)).shape[2])
    code_loaders = recipes.code_loaders(vqvae, image_loaders)

    def build():
        model = image_gpt.ImageGPT(in_channels=k, out_channels=k, in_size=h, n_transformer_blocks=8, n_attention_heads=2,
                                   n_embedding_channels=64, sample_fn=nn_utils.CategoricalSampler(k))
        model.input_codes = k
        vqvae.set_prior(model)
        return model

    return recipes.run(build, loaders=lambda _batch_size: code_loaders, loss_fn=recipes.categorical_loss(k), lr=5e-3,
                       lr_decay=0.999977, n_epochs=n_epochs, batch_size=batch_size, log_dir=log_dir, n_gpus=n_gpus,
                       device_id=device_id, debug_loader=None, defer_head=defer_head)
