"""The shared body of every model module's reproduce() (reference e.g.
models/autoregressive/image_gpt.py:112-175, models/vae/vae.py:104-167).

A reference recipe is: loaders -> model -> Adam (+ per-batch MultiplicativeLR) -> loss_fn ->
Trainer(...).interleaved_train_and_eval(n_epochs). The MI355X version keeps the hyper-parameters
and the Trainer contract and swaps the moving parts for the native ones: the model is built on
its GPU, `optim.FlatAdam` holds parameters / gradients / moments in flat buffers with the lr decay
applied on the device, the losses are the HIP loss kernels, and the Trainer replays the step from
a hipGraph.
"""

import torch

from pytorch_generative_amd import datasets, ops, optim, trainer


def bce_loss(x, _, preds):
    """sum-over-pixels, mean-over-batch BCE with logits (image_gpt.py:158-162 and the other
    autoregressive recipes)."""
    return ops.bce_with_logits_sum_mean(preds, x)


def categorical_loss(n_classes):
    """loss_fn of a model with a K-way softmax head (out_channels = n_classes * in_channels, class-major): sum-over-sub-pixels,
    mean-over-batch negative log-likelihood of images at the levels j / (n_classes - 1) (`grey_mnist` for 256)."""

    def loss_fn(x, _, preds):
        return ops.categorical_nll_sum_mean(preds, x, n_classes)

    return loss_fn


def elbo_loss(x, _, preds):
    """{"recon_loss", "kl_div", "loss"} of the VAE recipes (vae.py:149-159)."""
    logits, kl_div = preds
    recon, kl = ops.elbo_terms(logits, x, kl_div)
    return {"recon_loss": recon, "kl_div": kl, "loss": recon + kl}


def nice_loss(x, _, preds):
    """{"loss", "prior_log_likelihood", "log_det_J"} of NICE's recipe (flow/nice.py:205-213): the logistic prior's log-density
    of z summed per sample (ops.logistic_logprob) plus log det J, negated and averaged over the batch."""
    z, log_det_j = preds
    log_prob = ops.logistic_logprob(z)
    prior = log_prob.mean()
    return {"loss": -(prior + log_det_j), "prior_log_likelihood": prior, "log_det_J": log_det_j}


def _device(n_gpus, device_id):
    if not torch.cuda.is_available():
        raise RuntimeError("reproduce(): this path needs an MI355X (no CPU fallback)")
    index = device_id if (n_gpus > 1 and device_id is not None) else torch.cuda.current_device()
    torch.cuda.set_device(index)
    return torch.device("cuda", index)


def run(build_model, *, loaders, loss_fn, lr, lr_decay=1.0, n_epochs, batch_size, log_dir, n_gpus,
        device_id, debug_loader, defer_head=False, trainer_cls=None):
    """Builds everything a recipe names and trains for `n_epochs`; returns the Trainer. defer_head=True sets the attribute
    of that name on the model (autoregressive models with a categorical head: the head runs inside the loss kernels).
    trainer_cls: a Trainer subclass with the same constructor (trainer.ConditionalTrainer), default trainer.Trainer."""
    device = _device(n_gpus, device_id)
    if debug_loader is not None:
        train_loader = test_loader = debug_loader
    else:
        train_loader, test_loader = loaders(batch_size)
    model = build_model().to(device)
    if defer_head:
        model.defer_head = True
    optimizer = optim.FlatAdam(model.parameters(), lr=lr, lr_decay=lr_decay)
    t = (trainer_cls or trainer.Trainer)(model=model, loss_fn=loss_fn, optimizer=optimizer, train_loader=train_loader,
                                         eval_loader=test_loader, log_dir=log_dir, n_gpus=n_gpus, device_id=device_id)
    t.interleaved_train_and_eval(n_epochs)
    return t


def binarized_mnist(batch_size):
    return datasets.get_mnist_loaders(batch_size, dynamically_binarize=True)


def dequantized_mnist(batch_size):
    return datasets.get_mnist_loaders(batch_size, dequantize=True)


def grey_mnist(batch_size):
    """MNIST at its 256 grey levels / 255, for `categorical_loss(256)`."""
    return datasets.get_mnist_loaders(batch_size)


def binarized_mnist_32(batch_size):
    return datasets.get_mnist_loaders(batch_size, dynamically_binarize=True, resize_to_32=True)


def cifar10(batch_size):
    return datasets.get_cifar10_loaders(batch_size, normalize=True)


def vq_loss(vq_weight):
    """loss_fn of the VQ-VAE recipes (vq_vae.py:127-136, vq_vae_2.py:160-169):
    {"vq_loss", "reconstruction_loss", "loss" = MSE + vq_weight * quantization loss}."""
    from pytorch_generative_amd.nn import utils as nn_utils

    def loss_fn(x, _, preds):
        recon, quantization_loss = preds
        recon_loss = nn_utils.mse_loss(recon, x)
        return {"vq_loss": quantization_loss, "reconstruction_loss": recon_loss,
                "loss": recon_loss + vq_weight * quantization_loss}

    return loss_fn


class _CodeLoader:
    """A loader whose (x, y) batches become (vqvae.encode_codes(x), y): the training data of a prior over the codes."""

    def __init__(self, vqvae, loader):
        self._vqvae, self._loader = vqvae, loader

    def __len__(self):
        return len(self._loader)

    def __iter__(self):
        vqvae = self._vqvae
        device = vqvae.device
        for x, y in self._loader:
            was_training = vqvae.training
            vqvae.eval()  # frozen
            try:
                codes = vqvae.encode_codes(x.to(device))
            finally:
                vqvae.train(was_training)
            yield codes, y


def code_loaders(vqvae, loaders):
    """Wraps a tuple of loaders (train, eval): each batch (x, y) becomes (vqvae.encode_codes(x), y), encoded by the frozen
    VQ-VAE in eval mode on its device — code images (N, 1, h, w) at the levels j / (n_embeddings - 1), the input of a model
    with `input_codes` and the target of `categorical_loss`."""
    return tuple(_CodeLoader(vqvae, loader) for loader in loaders)


class _CodeLoader2:
    """A loader whose (x, y) batches become a level of vqvae2.encode_codes(x): "top" -> (top, y), "bottom" -> (bottom, top),
    the training data of the two priors of a VQ-VAE-2 (the second is trained by trainer.ConditionalTrainer)."""

    def __init__(self, vqvae2, loader, level):
        if level not in ("top", "bottom"):
            raise ValueError(f"code_loaders_2: level {level!r} is neither 'top' nor 'bottom'")
        self._vqvae, self._loader, self._level = vqvae2, loader, level

    def __len__(self):
        return len(self._loader)

    def __iter__(self):
        vqvae = self._vqvae
        device = vqvae.device
        for x, y in self._loader:
            was_training = vqvae.training
            vqvae.eval()  # frozen
            try:
                top, bottom = vqvae.encode_codes(x.to(device))
            finally:
                vqvae.train(was_training)
            yield (top, y) if self._level == "top" else (bottom, top)


def code_loaders_2(vqvae2, loaders, level):
    """code_loaders for a two-level VQ-VAE: level "top" yields (top codes, y), level "bottom" yields (bottom codes, top
    codes) — the input and the context of the conditional prior."""
    return tuple(_CodeLoader2(vqvae2, loader, level) for loader in loaders)
