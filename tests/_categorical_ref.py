"""Plain-torch float64 restatement of the categorical pixel likelihood (csrc/categorical.hip): the per-image negative
log-likelihood, its gradient by autograd, and the inverse-CDF pick exactly as the kernel's contract defines it.

Layout: logits (N, K * C, H, W) read as (N, K, C, H, W) (class-major); images (N, C, H, W) at the levels j / (K - 1)."""

import torch
import torch.nn.functional as F


def levels(k):
    """The K intensity levels as the data holds them: fp32 j / (K - 1)."""
    return torch.arange(k, dtype=torch.float32) / (k - 1)


def classes(images, k):
    """t = clamp(rint(x * (K - 1)), 0, K - 1) in fp32, as the kernels decode a target."""
    return torch.clamp(torch.round(images.float() * float(k - 1)), 0, k - 1).long()


def lse(logits, k):
    """(N, C, H, W) float64 logsumexp over the classes."""
    n, kc, h, w = logits.shape
    return torch.logsumexp(logits.double().view(n, k, kc // k, h, w), dim=1)


def nll_per_sample(logits, images, k):
    """(N,) float64 nats: F.cross_entropy(reduction='none') summed per image. Differentiable in `logits` if it is float64."""
    n, kc, h, w = logits.shape
    ce = F.cross_entropy(logits.double().view(n, k, kc // k, h, w), classes(images, k), reduction="none")
    return ce.sum(dim=(1, 2, 3))


def loss_and_grad(logits, images, k, grad_output=1.0):
    """Scalar loss (sum over sub-pixels, mean over the batch) and grad_output * d loss / d logits, both float64."""
    z = logits.detach().double().requires_grad_(True)
    loss = nll_per_sample(z, images, k).mean()
    (loss * grad_output).backward()
    return loss.detach(), z.grad


def cdf(logits, k, temperature=1.0):
    """logits (N, K * C) of one position -> the float64 running sums (N, C, K) of e_k = exp((z_k - max) / T) and their
    totals (N, C). The division by the temperature is the kernel's multiplication by the fp32 value of 1 / T."""
    n, kc = logits.shape
    z = logits.double().view(n, k, kc // k).permute(0, 2, 1)  # (N, C, K)
    inv_t = float(torch.tensor(1.0 / float(temperature), dtype=torch.float32))
    e = torch.exp((z - z.max(dim=2, keepdim=True).values) * inv_t)
    run = torch.cumsum(e, dim=2)
    return run, run[:, :, -1]


def pick(logits, uniforms, k, temperature=1.0):
    """(N, C) int64: the first class whose inclusive running sum exceeds u * total strictly, the last class if none."""
    run, total = cdf(logits, k, temperature)
    over = run > (uniforms.double() * total).unsqueeze(2)
    first = torch.argmax(over.to(torch.int8), dim=2)  # argmax returns the first maximum
    return torch.where(over.any(dim=2), first, torch.full_like(first, k - 1))


def to_level(cls, k):
    """The fp32 output of a draw: class / (K - 1)."""
    return cls.float() / float(k - 1)
