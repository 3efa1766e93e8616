"""Float64 restatement of one pixel's draw from the discretized logistic mixture, GIVEN the uniforms (test infrastructure).

The arithmetic of PixelCNNpp.sample_from_mixture (Salimans et al. 2017, sections 2.1-2.2): component by Gumbel-max over the K
logits, a logistic variate by inverse CDF per sub-pixel, log-scale floor -7, tanh of the coefficients, G and B shifted by the
drawn R / G, every value clamped to [-1, 1]. tests/test_pcnnpp_rows_cpu.py pins it against that method (torch.rand_like
patched to hand out the same uniforms) and at hand-built cases; tests/test_gpu_pcnnpp_sampling.py holds ops.dmol_sample to it.

The uniforms are clamped to [1e-5, 1 - 1e-5] in THEIR OWN dtype, as torch.rand_like(...).clamp_ does, and only then widened:
for float32 uniforms the bounds are the float32 roundings, which matters at the upper clamp, where log1p(-v) reads 1 - v."""

import torch

NEAR_TIE = 1e-4  # float64 gap of the two largest perturbed logits below which fp32 may pick the other component
# the GPU kernel test's cases: seed per K, batch sizes, and the first / an interior / the last position of its 4 x 8 image
KERNEL_SEEDS = {1: 101, 5: 105, 10: 110, 17: 117, 32: 132}  # 17 / 32: past lane 16 of the argmax butterfly, and its bound
KERNEL_BATCHES = (1, 3, 64, 65)
KERNEL_POSITIONS = ((0, 0), (1, 5), (3, 7))


def draw(params, u_mix, u_pix, n_mix):
    """params (N, 10 K), u_mix (N, K), u_pix (N, 3) -> (x (N, 3) float64 in [-1, 1], gap (N,) float64: the difference of the
    two largest Gumbel-perturbed logits, +inf for K = 1)."""
    n, k = params.shape[0], int(n_mix)
    p = params.double()
    u = u_mix.clone().clamp_(1e-5, 1.0 - 1e-5).double()
    v = u_pix.clone().clamp_(1e-5, 1.0 - 1e-5).double()
    pert = p[:, :k] - torch.log(-torch.log(u))
    top = pert.topk(min(2, k), dim=1).values
    gap = top[:, 0] - top[:, 1] if k > 1 else torch.full((n,), float("inf"), dtype=torch.float64)
    sel = pert.argmax(dim=1)
    rest = p[:, k:].reshape(n, 3, 3, k)  # (sub-pixel, field: mean / log-scale / coefficient, component)
    chosen = rest.gather(3, sel.view(n, 1, 1, 1).expand(n, 3, 3, 1)).squeeze(3)  # (N, 3, 3)
    means, log_scales, coeffs = chosen[:, :, 0], chosen[:, :, 1].clamp(min=-7.0), torch.tanh(chosen[:, :, 2])
    x = means + torch.exp(log_scales) * (torch.log(v) - torch.log1p(-v))
    x0 = x[:, 0].clamp(-1.0, 1.0)
    x1 = (x[:, 1] + coeffs[:, 0] * x0).clamp(-1.0, 1.0)
    x2 = (x[:, 2] + coeffs[:, 1] * x0 + coeffs[:, 2] * x1).clamp(-1.0, 1.0)
    return torch.stack((x0, x1, x2), dim=1), gap


def kernel_case(seed, n, k, h=4, w=8):
    """The fixed-seed inputs of the GPU kernel test (float32, CPU): row parameters (N, 10 K, 1, W) with logits ~ 2 N(0, 1),
    means uniform in [-2, 2], log-scales uniform in [-8, 1] (so that the floor at -7 is crossed), coefficients ~ N(0, 1);
    uniforms (H W, N, K + 3); a canvas in [-1, 1] and a mask with about a quarter of the entries known."""
    g = torch.Generator().manual_seed(seed)
    logits = 2.0 * torch.randn(n, k, 1, w, generator=g)
    sub = torch.empty(n, 3, 3, k, 1, w)
    sub[:, :, 0] = torch.rand(n, 3, k, 1, w, generator=g) * 4.0 - 2.0
    sub[:, :, 1] = torch.rand(n, 3, k, 1, w, generator=g) * 9.0 - 8.0
    sub[:, :, 2] = torch.randn(n, 3, k, 1, w, generator=g)
    params = torch.cat((logits, sub.reshape(n, 9 * k, 1, w)), dim=1).contiguous()
    uniforms = torch.rand(h * w, n, k + 3, generator=g)
    canvas = torch.rand(n, 3, h, w, generator=g) * 2.0 - 1.0
    unknown = torch.rand(n, 3, h, w, generator=g) < 0.75
    return params, uniforms, canvas, unknown


def apply(params, uniforms, canvas, unknown, k, r, c):
    """What one call of the kernel at pixel (r, c) must leave behind: (canvas (N, 3, H, W) float64, gap (N,))."""
    w = canvas.shape[3]
    u = uniforms[r * w + c]
    x, gap = draw(params[:, :, 0, c], u[:, :k], u[:, k:], k)
    out = canvas.double().clone()
    out[:, :, r, c] = torch.where(unknown[:, :, r, c], x, out[:, :, r, c])
    return out, gap
