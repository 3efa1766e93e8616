"""ops.losses — BCE-with-logits, discretized mixture of logistics, ELBO terms.

Part of the operator layer (pytorch_generative_amd.ops): HIP kernels behind torch.autograd.Function, called through the C-ABI
with tensor.data_ptr() and the current stream. No CPU / ATen fallback: a missing library, a CPU tensor or an unsupported shape raises."""

import torch

from pytorch_generative_amd import _lib
from pytorch_generative_amd.ops import linear_categorical
from pytorch_generative_amd.ops._common import _chk, _stream, zeros


# --------------------------------------------------------------------------------------------
# loss
# --------------------------------------------------------------------------------------------
class _BCEWithLogitsSumMean(torch.autograd.Function):
    @staticmethod
    def forward(ctx, z, x):
        lib = _lib.load()
        z = _chk(z, "bce.logits")
        x = _chk(x, "bce.targets")
        if z.numel() != x.numel():
            raise ValueError("bce: logits/targets size mismatch")
        n = z.shape[0]
        loss = zeros((1,), z.device)
        _lib.check(lib.pg_bce_logits_fwd(z.data_ptr(), x.data_ptr(), loss.data_ptr(), n,
                                         z.numel() // n, _stream()), "pg_bce_logits_fwd")
        ctx.save_for_backward(z, x)
        return loss.view(())

    @staticmethod
    def backward(ctx, g):
        lib = _lib.load()
        z, x = ctx.saved_tensors
        g = _chk(g.reshape(1), "bce.grad")
        n = z.shape[0]
        dz = torch.empty_like(z)
        _lib.check(lib.pg_bce_logits_bwd(z.data_ptr(), x.data_ptr(), g.data_ptr(), dz.data_ptr(), n,
                                         z.numel() // n, _stream()), "pg_bce_logits_bwd")
        return dz, None


class _DmolLossSumMean(torch.autograd.Function):
    @staticmethod
    def forward(ctx, l, x, n_mix):
        lib = _lib.load()
        l = _chk(l, "dmol.params")
        x = _chk(x, "dmol.images")
        n, c, h, w = l.shape
        if c != 10 * n_mix or tuple(x.shape) != (n, 3, h, w):
            raise ValueError("dmol: expected (N, 10 * n_mix, H, W) parameters and (N, 3, H, W) images in [-1, 1]")
        loss = zeros((1,), l.device)
        _lib.check(lib.pg_dmol_fwd(l.data_ptr(), x.data_ptr(), loss.data_ptr(), n, n_mix, h * w, _stream()),
                   "pg_dmol_fwd")
        ctx.save_for_backward(l, x)
        ctx.n_mix = n_mix
        return loss.view(())

    @staticmethod
    def backward(ctx, g):
        lib = _lib.load()
        l, x = ctx.saved_tensors
        g = _chk(g.reshape(1), "dmol.grad")
        n, _, h, w = l.shape
        dl = torch.empty_like(l)
        _lib.check(lib.pg_dmol_bwd(l.data_ptr(), x.data_ptr(), g.data_ptr(), dl.data_ptr(), n, ctx.n_mix, h * w,
                                   _stream()), "pg_dmol_bwd")
        return dl, None, None


def dmol_loss_sum_mean(params, images, n_mix=10):
    """Discretized mixture-of-logistics negative log-likelihood (PixelCNN++, Salimans et al. 2017), nats,
    summed over pixels and averaged over the batch. params (N, 10 * n_mix, H, W), images (N, 3, H, W) in
    [-1, 1]. Not in the reference (BASELINE.json configs[2] names it): parity is against oracle/dmol.py."""
    return _DmolLossSumMean.apply(params, images, int(n_mix))


DMOL_SAMPLE_MAX_K = 32  # include/pg_hip.h PG_DMOL_SAMPLE_MAX_K


def dmol_sample(params, uniforms, canvas, unknown, n_mix, row=0, col=0, *, row_buf=None, pos_dev=None):
    """Draws pixel (row, col) of every image from its logistic mixture, in one launch (pg_dmol_sample): the arithmetic of
    PixelCNNpp.sample_from_mixture followed by where(unknown, drawn, canvas), in place.

    params (N, 10 * n_mix, 1, W): the mixture parameters of image row `row` (any strides; column `col` is read);
    uniforms (H * W, N, n_mix + 3) in [0, 1): raster position row * W + col is read; canvas (N, 3, H, W) float32 and
    unknown (N, 3, H, W) bool, both contiguous: canvas[:, :, row, col] is replaced where unknown; row_buf (N, 3, 1, W),
    optional: receives canvas[:, :, row, col] as it stands afterwards. pos_dev (int32 device scalar, optional): the
    raster position is read from it instead of (row, col), so that one captured graph serves every pixel.
    Sampling only: no gradient is defined."""
    lib = _lib.load()
    n, c, one, w = params.shape
    h = canvas.shape[2]
    k = int(n_mix)
    if c != 10 * k or one != 1 or tuple(canvas.shape) != (n, 3, h, w) or tuple(unknown.shape) != (n, 3, h, w):
        raise ValueError("dmol_sample: expected (N, 10 * n_mix, 1, W) parameters, an (N, 3, H, W) canvas and its mask")
    if tuple(uniforms.shape) != (h * w, n, k + 3):
        raise ValueError(f"dmol_sample: uniforms {tuple(uniforms.shape)} != {(h * w, n, k + 3)}")
    for t, name in ((params, "params"), (uniforms, "uniforms"), (canvas, "canvas")) + (
            ((row_buf, "row_buf"),) if row_buf is not None else ()):
        if not t.is_cuda or t.dtype != torch.float32 or t.device != canvas.device:
            raise RuntimeError(f"dmol_sample.{name}: expected a float32 tensor on the canvas's MI355X (cuda) device")
    if canvas.device.index != torch.cuda.current_device():
        raise RuntimeError("dmol_sample: the canvas does not live on the current device")
    if unknown.dtype != torch.bool or unknown.device != canvas.device:
        raise TypeError("dmol_sample.unknown: expected a bool tensor on the canvas's device")
    if not (uniforms.is_contiguous() and canvas.is_contiguous() and unknown.is_contiguous()):
        raise ValueError("dmol_sample: uniforms, canvas and unknown must be contiguous (they are updated / indexed in place)")
    if row_buf is not None and (tuple(row_buf.shape) != (n, 3, 1, w) or not row_buf.is_contiguous()):
        raise ValueError("dmol_sample: row_buf must be a contiguous (N, 3, 1, W) tensor")
    if pos_dev is not None and (pos_dev.dtype != torch.int32 or pos_dev.numel() != 1 or pos_dev.device != canvas.device):
        raise TypeError("dmol_sample.pos_dev: expected one int32 on the canvas's device")
    sn, sc, _, sw = params.stride()
    _lib.check(lib.pg_dmol_sample(params.data_ptr(), sn, sc, sw, uniforms.data_ptr(), canvas.data_ptr(),
                                  unknown.data_ptr(), None if row_buf is None else row_buf.data_ptr(), n, k, h, w,
                                  int(row), int(col), None if pos_dev is None else pos_dev.data_ptr(), _stream()),
               "pg_dmol_sample")
    return canvas


def bce_with_logits_sum_mean(logits, targets):
    """F.binary_cross_entropy_with_logits(reduction='none').sum(pixels).mean(batch)
    (reference image_gpt.py:158-162 and every other AR reproduce())."""
    return _BCEWithLogitsSumMean.apply(logits, targets)


CATEGORICAL_MAX_CLASSES = 4096  # csrc/categorical.hip


def _categorical_dims(logits, images, n_classes, what):
    k = int(n_classes)
    if not 2 <= k <= CATEGORICAL_MAX_CLASSES:
        raise ValueError(f"{what}: n_classes = {k} outside 2..{CATEGORICAL_MAX_CLASSES}")
    if logits.dim() != 4 or images.dim() != 4:
        raise ValueError(f"{what}: expected (N, n_classes * C, H, W) logits and (N, C, H, W) images")
    n, c, h, w = images.shape
    if tuple(logits.shape) != (n, k * c, h, w):
        raise ValueError(f"{what}: logits {tuple(logits.shape)} != {(n, k * c, h, w)} for images {tuple(images.shape)} "
                         f"and {k} classes")
    return n, c, k, h * w


class _CategoricalNLLSumMean(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, images, n_classes):
        lib = _lib.load()
        logits = _chk(logits, "categorical.logits")
        images = _chk(images, "categorical.images")
        n, c, k, hw = _categorical_dims(logits, images, n_classes, "categorical_nll")
        loss = zeros((1,), logits.device)
        lse = torch.empty((2,) + tuple(images.shape), device=images.device, dtype=torch.float32)  # lse | its rounding residual
        _lib.check(lib.pg_categorical_nll_fwd(logits.data_ptr(), images.data_ptr(), lse.data_ptr(), None, loss.data_ptr(),
                                              n, c, k, hw, _stream()), "pg_categorical_nll_fwd")
        ctx.save_for_backward(logits, images, lse)
        ctx.dims = (n, c, k, hw)
        return loss.view(())

    @staticmethod
    def backward(ctx, g):
        lib = _lib.load()
        logits, images, lse = ctx.saved_tensors
        g = _chk(g.reshape(1), "categorical.grad")
        n, c, k, hw = ctx.dims
        dlogits = torch.empty_like(logits)
        _lib.check(lib.pg_categorical_nll_bwd(logits.data_ptr(), images.data_ptr(), lse.data_ptr(), g.data_ptr(),
                                              dlogits.data_ptr(), n, c, k, hw, _stream()), "pg_categorical_nll_bwd")
        return dlogits, None, None


def categorical_nll_sum_mean(logits, images, n_classes):
    """K-way softmax negative log-likelihood, nats, summed over sub-pixels and averaged over the batch:
    F.cross_entropy(logits.view(N, K, C, H, W), classes, reduction='none').sum((1, 2, 3)).mean().
    logits (N, n_classes * C, H, W), class-major; images (N, C, H, W) at the levels j / (n_classes - 1), from which the
    class is rint(x * (n_classes - 1)) clamped to the range. The gradient goes to the logits only.
    logits may be an ops.DeferredLogits (a model with defer_head = True): the head's 1x1 convolution then runs inside the loss
    kernels (ops.linear_categorical) where they cover it, and as .dense() in front of this function's kernels where not."""
    if isinstance(logits, linear_categorical.DeferredLogits):
        dims = linear_categorical.fused_route(logits, images, n_classes)
        if dims is not None:
            return linear_categorical.linear_categorical_nll_sum_mean(logits, images, dims)
        logits = logits.dense()
    return _CategoricalNLLSumMean.apply(logits, images, int(n_classes))


@torch.no_grad()
def categorical_nll_per_sample(logits, images, n_classes):
    """The same likelihood per image: (N,) nats, no gradient (evaluation, bits/dim). logits may be an ops.DeferredLogits."""
    if isinstance(logits, linear_categorical.DeferredLogits):
        dims = linear_categorical.fused_route(logits, images, n_classes, "categorical_nll_per_sample")
        if dims is not None:
            return linear_categorical.linear_categorical_nll_per_sample(logits, images, dims)
        logits = logits.dense()
    lib = _lib.load()
    logits = _chk(logits, "categorical.logits")
    images = _chk(images, "categorical.images")
    n, c, k, hw = _categorical_dims(logits, images, n_classes, "categorical_nll_per_sample")
    loss = zeros((1,), logits.device)
    lse = torch.empty((2,) + tuple(images.shape), device=images.device, dtype=torch.float32)  # lse | its rounding residual
    per_sample = torch.empty(n, device=logits.device, dtype=torch.float32)
    _lib.check(lib.pg_categorical_nll_fwd(logits.data_ptr(), images.data_ptr(), lse.data_ptr(), per_sample.data_ptr(),
                                          loss.data_ptr(), n, c, k, hw, _stream()), "pg_categorical_nll_fwd")
    return per_sample


@torch.no_grad()
def categorical_sample(logits, uniforms, n_classes, temperature=1.0):
    """One position's draw from the K-way softmax by inverse CDF, in one launch (pg_categorical_sample).

    logits (N, n_classes * C), class-major, any positive strides (a column of a row step's output goes in without a
    copy); uniforms (N, C) in [0, 1). Returns (N, C) levels class / (n_classes - 1): the first class whose running sum of
    exp((z - max) / temperature) exceeds u times the total. Sampling only: no gradient is defined."""
    lib = _lib.load()
    k = int(n_classes)
    if not 2 <= k <= CATEGORICAL_MAX_CLASSES:
        raise ValueError(f"categorical_sample: n_classes = {k} outside 2..{CATEGORICAL_MAX_CLASSES}")
    if not float(temperature) > 0.0:
        raise ValueError(f"categorical_sample: temperature {temperature} must be positive")
    for t, name in ((logits, "logits"), (uniforms, "uniforms")):
        if not t.is_cuda:
            raise RuntimeError(f"categorical_sample.{name}: expected a tensor on the MI355X (cuda) device, got {t.device}; "
                               "the HIP operator path has no CPU fallback")
        if t.dtype != torch.float32:
            raise TypeError(f"categorical_sample.{name}: expected float32, got {t.dtype}")
        if t.device.index != torch.cuda.current_device():
            raise RuntimeError(f"categorical_sample.{name}: tensor lives on {t.device} but the current device is "
                               f"cuda:{torch.cuda.current_device()}")
    if logits.dim() != 2 or logits.shape[1] % k or uniforms.dim() != 2:
        raise ValueError(f"categorical_sample: expected (N, {k} * C) logits and (N, C) uniforms, got "
                         f"{tuple(logits.shape)} and {tuple(uniforms.shape)}")
    n, c = logits.shape[0], logits.shape[1] // k
    if tuple(uniforms.shape) != (n, c) or n < 1 or c < 1:
        raise ValueError(f"categorical_sample: uniforms {tuple(uniforms.shape)} != {(n, c)}")
    sn, sk = logits.stride()
    if sn <= 0 or sk <= 0:  # an expanded or size-one dimension: the kernel wants real strides
        logits = logits.contiguous()
        sn, sk = logits.stride()
    uniforms = uniforms.contiguous()
    out = torch.empty((n, c), device=logits.device, dtype=torch.float32)
    _lib.check(lib.pg_categorical_sample(logits.data_ptr(), sn, sk, uniforms.data_ptr(), out.data_ptr(), n, c, k,
                                         1.0 / float(temperature), _stream()), "pg_categorical_sample")
    return out


class _ElboMean(torch.autograd.Function):
    """loss = mean_n(recon_n) + mean_n(kl_n) with recon_n the per-sample BCE-with-logits sum."""

    @staticmethod
    def forward(ctx, logits, x, kl):
        lib = _lib.load()
        logits, x, kl = _chk(logits, "elbo.logits"), _chk(x, "elbo.x"), _chk(kl, "elbo.kl")
        n = logits.shape[0]
        recon = zeros((1,), logits.device)
        klm = zeros((1,), logits.device)
        _lib.check(lib.pg_bce_logits_fwd(logits.data_ptr(), x.data_ptr(), recon.data_ptr(), n,
                                         logits.numel() // n, _stream()), "pg_bce_logits_fwd")
        _lib.check(lib.pg_vec_mean_accum(kl.data_ptr(), n, klm.data_ptr(), _stream()),
                   "pg_vec_mean_accum")
        ctx.save_for_backward(logits, x)
        ctx.n = n
        return recon.view(()), klm.view(())

    @staticmethod
    def backward(ctx, g_recon, g_kl):
        lib = _lib.load()
        logits, x = ctx.saved_tensors
        n = ctx.n
        dz = torch.empty_like(logits)
        g_recon = _chk(g_recon.reshape(1), "elbo.g")
        _lib.check(lib.pg_bce_logits_bwd(logits.data_ptr(), x.data_ptr(), g_recon.data_ptr(),
                                         dz.data_ptr(), n, logits.numel() // n, _stream()),
                   "pg_bce_logits_bwd")
        dkl = torch.empty(n, device=logits.device, dtype=torch.float32)
        g_kl = _chk(g_kl.reshape(1), "elbo.gk")
        _lib.check(lib.pg_fill_scaled(g_kl.data_ptr(), 1.0 / n, dkl.data_ptr(), n, _stream()),
                   "pg_fill_scaled")
        return dz, None, dkl


def elbo_terms(logits, x, kl):
    """Returns (recon_loss.mean(), kl_div.mean()) of the reference VAE loss_fn (vae.py:149-159)."""
    return _ElboMean.apply(logits, x, kl)
