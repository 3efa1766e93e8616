"""VectorQuantizer on the HIP operator path (reference nn/utils.py:16-96) — SURVEY.md §8(f) rank 4.

Same constructor signature and the same state_dict in both codebook modes: with `use_ema=True` (the default, what
the VQ-VAE models use) the buffers `_embedding`, `_cluster_size`, `_embedding_avg` and the EMA update inside a
training forward; with `use_ema=False` the single parameter `_embedding`, trained by gradient descent on the embedding
loss, which forward adds to the commitment loss. Any `embedding_dim >= 1`.
Kernels: csrc/vq.hip (assignment for widths up to 64 with one position per thread, EMA update, straight-through
backward, MSE loss) and csrc/vq_mfma.hip (assignment for wider codes as a tiled fp32-MFMA distance GEMM with a running
argmin; the codebook gradient as a one-hot GEMM over position ranges merged in a fixed order: no float atomics,
bit-reproducible). Both assignments use the reference's distance form and first-minimum rule. The EMA path at widths
up to 64 is validated on MI355X against outputs of the reference (tests/golden/vq_*.pt, tests/test_gpu_f4.py); the
gradient mode and the wide codes are checked by tests/test_gpu_vq_codebook.py against tests/golden/vq_wide/, which had
not yet run on hardware when this was written, and tools/vq_bench.py (-> profiles/vq.json) had not been measured either.
`ReZeroWrapper` (nn/utils.py:7-13) is not provided: the reference's cannot be constructed.
"""

import torch
from torch import nn
from torch.nn import init

from pytorch_generative_amd import _lib, ops


TILED_MIN_DIM = 65  # embedding widths from here on take pg_vq_assign_tiled; narrower ones stay on pg_vq_assign (profiles/vq.json)


class _VectorQuantize(torch.autograd.Function):
    """EMA mode: `embedding` is a buffer that the forward updates in place when training. Gradient mode (`use_ema`
    false): `embedding` is the parameter, nothing is updated, the loss is commitment + embedding loss (two equal values)
    and the backward adds the codebook gradient (pg_vq_codebook_grad), into `sink` when the parameter has one."""

    @staticmethod
    def forward(ctx, x, embedding, cluster_size, embedding_avg, decay, training, use_ema, sink):
        lib = _lib.load()
        x = ops._chk(x, "vq.x")
        embedding = ops._chk(embedding, "vq.embedding")
        n, d, h, w = x.shape
        k = embedding.shape[0]
        L = h * w
        idx = torch.empty(n * L, device=x.device, dtype=torch.int32)
        q = torch.empty_like(x)
        st = torch.empty_like(x)
        loss = torch.zeros(1, device=x.device, dtype=torch.float32)
        assign, name = (lib.pg_vq_assign_tiled, "pg_vq_assign_tiled") if d >= TILED_MIN_DIM else \
            (lib.pg_vq_assign, "pg_vq_assign")
        _lib.check(assign(x.data_ptr(), embedding.data_ptr(), idx.data_ptr(), q.data_ptr(), st.data_ptr(),
                          loss.data_ptr(), n, d, L, k, ops._stream()), name)
        if use_ema and training:  # EMA codebook update, in place on the buffers like the reference's .data updates
            count = torch.empty(k, device=x.device, dtype=torch.float32)
            total = torch.empty(k * d, device=x.device, dtype=torch.float32)
            _lib.check(lib.pg_vq_ema_update(x.data_ptr(), idx.data_ptr(), cluster_size.data_ptr(),
                                            embedding_avg.data_ptr(), embedding.data_ptr(), count.data_ptr(),
                                            total.data_ptr(), n, d, L, k, float(decay), ops._stream()),
                       "pg_vq_ema_update")
        if not use_ema:  # + mse(q, x.detach()): the same squares, so the same fp32 value once more (nn/utils.py:93)
            both = torch.empty_like(loss)
            _lib.check(lib.pg_add(loss.data_ptr(), loss.data_ptr(), both.data_ptr(), 1, ops._stream()), "pg_add")
            loss = both
        ctx.use_ema, ctx.sink, ctx.k = use_ema, sink, k
        ctx.save_for_backward(x, q, idx)
        ctx.mark_non_differentiable(idx)
        return st, loss.view(()), idx

    @staticmethod
    def backward(ctx, d_st, d_loss, _d_idx):
        lib = _lib.load()
        x, q, idx = ctx.saved_tensors
        d_st = ops._chk(d_st, "vq.d_quantized")
        g = ops._chk(d_loss.reshape(1), "vq.d_loss")
        dx = None
        if ctx.needs_input_grad[0]:
            dx = torch.empty_like(x)
            _lib.check(lib.pg_vq_bwd(x.data_ptr(), q.data_ptr(), d_st.data_ptr(), g.data_ptr(), dx.data_ptr(),
                                     x.numel(), ops._stream()), "pg_vq_bwd")
        d_emb = None
        if not ctx.use_ema and ctx.needs_input_grad[1]:
            n, d, h, w = x.shape
            floats = lib.pg_vq_codebook_grad_workspace_floats(n, d, h * w, ctx.k)
            ws = torch.empty(max(floats, 1), device=x.device, dtype=torch.float32)
            out = ctx.sink
            if out is None:
                out = d_emb = torch.empty((ctx.k, d), device=x.device, dtype=torch.float32)
            _lib.check(lib.pg_vq_codebook_grad(x.data_ptr(), q.data_ptr(), idx.data_ptr(), g.data_ptr(), out.data_ptr(),
                                               0 if ctx.sink is None else 1, n, d, h * w, ctx.k, ws.data_ptr(), floats,
                                               ops._stream()), "pg_vq_codebook_grad")
        return dx, d_emb, None, None, None, None, None, None


class _MSE(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, b):
        lib = _lib.load()
        a = ops._chk(a, "mse.a")
        b = ops._chk(b, "mse.b")
        if a.shape != b.shape:
            raise ValueError("mse_loss: shape mismatch")
        loss = torch.zeros(1, device=a.device, dtype=torch.float32)
        _lib.check(lib.pg_mse_fwd(a.data_ptr(), b.data_ptr(), loss.data_ptr(), a.numel(), ops._stream()),
                   "pg_mse_fwd")
        ctx.save_for_backward(a, b)
        return loss.view(())

    @staticmethod
    def backward(ctx, g):
        lib = _lib.load()
        a, b = ctx.saved_tensors
        g = ops._chk(g.reshape(1), "mse.grad")
        da = torch.empty_like(a) if ctx.needs_input_grad[0] else None
        db = torch.empty_like(b) if ctx.needs_input_grad[1] else None
        _lib.check(lib.pg_mse_bwd(a.data_ptr(), b.data_ptr(), g.data_ptr(),
                                  da.data_ptr() if da is not None else 0,
                                  db.data_ptr() if db is not None else 0, a.numel(), ops._stream()),
                   "pg_mse_bwd")
        return da, db


def mse_loss(a, b):
    """F.mse_loss(a, b) (mean over every element), gradients to both arguments."""
    return _MSE.apply(a, b)


class VectorQuantizer(nn.Module):
    """nn/utils.py:16-96. forward(x) -> (quantized with the straight-through gradient, loss): the commitment loss with
    the EMA codebook, commitment + embedding loss (training and eval) with the gradient-trained one."""

    def __init__(self, n_embeddings, embedding_dim, use_ema=True, ema_decay=0.99):
        super().__init__()
        self.n_embeddings = n_embeddings
        self.embedding_dim = embedding_dim
        self._use_ema = use_ema
        self._decay = ema_decay
        embedding = torch.zeros(n_embeddings, embedding_dim)
        init.kaiming_uniform_(embedding, nonlinearity="linear")
        if self._use_ema:
            self.register_buffer("_embedding", embedding)
            self.register_buffer("_cluster_size", torch.zeros(n_embeddings))
            self.register_buffer("_embedding_avg", embedding.clone())
        else:
            self._embedding = nn.Parameter(embedding)
        self.last_indices = None  # (N*H*W,) int32 of the latest forward (extension, for inspection)

    def forward(self, x):
        assert x.shape[1] == self.embedding_dim, "Input channels must equal embedding_dim."
        if self._use_ema:
            st, loss, idx = _VectorQuantize.apply(x, self._embedding, self._cluster_size, self._embedding_avg,
                                                  self._decay, self.training, True, None)
        else:
            st, loss, idx = _VectorQuantize.apply(x, self._embedding, None, None, self._decay, self.training, False,
                                                  ops._sink(self._embedding))
        self.last_indices = idx
        return st, loss


class CategoricalSampler:
    """Draws sub-pixel intensities from K-way softmax logits: the `sample_fn` of an AutoregressiveModel whose output has
    `n_classes * in_channels` channels, class-major (the layout of ops.categorical_nll_sum_mean). Every sampler of the
    package (full forward per pixel, row-cached, ImageGPT's incremental one) calls `sample_fn(logits).view(n, c)` on one
    position's (N, n_classes * C) logits; this returns the (N, C) levels class / (n_classes - 1) in [0, 1], drawn by
    inverse CDF in one kernel launch (ops.categorical_sample) from uniforms of `generator` (None: the device's default).
    temperature divides the logits: below 1 sharpens the distribution.

    `sample(return_logits=True)` of the models stores logits in a canvas-shaped tensor, that is, it assumes
    out_channels == in_channels: it cannot be combined with a categorical head."""

    def __init__(self, n_classes, temperature=1.0, generator=None):
        n_classes = int(n_classes)
        if not 2 <= n_classes <= ops.CATEGORICAL_MAX_CLASSES:
            raise ValueError(f"CategoricalSampler: n_classes = {n_classes} outside 2..{ops.CATEGORICAL_MAX_CLASSES}")
        if not float(temperature) > 0.0:
            raise ValueError(f"CategoricalSampler: temperature {temperature} must be positive")
        self.n_classes, self.temperature, self.generator = n_classes, float(temperature), generator

    def draw(self, logits, uniforms):
        """The draw as a pure function of (N, n_classes * C) logits and (N, C) uniforms in [0, 1)."""
        return ops.categorical_sample(logits, uniforms, self.n_classes, self.temperature)

    def __call__(self, logits):
        if logits.dim() != 2 or logits.shape[1] % self.n_classes:
            raise ValueError(f"CategoricalSampler: expected (N, {self.n_classes} * C) logits, got {tuple(logits.shape)}")
        shape = (logits.shape[0], logits.shape[1] // self.n_classes)
        return self.draw(logits, torch.rand(shape, device=logits.device, generator=self.generator))
