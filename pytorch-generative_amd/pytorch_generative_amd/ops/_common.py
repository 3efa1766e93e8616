"""ops._common — shared helpers: stream / pointer plumbing, activation ids, zero fills, gradient sinks, the row-decode context.

Part of the operator layer (pytorch_generative_amd.ops): HIP kernels behind torch.autograd.Function, called through the C-ABI
with tensor.data_ptr() and the current stream. No CPU / ATen fallback: a missing library, a CPU tensor or an unsupported shape raises."""

import os

import torch

from pytorch_generative_amd import _lib


ACT_NONE, ACT_RELU, ACT_ELU, ACT_GELU = 0, 1, 2, 3
ACT_ELU_OUT = 4  # dgrad epilogue only: derivative of ELU from its output (include/pg_hip.h)
GATE_TANH, GATE_IDENTITY = 0, 1
_ACT_IDS = {None: ACT_NONE, "none": ACT_NONE, "relu": ACT_RELU, "elu": ACT_ELU, "gelu": ACT_GELU}


def _stream():
    return torch.cuda.current_stream().cuda_stream


class RowDecode:
    """Context of row-cached incremental sampling (models/base.py).

    While active, the convolutional models' ordinary forward() is called on ONE image row
    (N, C, 1, W): every layer of these models is row-causal (its output row r depends on input rows
    <= r only), so nn.Conv2d keeps the last k input rows it needs (k = upward reach of its taps) in a
    private band buffer and evaluates only the current row; nn.CausalAttention keeps K / V caches of
    the rows above (ops.attention_row); image_positional_encoding returns the current row of the full-size encoding. `commit`
    marks the pass that runs once a row is final and pushes it into the caches.

    `row_dev` is the row index as an int32 device scalar for the kernels that take it from the device (ops.attention_row,
    ops.row_gather): a row step that uses it instead of `row` is the same sequence of launches for every row, so it can be
    captured into a hipGraph. It is created on first request (on `device`, default the current GPU) and from then on every
    assignment to `row` also fills it — a fill on the current stream, no host synchronisation.

    The caches belong to the layers; a sampler speaks to them through two hooks a caching module may define, called on every
    module of a model: `_row_reset()` drops its caches (drop_caches: before and after a call, and when a capture was refused)
    and `_row_clear()` puts them back to their start-of-image contents WITHOUT reallocating (clear_caches: after the warm-up
    and capture passes pushed rows into buffers whose addresses the graphs now hold). A cache that is never read at rows >=
    the current one (attention's K / V) needs no `_row_clear`."""

    current = None

    @staticmethod
    def _call_hook(model, hook):
        for m in model.modules():
            fn = getattr(m, hook, None)
            if fn is not None:
                fn()

    @staticmethod
    def drop_caches(model):
        RowDecode._call_hook(model, "_row_reset")

    @staticmethod
    def clear_caches(model):
        RowDecode._call_hook(model, "_row_clear")

    def __init__(self, height, device=None):
        self.height, self.commit = int(height), False
        self._device, self._row, self._row_dev = device, 0, None

    @property
    def row(self):
        return self._row

    @row.setter
    def row(self, value):
        self._row = int(value)
        if self._row_dev is not None:
            self._row_dev.fill_(self._row)

    @property
    def row_dev(self):
        if self._row_dev is None:
            if torch.cuda.is_available() and torch.cuda.is_current_stream_capturing():
                raise RuntimeError("RowDecode.row_dev: first requested inside a stream capture (its fill would be replayed)")
            device =self._device if self._device is not None else torch.device("cuda", torch.cuda.current_device())
            self._row_dev = torch.full((1,), self._row, dtype=torch.int32, device=device)
        return self._row_dev

    def __enter__(self):
        RowDecode.current = self
        return self

    def __exit__(self, *exc):
        RowDecode.current = None
        return False


def _chk(t, name):
    if not t.is_cuda:
        raise RuntimeError(
            f"{name}: expected a tensor on the MI355X (cuda) device, got {t.device}; "
            "the HIP operator path has no CPU fallback"
        )
    if t.dtype != torch.float32:
        raise TypeError(f"{name}: expected float32, got {t.dtype}")
    if t.device.index != torch.cuda.current_device():
        # kernels are enqueued on the CURRENT device's stream with raw pointers: a tensor of another
        # GPU would be dereferenced from the wrong device (Trainer / recipes call set_device)
        raise RuntimeError(f"{name}: tensor lives on {t.device} but the current device is "
                           f"cuda:{torch.cuda.current_device()}; call torch.cuda.set_device first")
    return t if t.is_contiguous() else t.contiguous()


def _p(t):
    return 0 if t is None else t.data_ptr()


def zeros(shape, device):
    """torch.zeros(shape, dtype=float32) with the fill done by the library's own kernel (pg_fill): gradient sinks, loss scalars,
    KL accumulators — no ATen fill kernel inside a captured step."""
    t = torch.empty(shape, device=device, dtype=torch.float32)
    if t.numel():
        _lib.check(_lib.load().pg_fill(t.data_ptr(), 0.0, t.numel(), _stream()), "pg_fill")
    return t


def zeros_like(t):
    return zeros(tuple(t.shape), t.device)


def _sink(param):
    """Returns the direct gradient sink of a parameter (or None)."""
    return getattr(param, "_pg_grad", None) if param is not None else None


def _grad_targets(params, sinks=None):
    """Per parameter: (tensor the kernel adds into, value to return to autograd): the direct sink if
    the parameter has one (then autograd gets None), else a fresh zero tensor. `sinks`: the sinks, one per parameter,
    where the caller resolved them already (the tensor it holds is a view of the parameter that carries the sink)."""
    tgt, ret = [], []
    for p, sink in zip(params, map(_sink, params) if sinks is None else sinks):
        if sink is not None:
            tgt.append(sink)
            ret.append(None)
        else:
            z = zeros_like(p)
            tgt.append(z)
            ret.append(z)
    return tgt, ret


CONV_FMT_F32, CONV_FMT_B3, CONV_FMT_B3_GATE = 1, 2, 3  # include/pg_hip.h PG_CONV_FMT_*
FUSE_SKIP = os.environ.get("PG_FUSE_SKIP", "1") != "0"  # A/B: 0 = plain fan-out, autograd sums the gradients


def _dense_per_image(t):
    """True if every image of the (N, C, H, W) tensor is a dense (C, H, W) block and the data is fp32 on
    the GPU: the batch stride may be larger than C*H*W (a channel slice of a wider tensor)."""
    if not (t.is_cuda and t.dtype == torch.float32 and t.dim() == 4):
        return False
    _, c, h, w = t.shape
    st = t.stride()
    return st[3] == 1 and st[2] == w and st[1] == h * w and st[0] >= c * h * w and t.data_ptr() % 16 == 0
