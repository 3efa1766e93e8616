"""ops.linear_categorical — the model's last 1x1 convolution fused into the K-way softmax likelihood (linear_categorical.hip):
the (N, K C, H, W) logits and their gradient are never written.

Part of the operator layer (pytorch_generative_amd.ops): HIP kernels behind torch.autograd.Function, called through the C-ABI
with tensor.data_ptr() and the current stream. A model with `defer_head = True` returns a DeferredLogits instead of running its
last convolution; ops.categorical_nll_sum_mean / _per_sample take it in place of the logits. Where the fused kernels do not
cover the head, the same functions run `.dense()` and the dense loss kernels: that is the model's own unfused path, not an
ATen fallback."""

import ctypes

import torch

from pytorch_generative_amd import _lib
from pytorch_generative_amd.ops._common import RowDecode, _chk, _grad_targets, _p, _stream, zeros
from pytorch_generative_amd.ops.gpt_ends import gpt_out_head_supported

TRANSFORM_NONE, TRANSFORM_RELU, TRANSFORM_LN = 0, 1, 2  # include/pg_hip.h PG_LC_*
MAX_CLASSES = 4096


class DeferredLogits:
    """The logits conv(transform(features)) of a K-way softmax head, not yet computed. A plain object, not a tensor.

    features (N, Cin, H, W); conv: the model's last 1x1 convolution; in_act="relu" or pre_ln=<NCHWLayerNorm>: what the model
    applies to the features in front of it (at most one of the two)."""

    def __init__(self, features, conv, *, in_act=None, pre_ln=None):
        if in_act is not None and pre_ln is not None:
            raise ValueError("DeferredLogits: in_act and pre_ln exclude each other")
        if features.dim() != 4 or features.shape[1] != conv.in_channels:
            raise ValueError(f"DeferredLogits: features {tuple(features.shape)} do not feed a convolution of "
                             f"{conv.in_channels} input channels")
        self.features, self.conv, self.in_act, self.pre_ln = features, conv, in_act, pre_ln

    @property
    def shape(self):
        n, _, h, w = self.features.shape
        return torch.Size((n, self.conv.out_channels, h, w))

    def dense(self):
        """Exactly what the model returns without deferral."""
        if self.in_act is not None:
            return self.conv(self.features, in_act=self.in_act)
        if self.pre_ln is not None:
            if gpt_out_head_supported(self.features, self.pre_ln, self.conv):
                return self.conv(self.features, pre_ln=self.pre_ln)
            return self.conv(self.pre_ln(self.features))
        return self.conv(self.features)


def _transform(in_act, pre_ln):
    if pre_ln is not None:
        return TRANSFORM_LN
    return TRANSFORM_RELU if in_act == "relu" else TRANSFORM_NONE


def linear_categorical_supported(features, conv, in_act=None, pre_ln=None):
    """True where the fused kernels cover the head: a 1x1 Conv2d of the project (stride 1, no padding), float32 features and
    parameters on the current device, Cin a multiple of 4 in 4..256, in_act None / "relu" or an affine LayerNorm over the Cin
    channels, 16-byte aligned weights, and no open RowDecode. (The class count is the loss function's: it checks 2..4096.)"""
    if RowDecode.current is not None or type(conv).__name__ != "Conv2d" or not hasattr(conv, "_conv_spec"):
        return False
    if not (torch.is_tensor(features) and features.is_cuda and features.dtype == torch.float32 and features.dim() == 4
            and features.device.index == torch.cuda.current_device()):
        return False
    cin = features.shape[1]
    if cin % 4 or not 4 <= cin <= 256 or tuple(conv.weight.shape[1:]) != (cin, 1, 1) or getattr(conv, "_down2", False):
        return False
    pad = conv.padding if isinstance(conv.padding, tuple) else (conv.padding, conv.padding)
    if tuple(pad) != (0, 0) or (in_act is not None and pre_ln is not None) or in_act not in (None, "relu"):
        return False
    tensors = [conv.weight] + ([conv.bias] if conv.bias is not None else [])
    if pre_ln is not None:
        if (not isinstance(pre_ln, torch.nn.LayerNorm) or tuple(pre_ln.normalized_shape) != (cin,)
                or not pre_ln.elementwise_affine or pre_ln.bias is None):
            return False
        tensors += [pre_ln.weight, pre_ln.bias]
    return all(t.is_cuda and t.dtype == torch.float32 and t.device == features.device and t.is_contiguous()
               and t.data_ptr() % 16 == 0 for t in tensors)


def _plan(lib, n, c, k, cin, hw, transform):
    """(rows, workspace floats) of the launches, None outside the kernels' domain."""
    ppt, rows, lds = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)
    ws = ctypes.c_size_t(0)
    rc = lib.pg_linear_categorical_plan(n, c, k, cin, hw, transform, ctypes.byref(ppt), ctypes.byref(rows), ctypes.byref(lds),
                                        ctypes.byref(ws))
    return None if rc else (rows.value, ws.value)


def _dims(deferred, images, n_classes, what):
    k = int(n_classes)
    if not 2 <= k <= MAX_CLASSES:
        raise ValueError(f"{what}: n_classes = {k} outside 2..{MAX_CLASSES}")
    if images.dim() != 4:
        raise ValueError(f"{what}: expected (N, C, H, W) images")
    n, c, h, w = images.shape
    if tuple(deferred.shape) != (n, k * c, h, w):
        raise ValueError(f"{what}: logits {tuple(deferred.shape)} != {(n, k * c, h, w)} for images {tuple(images.shape)} "
                         f"and {k} classes")
    return n, c, k, h * w


class _LinearCategoricalNLL(torch.autograd.Function):
    """loss = categorical_nll(conv1x1(transform(h))). Saves h, the images and the two lse planes; backward recomputes the logits."""

    @staticmethod
    def forward(ctx, h, weight, bias, lnw, lnb, images, dims, transform, eps, params):
        lib = _lib.load()
        h = _chk(h, "linear_categorical.features")
        images = _chk(images, "linear_categorical.images")
        n, c, k, hw = dims
        cin = h.shape[1]
        loss = zeros((1,), h.device)
        lse = torch.empty((2,) + tuple(images.shape), device=h.device, dtype=torch.float32)  # lse | its rounding residual
        _lib.check(lib.pg_linear_categorical_nll_fwd(h.data_ptr(), weight.data_ptr(), _p(bias), _p(lnw), _p(lnb), eps,
                                                     images.data_ptr(), lse.data_ptr(), None, loss.data_ptr(), n, c, k, cin, hw,
                                                     transform, _stream()), "pg_linear_categorical_nll_fwd")
        ctx.save_for_backward(h, images, lse)
        ctx.dims, ctx.transform, ctx.eps, ctx.params = dims, transform, eps, params
        return loss.view(())

    @staticmethod
    def backward(ctx, g):
        lib = _lib.load()
        h, images, lse = ctx.saved_tensors
        weight, bias, lnw, lnb = ctx.params
        n, c, k, hw = ctx.dims
        cin = h.shape[1]
        g = _chk(g.reshape(1), "linear_categorical.grad")
        live = [p for p in ctx.params if p is not None]
        tgt, ret = _grad_targets(live)
        tgt = dict(zip(map(id, live), tgt))
        ret = dict(zip(map(id, live), ret))
        rows, ws_n = _plan(lib, n, c, k, cin, hw, ctx.transform)
        ws = torch.empty(ws_n, device=h.device, dtype=torch.float32)
        dh = torch.empty_like(h)
        _lib.check(lib.pg_linear_categorical_nll_bwd(h.data_ptr(), weight.data_ptr(), _p(bias), _p(lnw), _p(lnb), ctx.eps,
                                                     images.data_ptr(), lse.data_ptr(), g.data_ptr(), dh.data_ptr(), n, c, k, cin,
                                                     hw, ctx.transform, ws.data_ptr(), ws_n, _stream()),
                   "pg_linear_categorical_nll_bwd")
        _lib.check(lib.pg_linear_categorical_reduce(ws.data_ptr(), rows, k * c, cin, ctx.transform, tgt[id(weight)].data_ptr(),
                                                    _p(tgt.get(id(bias))), _p(tgt.get(id(lnw))), _p(tgt.get(id(lnb))),
                                                    _stream()), "pg_linear_categorical_reduce")
        return (dh,) + tuple(ret.get(id(p)) if p is not None else None for p in ctx.params) + (None,) * 5


def _operands(deferred):
    conv, ln = deferred.conv, deferred.pre_ln
    transform = _transform(deferred.in_act, ln)
    weight = conv.weight
    params = (weight, conv.bias, ln.weight if ln is not None else None, ln.bias if ln is not None else None)
    return transform, float(ln.eps) if ln is not None else 0.0, params


def fused_route(deferred, images, n_classes, what="categorical_nll"):
    """(n, c, k, hw) if the loss of `deferred` runs on the fused kernels, else None (the caller takes .dense())."""
    dims = _dims(deferred, images, n_classes, what)
    if not linear_categorical_supported(deferred.features, deferred.conv, deferred.in_act, deferred.pre_ln):
        return None
    n, c, k, hw = dims
    if _plan(_lib.load(), n, c, k, deferred.features.shape[1], hw, _transform(deferred.in_act, deferred.pre_ln)) is None:
        return None
    return dims


def linear_categorical_nll_sum_mean(deferred, images, dims):
    transform, eps, params = _operands(deferred)
    weight, bias, lnw, lnb = params
    return _LinearCategoricalNLL.apply(deferred.features, weight, bias, lnw, lnb, images, dims, transform, eps, params)


@torch.no_grad()
def linear_categorical_nll_per_sample(deferred, images, dims):
    lib = _lib.load()
    transform, eps, (weight, bias, lnw, lnb) = _operands(deferred)
    h = _chk(deferred.features, "linear_categorical.features")
    images = _chk(images, "linear_categorical.images")
    n, c, k, hw = dims
    loss = zeros((1,), h.device)
    lse = torch.empty((3,) + tuple(images.shape), device=h.device, dtype=torch.float32)  # lse | residual | lse - z_t
    per_sample = torch.empty(n, device=h.device, dtype=torch.float32)
    _lib.check(lib.pg_linear_categorical_nll_fwd(h.data_ptr(), weight.data_ptr(), _p(bias), _p(lnw), _p(lnb), eps,
                                                 images.data_ptr(), lse.data_ptr(), per_sample.data_ptr(), loss.data_ptr(), n, c, k,
                                                 h.shape[1], hw, transform, _stream()), "pg_linear_categorical_nll_fwd")
    return per_sample
