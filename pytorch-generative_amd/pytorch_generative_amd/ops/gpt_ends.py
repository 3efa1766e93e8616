"""ops.gpt_ends — ImageGPT's stem (positional add + type A causal 3x3 convolution) and output head (LayerNorm + 1x1
convolution) on the four kernels of gpt_ends.hip.

Part of the operator layer (pytorch_generative_amd.ops): HIP kernels behind torch.autograd.Function, called through the C-ABI
with tensor.data_ptr() and the current stream. No CPU / ATen fallback: a missing library, a CPU tensor or an unsupported shape raises."""

import ctypes
import os

import torch

from pytorch_generative_amd import _lib
from pytorch_generative_amd.ops._common import RowDecode, _chk, _grad_targets, _stream
from pytorch_generative_amd.ops.gpt_block import reduce_rows

FUSE_ENDS = os.environ.get("PG_FUSE_ENDS", "1") != "0"  # A/B: 0 = the generic operators (add, mask, conv_taps, LayerNorm, 1x1)
MAX_OUT_CHANNELS = 4  # csrc/gpt_ends.h MAX_COUT


# --------------------------------------------------------------------------------------------
# stem
# --------------------------------------------------------------------------------------------
def gpt_stem_supported(img, pos, conv):
    """The stem kernels cover the BASELINE.json ImageGPT stem: one input channel, 16 embedding channels, a 3x3 type A
    CausalConv2d with padding 1 and a bias, and an image that needs no gradient."""
    if (not FUSE_ENDS or RowDecode.current is not None or conv.bias is None or not getattr(conv, "_mask_center", False)
            or not hasattr(conv, "mask")):
        return False
    pad = conv.padding if isinstance(conv.padding, tuple) else (conv.padding, conv.padding)
    stride = conv.stride if isinstance(conv.stride, tuple) else (conv.stride, conv.stride)
    return (img.dim() == 4 and img.shape[1] == 1 and tuple(conv.weight.shape) == (16, 1, 3, 3) and tuple(pad) == (1, 1)
            and tuple(stride) == (1, 1) and tuple(pos.shape) == (1, 1, img.shape[2], img.shape[3])
            and not img.requires_grad and img.is_cuda and img.dtype == torch.float32)


class _GPTStem(torch.autograd.Function):
    """x0 = conv_A(img + pos). The forward kernel also zeroes the masked weight entries in place; backward leaves d weight of
    all nine taps (the reference's gradient is not masked), d bias and d pos, and — when the model handed it the block chain —
    flushes every reduction of the step: it is the last backward to run."""

    @staticmethod
    def forward(ctx, img, pos, weight, bias, params, chain, grid_cap):
        lib = _lib.load()
        img = _chk(img, "gpt_stem.img")
        pos, weight, bias = (_chk(t, "gpt_stem.param") for t in (pos, weight, bias))
        n, _, h, w = img.shape
        x0 = torch.empty((n, 16, h, w), device=img.device, dtype=torch.float32)
        _lib.check(lib.pg_gpt_stem_fwd(img.data_ptr(), pos.data_ptr(), weight.data_ptr(), bias.data_ptr(), x0.data_ptr(),
                                       n, h, w, grid_cap, _stream()), "pg_gpt_stem_fwd")
        ctx.save_for_backward(img, pos, weight)
        ctx.params, ctx.chain, ctx.grid_cap = params, chain, grid_cap
        return x0

    @staticmethod
    def backward(ctx, dx0):
        lib = _lib.load()
        img, pos, weight = ctx.saved_tensors
        n, _, h, w = img.shape
        chain = ctx.chain
        try:
            dx0 = _chk(dx0, "gpt_stem.dx0")
            tgt, ret = _grad_targets(ctx.params)  # order: pos, weight, bias
            rows, slices = ctypes.c_int(0), ctypes.c_int(0)
            _lib.check(lib.pg_gpt_stem_bwd_plan(n, h, w, ctx.grid_cap, ctypes.byref(rows), ctypes.byref(slices)),
                       "pg_gpt_stem_bwd_plan")
            ws_n = lib.pg_gpt_stem_bwd_workspace_floats(n, h, w, ctx.grid_cap)
            ws = torch.empty(ws_n, device=img.device, dtype=torch.float32)
            _lib.check(lib.pg_gpt_stem_bwd(dx0.data_ptr(), img.data_ptr(), pos.data_ptr(), weight.data_ptr(), n, h, w,
                                           ctx.grid_cap, ws.data_ptr(), ws_n, _stream()), "pg_gpt_stem_bwd")
            stem = (ws, rows.value, slices.value, h, w, [tgt[1], tgt[2], tgt[0]])
        except BaseException:
            if chain is not None:  # whatever was queued still reaches its destinations
                chain.flush(n, 16, h * w)
            raise
        if chain is not None:
            chain.flush(n, 16, h * w, stem=stem)
        else:
            reduce_rows([], n, 16, h * w, stem=stem)
        return None, ret[0], ret[1], ret[2], None, None, None


def gpt_stem(img, pos, conv, chain=None, grid_cap=0):
    """chain: the model's block chain (ops.new_block_chain) when this stem's backward is to flush it."""
    params = (pos, conv.weight, conv.bias)
    return _GPTStem.apply(img, pos, conv.weight, conv.bias, params, chain, grid_cap)


# --------------------------------------------------------------------------------------------
# output head
# --------------------------------------------------------------------------------------------
def gpt_out_head_supported(x, ln, conv):
    """ImageGPT's head: LayerNorm over 16 channels in front of a 1x1 convolution with a bias and at most 4 output channels."""
    if not FUSE_ENDS or RowDecode.current is not None or conv.bias is None or x.dim() != 4 or x.shape[1] != 16:
        return False
    cout = conv.weight.shape[0]
    return (tuple(conv.weight.shape) == (cout, 16, 1, 1) and 1 <= cout <= MAX_OUT_CHANNELS
            and tuple(ln.normalized_shape) == (16,) and type(conv).__name__ == "Conv2d")


class _GPTOutHead(torch.autograd.Function):
    """logits = conv1x1(LN(x)); the normalised tensor is never stored, backward recomputes the statistics."""

    @staticmethod
    def forward(ctx, x, lnw, lnb, cw, cb, eps, params, chain, grid_cap):
        lib = _lib.load()
        x = _chk(x, "gpt_out_head.x")
        lnw, lnb, cw, cb = (_chk(t, "gpt_out_head.param") for t in (lnw, lnb, cw, cb))
        n, c, h, w = x.shape
        cout = cw.shape[0]
        logits = torch.empty((n, cout, h, w), device=x.device, dtype=torch.float32)
        _lib.check(lib.pg_gpt_out_head_fwd(x.data_ptr(), lnw.data_ptr(), lnb.data_ptr(), cw.data_ptr(), cb.data_ptr(),
                                           logits.data_ptr(), n, c, cout, h * w, eps, grid_cap, _stream()),
                   "pg_gpt_out_head_fwd")
        ctx.save_for_backward(x, lnw, lnb, cw)
        ctx.eps, ctx.params, ctx.chain, ctx.grid_cap = eps, params, chain, grid_cap
        return logits

    @staticmethod
    def backward(ctx, dlogits):
        lib = _lib.load()
        x, lnw, lnb, cw = ctx.saved_tensors
        n, c, h, w = x.shape
        cout, L = cw.shape[0], h * w
        dlogits = _chk(dlogits, "gpt_out_head.dlogits")
        dx = torch.empty_like(x)
        tgt, ret = _grad_targets(ctx.params)  # order: ln.weight, ln.bias, conv.weight, conv.bias
        rows = lib.pg_gpt_out_head_bwd_rows(n, L, ctx.grid_cap)
        ws_n = rows * (32 + 17 * cout)
        ws = torch.empty(ws_n, device=x.device, dtype=torch.float32)
        _lib.check(lib.pg_gpt_out_head_bwd(x.data_ptr(), lnw.data_ptr(), lnb.data_ptr(), cw.data_ptr(),
                                           dlogits.data_ptr(), dx.data_ptr(), n, c, cout, L, ctx.eps, ctx.grid_cap,
                                           ws.data_ptr(), ws_n, _stream()), "pg_gpt_out_head_bwd")
        out = (ws, rows, cout, tgt)
        if ctx.chain is not None and all(r is None for r in ret):
            ctx.chain.out = out  # the stem's backward adds these rows in the step's one reduce launch
        else:
            reduce_rows([], n, c, L, out=out)
        return dx, ret[0], ret[1], ret[2], ret[3], None, None, None, None


def gpt_out_head(x, ln, conv, chain=None, grid_cap=0):
    """chain: only when a stem that flushes it (gpt_stem with the same chain) is part of the same graph."""
    params = (ln.weight, ln.bias, conv.weight, conv.bias)
    return _GPTOutHead.apply(x, *params, float(ln.eps), params, chain, grid_cap)
