"""ops.code_up — upsampling lookup over an image of code indices (csrc/code_up.hip): how an autoregressive model takes a
second, coarser code image as context.

F.conv_transpose2d(one_hot(codes), weight, stride=f) with kernel = stride = f is a table lookup with a phase:
out[n, :, i f + a, j f + b] = base[n, :, i f + a, j f + b] + weight[code(n, i, j), :, a, b]. The code image is a LEVEL image
(N, 1, h, w) at the levels j / (n_codes - 1), as in ops.code_conv; a negative level adds nothing.

Part of the operator layer (pytorch_generative_amd.ops): HIP kernels behind torch.autograd.Function, called through the C-ABI
with tensor.data_ptr() and the current stream. No CPU / ATen fallback: a missing library, a CPU tensor or an unsupported shape raises."""

import ctypes

import torch

from pytorch_generative_amd import _lib
from pytorch_generative_amd.ops._common import _chk, _p, _sink, _stream

CODE_UP_MAX_FACTOR = 4


class _CodeUpsample(torch.autograd.Function):
    @staticmethod
    def forward(ctx, levels, weight, base, factor, gw):
        lib = _lib.load()
        levels = _chk(levels, "code_upsample.levels")
        weight = _chk(weight, "code_upsample.weight")
        n, _, h, w = levels.shape
        k, cout, f, _ = weight.shape
        if base is not None:
            base = _chk(base, "code_upsample.base")
        ws_n = lib.pg_code_up_fwd_workspace_floats(k, cout, f)
        ws = torch.empty(max(ws_n, 1), device=levels.device, dtype=torch.float32)
        out = torch.empty((n, cout, h * f, w * f), device=levels.device, dtype=torch.float32)
        _lib.check(lib.pg_code_up_fwd(levels.data_ptr(), weight.data_ptr(), _p(base), out.data_ptr(), n, k, h, w, cout, f,
                                      ws.data_ptr(), ws_n, _stream()), "pg_code_up_fwd")
        ctx.save_for_backward(levels)
        ctx.wshape, ctx.gw, ctx.has_base = tuple(weight.shape), gw, base is not None
        return out

    @staticmethod
    def backward(ctx, dy):
        lib = _lib.load()
        (levels,) = ctx.saved_tensors
        dw = None
        if ctx.needs_input_grad[1]:
            dy = _chk(dy, "code_upsample.dy")
            n, _, h, w = levels.shape
            k, cout, f, _ = ctx.wshape
            tgt = ctx.gw
            if tgt is None:
                tgt = dw = torch.empty(ctx.wshape, device=dy.device, dtype=torch.float32)
            ws_n = lib.pg_code_up_wgrad_workspace_floats(n, k, h, w, cout, f)
            ws = torch.empty(max(ws_n, 1), device=dy.device, dtype=torch.float32)
            _lib.check(lib.pg_code_up_wgrad(levels.data_ptr(), dy.data_ptr(), tgt.data_ptr(), int(ctx.gw is not None), n, k, h,
                                            w, cout, f, ws.data_ptr(), ws_n, _stream()), "pg_code_up_wgrad")
        db = dy if ctx.has_base and ctx.needs_input_grad[2] else None  # the addition passes dy through as it is
        return None, dw, db, None, None


def _check_up(levels, weight, factor, base):
    factor = int(factor)
    if not 1 <= factor <= CODE_UP_MAX_FACTOR:
        raise ValueError(f"code_upsample: factor = {factor} outside 1..{CODE_UP_MAX_FACTOR}")
    if levels.dim() != 4 or levels.shape[1] != 1:
        raise ValueError(f"code_upsample: expected a level image (N, 1, h, w), got {tuple(levels.shape)}")
    if weight.dim() != 4 or tuple(weight.shape[2:]) != (factor, factor):
        raise ValueError(f"code_upsample: expected a weight (n_codes, C, {factor}, {factor}), got {tuple(weight.shape)}")
    n, _, h, w = levels.shape
    shape = (n, weight.shape[1], h * factor, w * factor)
    if base is not None and tuple(base.shape) != shape:
        raise ValueError(f"code_upsample: base {tuple(base.shape)} is not the output's shape {shape}")
    return factor


def code_upsample(levels, weight, factor, *, base=None, weight_param=None):
    """base + F.conv_transpose2d(one_hot(codes), weight, stride=factor) for the code image `levels` (N, 1, h, w) and a weight
    (n_codes, C, factor, factor): (N, C, h factor, w factor), one fp32 addition per element. No gradient with respect to
    `levels`; the gradient to `base` is the incoming one as it is; the weight gradient is added into the parameter's
    flat-gradient sink where weight_param carries one. Bit-reproducible in both directions."""
    factor = _check_up(levels, weight, factor, base)
    return _CodeUpsample.apply(levels, weight, base, factor, _sink(weight_param))


def code_upsample_(x, levels, weight, factor):
    """x += the lookup, in place and without autograd: the conditioned stem as one pass over x. Returns x."""
    lib = _lib.load()
    factor = _check_up(levels, weight, factor, x)
    levels, weight = _chk(levels.detach(), "code_upsample_.levels"), _chk(weight.detach(), "code_upsample_.weight")
    if not x.is_contiguous():
        raise ValueError("code_upsample_: x must be contiguous")
    _chk(x, "code_upsample_.x")
    n, _, h, w = levels.shape
    k, cout = weight.shape[:2]
    ws_n = lib.pg_code_up_fwd_workspace_floats(k, cout, factor)
    ws = torch.empty(max(ws_n, 1), device=x.device, dtype=torch.float32)
    _lib.check(lib.pg_code_up_fwd(levels.data_ptr(), weight.data_ptr(), x.data_ptr(), x.data_ptr(), n, k, h, w, cout, factor,
                                  ws.data_ptr(), ws_n, _stream()), "pg_code_up_fwd")
    return x


def code_up_plan(n, n_codes, h, w):
    """(max_chunks, items) of pg_code_up_wgrad for a (n, 1, h, w) code image, as ops.code_conv_wgrad_plan. Host only."""
    a, b = ctypes.c_int(0), ctypes.c_int(0)
    _lib.check(_lib.load().pg_code_up_plan(int(n), int(n_codes), int(h), int(w), ctypes.byref(a), ctypes.byref(b)),
               "pg_code_up_plan")
    return a.value, b.value


def sample_cond_codes_(x_plane, cond_levels, weight, factor, *, ld, pos_dev=None, row=0, col=0):
    """One raster position of the lookup for the incremental sampler: x_plane (the (C, ld) plane pg_sample_embed_codes
    writes) [co, n] += weight[code(n, r // f, c // f), co, r % f, c % f], the position from the int32 device scalar
    `pos_dev` (clamped to the image) or from (row, col)."""
    lib = _lib.load()
    cond_levels, weight = _chk(cond_levels, "sample_cond_codes.cond"), _chk(weight.detach(), "sample_cond_codes.weight")
    _chk(x_plane, "sample_cond_codes.x")
    n, _, h, w = cond_levels.shape
    k, cout = weight.shape[:2]
    if x_plane.numel() < cout * ld or not x_plane.is_contiguous():
        raise ValueError(f"sample_cond_codes: the plane holds {x_plane.numel()} floats, {cout} x {ld} needed, contiguous")
    _lib.check(lib.pg_sample_cond_codes(cond_levels.data_ptr(), weight.data_ptr(), x_plane.data_ptr(), n, k, h, w, cout,
                                        int(factor), int(row), int(col), int(ld), _p(pos_dev), _stream()),
               "pg_sample_cond_codes")
    return x_plane
