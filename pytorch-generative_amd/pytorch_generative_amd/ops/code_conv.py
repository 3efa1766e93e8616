"""ops.code_conv — convolution over an image of code indices (csrc/code_conv.hip), the VQ codebook lookup by code image.

F.conv2d(one_hot(codes), weight) is a table lookup: out[n, :, y, x] = b + sum_taps W[:, code(n, y + dy, x + dx), tap]. The code
image is a LEVEL image (N, 1, H, W) at the levels j / (n_codes - 1) — what ops.categorical_nll_sum_mean takes as its target and
nn.CategoricalSampler returns — and a negative level (an undrawn canvas position) is the all-zero one-hot vector.

Part of the operator layer (pytorch_generative_amd.ops): HIP kernels behind torch.autograd.Function, called through the C-ABI
with tensor.data_ptr() and the current stream. No CPU / ATen fallback: a missing library, a CPU tensor or an unsupported shape raises."""

import ctypes

import torch

from pytorch_generative_amd import _lib
from pytorch_generative_amd.ops._common import _chk, _p, _sink, _stream

CODE_MAX_CODES = 4096


def _check_codes(weight, n_codes, what):
    n_codes = int(n_codes)
    if not 2 <= n_codes <= CODE_MAX_CODES:
        raise ValueError(f"{what}: n_codes = {n_codes} outside 2..{CODE_MAX_CODES}")
    if weight.dim() != 4 or weight.shape[1] != n_codes:
        raise ValueError(f"{what}: n_codes = {n_codes} must equal the weight's {weight.shape[1]} input channels")
    return n_codes


class _CodeConv(torch.autograd.Function):
    @staticmethod
    def forward(ctx, levels, weight, bias, spec, n_codes, out_hw, gw, gb):
        lib = _lib.load()
        levels = _chk(levels, "code_conv2d.levels")
        weight = _chk(weight, "code_conv2d.weight")
        if bias is not None:
            bias = _chk(bias, "code_conv2d.bias")
        if levels.dim() != 4 or levels.shape[1] != 1:
            raise ValueError(f"code_conv2d: expected a level image (N, 1, H, W), got {tuple(levels.shape)}")
        n, _, ih, iw = levels.shape
        cout, k, kh, kw = weight.shape
        if (kh, kw) != (spec.kh, spec.kw):
            raise ValueError("code_conv2d: the weight's kernel size differs from the ConvSpec's")
        oh, ow = out_hw
        t = len(spec.fwd_taps)
        ws_n = lib.pg_code_conv_fwd_workspace_floats(cout, k, t)
        ws = torch.empty(max(ws_n, 1), device=levels.device, dtype=torch.float32)
        out = torch.empty((n, cout, oh, ow), device=levels.device, dtype=torch.float32)
        _lib.check(lib.pg_code_conv_fwd(levels.data_ptr(), weight.data_ptr(), _p(bias), out.data_ptr(), n, k, ih, iw, cout,
                                        kh, kw, oh, ow, t, spec.f_u, spec.f_v, spec.pad_h, spec.pad_w, ws.data_ptr(), ws_n,
                                        _stream()), "pg_code_conv_fwd")
        ctx.save_for_backward(levels)
        ctx.spec, ctx.wshape, ctx.has_bias, ctx.gw, ctx.gb = spec, tuple(weight.shape), bias is not None, gw, gb
        return out

    @staticmethod
    def backward(ctx, dy):
        lib = _lib.load()
        (levels,) = ctx.saved_tensors
        need_w, need_b = ctx.needs_input_grad[1], ctx.has_bias and ctx.needs_input_grad[2]
        dw = db = None
        if need_w or need_b:
            dy = _chk(dy, "code_conv2d.dy")
            spec = ctx.spec
            if len(spec.wg_taps) != spec.kh * spec.kw:
                raise ValueError("code_conv2d: the weight gradient covers all taps (ConvSpec(wgrad_all=True))")
            n, _, ih, iw = levels.shape
            cout, k, kh, kw = ctx.wshape
            _, _, oh, ow = dy.shape
            gw_t = gb_t = None
            if need_w:
                gw_t = ctx.gw
                if gw_t is None:
                    gw_t = dw = torch.empty(ctx.wshape, device=dy.device, dtype=torch.float32)
            if need_b:
                gb_t = ctx.gb
                if gb_t is None:
                    gb_t = db = torch.empty((cout,), device=dy.device, dtype=torch.float32)
            # the two gradients share `accumulate`: a sink on one and not on the other takes two calls
            if gw_t is not None and gb_t is not None and (ctx.gw is None) == (ctx.gb is None):
                calls = [(gw_t, gb_t, ctx.gw is not None)]
            else:
                calls = [(gw_t, None, ctx.gw is not None)] if gw_t is not None else []
                if gb_t is not None:
                    calls.append((None, gb_t, ctx.gb is not None))
            ws_n = lib.pg_code_conv_wgrad_workspace_floats(n, k, ih, iw, cout, kh, kw)
            ws = torch.empty(max(ws_n, 1), device=dy.device, dtype=torch.float32)
            for w_t, b_t, acc in calls:
                _lib.check(lib.pg_code_conv_wgrad(levels.data_ptr(), dy.data_ptr(), _p(w_t), _p(b_t), int(acc), n, k, ih, iw,
                                                  cout, kh, kw, oh, ow, spec.pad_h, spec.pad_w, ws.data_ptr(), ws_n,
                                                  _stream()), "pg_code_conv_wgrad")
        return None, dw, db, None, None, None, None, None


def code_conv2d(levels, weight, bias, spec, n_codes, *, out_hw=None, weight_param=None, bias_param=None):
    """F.conv2d(one_hot(codes), weight (already masked), bias) restricted to spec's active taps, cropped to out_hw, for the
    code image `levels` (N, 1, H, W). No gradient with respect to `levels`; the weight gradient covers all kh * kw taps
    (the reference's is unmasked) and, like the bias gradient, is added into the parameter's flat-gradient sink where
    weight_param / bias_param carry one. Bit-reproducible in both directions."""
    _check_codes(weight, n_codes, "code_conv2d")
    if levels.dim() != 4 or levels.shape[1] != 1:
        raise ValueError(f"code_conv2d: expected a level image (N, 1, H, W), got {tuple(levels.shape)}")
    full = spec.full_out(levels.shape[2], levels.shape[3])
    if out_hw is None:
        out_hw = full
    if out_hw[0] > full[0] + spec.kh or out_hw[1] > full[1] + spec.kw or min(out_hw) < 1:
        # (up to one kernel's worth beyond the full extent reads only zero padding, as ops.conv2d_taps allows)
        raise ValueError(f"code_conv2d: requested output {tuple(out_hw)} is empty or more than one kernel beyond the "
                         f"full extent {full}")
    return _CodeConv.apply(levels, weight, bias, spec, int(n_codes), tuple(out_hw), _sink(weight_param), _sink(bias_param))


def code_conv_wgrad_plan(n, n_codes, h, w):
    """(max_chunks, items) of pg_code_conv_wgrad for a (n, 1, h, w) code image: the chunks of the longest possible list
    (more than one: the merge of partial sums in chunk order can run) and the work items reserved. Host only."""
    a, b = ctypes.c_int(0), ctypes.c_int(0)
    _lib.check(_lib.load().pg_code_conv_wgrad_plan(int(n), int(n_codes), int(h), int(w), ctypes.byref(a), ctypes.byref(b)),
               "pg_code_conv_wgrad_plan")
    return a.value, b.value


def vq_lookup(levels, embedding):
    """The (N, D, h, w) decoder input of a VQ-VAE from a code image (N, 1, h, w) at the levels j / (K - 1) and the
    codebook (K, D): embedding[codes] moved to channels-first, bit for bit. No gradient."""
    lib = _lib.load()
    levels = _chk(levels.detach(), "vq_lookup.levels")
    embedding = _chk(embedding.detach(), "vq_lookup.embedding")
    if levels.dim() != 4 or levels.shape[1] != 1 or embedding.dim() != 2:
        raise ValueError(f"vq_lookup: expected levels (N, 1, h, w) and a codebook (K, D), got {tuple(levels.shape)}, "
                         f"{tuple(embedding.shape)}")
    n, _, h, w = levels.shape
    k, d = embedding.shape
    out = torch.empty((n, d, h, w), device=levels.device, dtype=torch.float32)
    _lib.check(lib.pg_vq_lookup(levels.data_ptr(), embedding.data_ptr(), out.data_ptr(), n, d, h * w, k, _stream()),
               "pg_vq_lookup")
    return out


def codes_to_levels(indices, n_codes):
    """(…) integer codes -> float32 levels j / (n_codes - 1), the division done in fp32 as the kernels invert it."""
    return indices.to(torch.float32) / float(n_codes - 1)
