"""ops.masked_linear — MADE's masked linear layers (reference models/autoregressive/made.py:21-33) on the masked
fp32-MFMA GEMMs of csrc/masked_linear.hip.

Part of the operator layer (pytorch_generative_amd.ops): HIP kernels behind torch.autograd.Function, called through the C-ABI
with tensor.data_ptr() and the current stream. No CPU / ATen fallback: a missing library, a CPU tensor or an unsupported shape raises."""

import torch

from pytorch_generative_amd import _lib
from pytorch_generative_amd.ops._common import _chk, _p, _sink, _stream, zeros


def _chk_deg(t, n, name):
    if t is None:
        return None
    if not t.is_cuda or t.dtype != torch.int32 or t.dim() != 1 or t.numel() != n or not t.is_contiguous():
        raise ValueError(f"{name}: expected a contiguous int32 cuda vector of {n} degrees, got "
                         f"{tuple(t.shape)} {t.dtype} on {t.device}")
    return t


def _workspace(lib, n, in_f, out_f, dgrad, device):
    floats = int(lib.pg_masked_linear_workspace_floats(n, in_f, out_f, int(dgrad)))
    return (torch.empty(floats, device=device, dtype=torch.float32), floats) if floats else (None, 0)


class _MaskedMLP(torch.autograd.Function):
    """x -> L_{k-1}(relu(... relu(L_0(x)))) with L_l(h) = h (W_l o M_l)^T + b_l: ReLU fused into every epilogue but the
    last, its derivative into the next layer's data gradient (from the stored ReLU output, which is that layer's
    input). The weight gradients are unmasked and go straight into FlatAdam's gradient sinks when they exist."""

    @staticmethod
    def forward(ctx, x, layers, *params):
        lib = _lib.load()
        h = _chk(x, "masked_linear.x")
        if h.dim() != 2:
            raise ValueError(f"masked_linear: expected x of shape (N, in), got {tuple(h.shape)}")
        inputs, weights = [], []
        for li, (deg_in, deg_out, strict) in enumerate(layers):
            w, b = params[2 * li], params[2 * li + 1]
            _chk(w, "masked_linear.weight")  # in place: must already be contiguous (never a copy)
            if not w.is_contiguous() or w.dim() != 2 or w.shape[1] != h.shape[1]:
                raise ValueError(f"masked_linear: layer {li}: weight {tuple(w.shape)} does not take inputs "
                                 f"{tuple(h.shape)} (contiguous (out, in) expected)")
            out_f, in_f = w.shape
            if b is not None:
                b = _chk(b, "masked_linear.bias")
                if b.shape != (out_f,):
                    raise ValueError(f"masked_linear: layer {li}: bias {tuple(b.shape)} != ({out_f},)")
            if (deg_in is None) != (deg_out is None):
                raise ValueError("masked_linear: pass both degree vectors or neither")
            _chk_deg(deg_in, in_f, "masked_linear.deg_in")
            _chk_deg(deg_out, out_f, "masked_linear.deg_out")
            y = torch.empty((h.shape[0], out_f), device=h.device, dtype=torch.float32)
            ws, ws_floats = _workspace(lib, h.shape[0], in_f, out_f, False, h.device)
            _lib.check(lib.pg_masked_linear_fwd(h.data_ptr(), w.data_ptr(), _p(b), _p(deg_in), _p(deg_out),
                                                int(strict), y.data_ptr(), h.shape[0], in_f, out_f,
                                                int(li < len(layers) - 1), _p(ws), ws_floats, _stream()),
                       "pg_masked_linear_fwd")
            inputs.append(h)
            weights.append(w)
            h = y
        ctx.layers = layers
        ctx.has_bias = [params[2 * li + 1] is not None for li in range(len(layers))]
        ctx.sinks = [(_sink(params[2 * li]), _sink(params[2 * li + 1])) for li in range(len(layers))]
        ctx.save_for_backward(*inputs, *weights)
        return h

    @staticmethod
    def backward(ctx, g):
        lib = _lib.load()
        n_layers = len(ctx.layers)
        saved = ctx.saved_tensors
        inputs, weights = saved[:n_layers], saved[n_layers:]
        g = _chk(g, "masked_linear.grad")
        grads = [None] * (2 * n_layers)
        dx = None
        for li in reversed(range(n_layers)):
            x, w = inputs[li], weights[li]
            out_f, in_f = w.shape
            n = x.shape[0]
            need_w, need_b = ctx.needs_input_grad[2 + 2 * li], ctx.has_bias[li] and ctx.needs_input_grad[3 + 2 * li]
            if need_w or need_b:
                sw, sb = ctx.sinks[li]
                dw = sw if sw is not None else zeros((out_f, in_f), x.device)
                db = None
                if need_b:
                    db = sb if sb is not None else zeros((out_f,), x.device)
                _lib.check(lib.pg_masked_linear_wgrad(x.data_ptr(), g.data_ptr(), dw.data_ptr(), _p(db), n, in_f,
                                                      out_f, _stream()),
                           "pg_masked_linear_wgrad")
                if need_w and sw is None:
                    grads[2 * li] = dw
                if need_b and sb is None:
                    grads[2 * li + 1] = db
            if li > 0 or ctx.needs_input_grad[0]:
                deg_in, deg_out, strict = ctx.layers[li]
                d = torch.empty((n, in_f), device=x.device, dtype=torch.float32)
                ws, ws_floats = _workspace(lib, n, in_f, out_f, True, x.device)
                _lib.check(lib.pg_masked_linear_dgrad(g.data_ptr(), w.data_ptr(), _p(deg_in), _p(deg_out),
                                                      int(strict), x.data_ptr() if li > 0 else 0, d.data_ptr(), n,
                                                      in_f, out_f, _p(ws), ws_floats, _stream()),
                           "pg_masked_linear_dgrad")
                if li > 0:
                    g = d
                else:
                    dx = d
        return (dx, None, *grads)


def masked_mlp(x, layers):
    """MADE's network (made.py:59-64): `layers` is a list of (weight, bias, deg_in, deg_out, strict) with ReLU between
    consecutive layers and none after the last. weight (out, in) is masked IN PLACE (weight.data *= M, as the
    reference) with M[o][i] = deg_in[i] <= deg_out[o] (strict: <); deg_in / deg_out are int32 cuda vectors, or both
    None for an unmasked layer. bias may be None. Returns (N, out of the last layer)."""
    params, cfg = [], []
    for w, b, deg_in, deg_out, strict in layers:
        params += [w, b]
        cfg.append((deg_in, deg_out, bool(strict)))
    return _MaskedMLP.apply(x, tuple(cfg), *params)


def masked_linear(x, weight, bias=None, deg_in=None, deg_out=None, strict=False):
    """One masked linear layer, no activation: x (N, in) -> x (weight o M)^T + bias (see masked_mlp)."""
    return masked_mlp(x, [(weight, bias, deg_in, deg_out, strict)])


def mask_from_degrees(mask, deg_in, deg_out, strict=False):
    """Writes M[o][i] = deg_in[i] <= deg_out[o] (strict: <) as 0. / 1. into the float32 (out, in) tensor `mask`."""
    mask = _chk(mask, "mask_from_degrees.mask")
    out_f, in_f = mask.shape
    _chk_deg(deg_in, in_f, "mask_from_degrees.deg_in")
    _chk_deg(deg_out, out_f, "mask_from_degrees.deg_out")
    _lib.check(_lib.load().pg_masked_linear_mask(mask.data_ptr(), deg_in.data_ptr(), deg_out.data_ptr(), int(strict),
                                                 in_f, out_f, _stream()),
               "pg_masked_linear_mask")
    return mask


def mul_mask_(weight, mask):
    """weight.data *= mask in place (MaskedLinear.forward, made.py:32) for a dense float mask of any values."""
    w = _chk(weight.data, "mul_mask_.weight")
    m = _chk(mask, "mul_mask_.mask")
    if w.data_ptr() != weight.data_ptr() or w.shape != m.shape:
        raise ValueError("mul_mask_: weight must be contiguous and shaped like the mask")
    _lib.check(_lib.load().pg_mul_inplace(w.data_ptr(), m.data_ptr(), w.numel(), _stream()), "pg_mul_inplace")
    return weight
