"""ops.nice — NICE's building blocks (reference models/flow/nice.py) on the dense fp32-MFMA GEMMs and the streaming kernels of
csrc/dense_linear.hip: an additive coupling block as ONE autograd node, the diagonal scaling layer, the logistic prior.

Part of the operator layer (pytorch_generative_amd.ops): HIP kernels behind torch.autograd.Function, called through the C-ABI
with tensor.data_ptr() and the current stream. No CPU / ATen fallback: a missing library, a CPU tensor or an unsupported shape raises."""

import ctypes

import torch

from pytorch_generative_amd import _lib
from pytorch_generative_amd.ops._common import _chk, _p, _sink, _stream, zeros

DENSE_FWD, DENSE_DGRAD, DENSE_WGRAD = 0, 1, 2  # include/pg_hip.h PG_DENSE_*
_KINDS = {"fwd": DENSE_FWD, "dgrad": DENSE_DGRAD, "wgrad": DENSE_WGRAD, DENSE_FWD: DENSE_FWD, DENSE_DGRAD: DENSE_DGRAD,
          DENSE_WGRAD: DENSE_WGRAD}
PLAN_INTS = 14  # PG_DENSE_PLAN_INTS
_PLAN_FIELDS = ("variant", "tile_rows", "tile_cols", "k_chunk", "rows", "cols", "depth", "row_tiles", "col_tiles", "slices",
                "k_per_slice", "workgroups", "reduce_workgroups", "workspace_floats")
_F = 4  # bytes of a float


def _plan(n, in_f, out_f, kind, what):
    """dense_linear_plan that raises the library's message for a shape outside the domain."""
    lib = _lib.load()
    out = (ctypes.c_longlong * PLAN_INTS)()
    rc = lib.pg_dense_linear_plan(int(n), int(in_f), int(out_f), _KINDS[kind], out, PLAN_INTS)
    _lib.check(rc, what)
    return dict(zip(_PLAN_FIELDS, out))


def dense_linear_plan(N, in_features, out_features, kind="fwd"):
    """The planner's answer (pg_dense_linear_plan, host only) for the product `kind` ("fwd", "dgrad" or "wgrad") of a linear layer
    on N rows: None for a shape it refuses, else a dict with the tile variant (0: 64 x 64, 1: 128 x 128), the tile's rows and
    columns and its k chunk, the rows, columns and depth of the product, the row and column tiles, the k slices and the k of a
    slice, the workgroups of the GEMM and of the reduce launch, and the workspace floats (0 without a k-split)."""
    try:
        return _plan(N, in_features, out_features, kind, "dense_linear_plan")
    except ValueError:
        return None


def _workspace(n, in_f, out_f, kind, device, what):
    floats = _plan(n, in_f, out_f, kind, what)["workspace_floats"]
    return (torch.empty(floats, device=device, dtype=torch.float32), floats) if floats else (None, 0)


def _copy_half(lib, src, dst, n, f, off, half):
    _lib.check(lib.pg_copy_rows(src.data_ptr() + _F * off, dst.data_ptr() + _F * off, n, half, f, f, 0, _stream()), "pg_copy_rows")


class _Coupling(torch.autograd.Function):
    """x (N, F) -> y (N, F): the pass-through half copied, the other half + sign * m(pass-through half), m the ReLU network of
    `params` = (w_0, b_0, w_1, b_1, ...). The forward keeps the ReLU outputs; the backward runs weight and data gradient per
    layer, ReLU's derivative fused into the data gradient from the stored output, and writes the input gradient as one (N, F)
    tensor. Weight and bias gradients go straight into FlatAdam's gradient sinks when they exist."""

    @staticmethod
    def forward(ctx, x, reverse, sign, *params):
        lib = _lib.load()
        if _chk(x, "coupling.x") is not x:
            raise ValueError("coupling: x must be contiguous")
        if x.dim() != 2 or x.shape[1] % 2 or x.shape[1] < 2:
            raise ValueError(f"coupling: expected x of shape (N, F) with F even, got {tuple(x.shape)}")
        if sign not in (1, -1):
            raise ValueError(f"coupling: sign must be +1 or -1, got {sign!r}")
        n_layers = len(params) // 2
        if n_layers < 1 or len(params) != 2 * n_layers:
            raise ValueError("coupling: expected at least one (weight, bias) pair")
        n, f = x.shape
        half = f // 2
        pass_off, tr_off = (half, 0) if reverse else (0, half)
        width = half
        for li in range(n_layers):
            w, b = params[2 * li], params[2 * li + 1]
            if _chk(w, "coupling.weight") is not w or w.dim() != 2 or w.shape[1] != width:
                raise ValueError(f"coupling: layer {li}: weight {tuple(w.shape)} does not take {width} inputs (contiguous (out, in) expected)")
            if _chk(b, "coupling.bias") is not b or tuple(b.shape) != (w.shape[0],):
                raise ValueError(f"coupling: layer {li}: bias {tuple(b.shape)} != ({w.shape[0]},)")
            width = w.shape[0]
        if width != half:
            raise ValueError(f"coupling: the last layer gives {width} features, the transformed half has {half}")
        y = torch.empty_like(x)
        _copy_half(lib, x, y, n, f, pass_off, half)
        hidden = []
        h_ptr, h_ld = x.data_ptr() + _F * pass_off, f
        for li in range(n_layers):
            w, b = params[2 * li], params[2 * li + 1]
            out_f, in_f = w.shape
            ws, ws_floats = _workspace(n, in_f, out_f, DENSE_FWD, x.device, "coupling")
            if li < n_layers - 1:
                h = torch.empty((n, out_f), device=x.device, dtype=torch.float32)
                _lib.check(lib.pg_dense_linear_fwd(h_ptr, h_ld, w.data_ptr(), b.data_ptr(), 0, 0, 1, h.data_ptr(), out_f, n, in_f,
                                                   out_f, 1, _p(ws), ws_floats, _stream()), "pg_dense_linear_fwd")
                hidden.append(h)
                h_ptr, h_ld = h.data_ptr(), out_f
            else:
                _lib.check(lib.pg_dense_linear_fwd(h_ptr, h_ld, w.data_ptr(), b.data_ptr(), x.data_ptr() + _F * tr_off, f, sign,
                                                   y.data_ptr() + _F * tr_off, f, n, in_f, out_f, 0, _p(ws), ws_floats, _stream()),
                           "pg_dense_linear_fwd")
        ctx.geom = (n, f, half, pass_off, tr_off, sign, n_layers)
        ctx.sinks = [_sink(p) for p in params]
        ctx.save_for_backward(x, *hidden, *params[0::2])
        return y

    @staticmethod
    def backward(ctx, g):
        lib = _lib.load()
        n, f, half, pass_off, tr_off, sign, n_layers = ctx.geom
        saved = ctx.saved_tensors
        x, hidden, weights = saved[0], saved[1:n_layers], saved[n_layers:]
        g = _chk(g, "coupling.grad")
        dev = x.device
        grads = [None] * (2 * n_layers)
        dx = None
        if ctx.needs_input_grad[0]:
            dx = torch.empty_like(x)
            _copy_half(lib, g, dx, n, f, tr_off, half)  # y_t = x_t + sign m(x_p): the transformed half's gradient passes through
        d_ptr, d_ld = g.data_ptr() + _F * tr_off, f
        for li in reversed(range(n_layers)):
            w = weights[li]
            out_f, in_f = w.shape
            s = sign if li == n_layers - 1 else 1  # d m = sign * g_t: the scale enters at the last layer's products
            in_ptr, in_ld = (hidden[li - 1].data_ptr(), in_f) if li > 0 else (x.data_ptr() + _F * pass_off, f)
            need_w, need_b = ctx.needs_input_grad[3 + 2 * li], ctx.needs_input_grad[4 + 2 * li]
            if need_w or need_b:
                sw, sb = ctx.sinks[2 * li], ctx.sinks[2 * li + 1]
                # a weight that needs no gradient gets a scratch buffer, never its sink (the launch always forms dw)
                dw = sw if (need_w and sw is not None) else zeros((out_f, in_f), dev)
                db = None
                if need_b:
                    db = sb if sb is not None else zeros((out_f,), dev)
                ws, ws_floats = _workspace(n, in_f, out_f, DENSE_WGRAD, dev, "coupling")
                _lib.check(lib.pg_dense_linear_wgrad(in_ptr, in_ld, d_ptr, d_ld, s, dw.data_ptr(), _p(db), n, in_f, out_f, _p(ws),
                                                     ws_floats, _stream()), "pg_dense_linear_wgrad")
                if need_w and sw is None:
                    grads[2 * li] = dw
                if need_b and sb is None:
                    grads[2 * li + 1] = db
            if li > 0:
                d = torch.empty((n, in_f), device=dev, dtype=torch.float32)
                ws, ws_floats = _workspace(n, in_f, out_f, DENSE_DGRAD, dev, "coupling")
                _lib.check(lib.pg_dense_linear_dgrad(d_ptr, d_ld, w.data_ptr(), in_ptr, in_ld, 0, 0, s, d.data_ptr(), in_f, n, in_f,
                                                     out_f, _p(ws), ws_floats, _stream()), "pg_dense_linear_dgrad")
                d_ptr, d_ld = d.data_ptr(), in_f  # the allocator is stream ordered: the launch that reads d is already queued
            elif dx is not None:  # the pass-through half: its own incoming gradient + the network's
                ws, ws_floats = _workspace(n, in_f, out_f, DENSE_DGRAD, dev, "coupling")
                _lib.check(lib.pg_dense_linear_dgrad(d_ptr, d_ld, w.data_ptr(), 0, 0, g.data_ptr() + _F * pass_off, f, s,
                                                     dx.data_ptr() + _F * pass_off, f, n, in_f, out_f, _p(ws), ws_floats, _stream()),
                           "pg_dense_linear_dgrad")
        return (dx, None, None, *grads)


def coupling(x, layers, reverse, sign=1):
    """An additive coupling block (nice.py:48-63) on x (N, F), F even: `layers` is a list of (weight (out, in), bias (out)), ReLU
    between consecutive layers and none after the last; the first takes F / 2 inputs, the last gives F / 2 outputs. reverse =
    False: y1 = x1, y2 = x2 + sign * m(x1); True: y2 = x2, y1 = x1 + sign * m(x2). sign = -1 is the block's inverse. One
    autograd node; differentiable in x and every parameter. No host synchronisation (capturable); bit-identical run to run."""
    params = []
    for w, b in layers:
        params += [w, b]
    return _Coupling.apply(x, bool(reverse), int(sign), *params)


class _NiceScale(torch.autograd.Function):
    @staticmethod
    def forward(ctx, y, log_scale, sign):
        lib = _lib.load()
        y = _chk(y, "nice_scale.y")
        s = _chk(log_scale, "nice_scale.log_scale")
        if y.dim() != 2 or s.numel() != y.shape[1]:
            raise ValueError(f"nice_scale: expected y (N, F) and F log-scales, got {tuple(y.shape)}, {tuple(log_scale.shape)}")
        if sign not in (1, -1):
            raise ValueError(f"nice_scale: sign must be +1 or -1, got {sign!r}")
        z = torch.empty_like(y)
        _lib.check(lib.pg_nice_scale_fwd(y.data_ptr(), s.data_ptr(), z.data_ptr(), y.shape[0], y.shape[1], sign, _stream()),
                   "pg_nice_scale_fwd")
        ctx.sign, ctx.sink, ctx.s_shape = sign, _sink(log_scale), tuple(log_scale.shape)
        ctx.save_for_backward(z, s)
        return z

    @staticmethod
    def backward(ctx, g):
        lib = _lib.load()
        z, s = ctx.saved_tensors
        g = _chk(g, "nice_scale.grad")
        n, f = z.shape
        dy = torch.empty_like(z) if ctx.needs_input_grad[0] else None
        ds = ret = None
        if ctx.needs_input_grad[1]:
            ds = ctx.sink
            if ds is None:
                ds = ret = zeros(ctx.s_shape, z.device)
        floats = int(lib.pg_nice_scale_bwd_workspace_floats(n, f))
        ws = torch.empty(floats, device=z.device, dtype=torch.float32)
        _lib.check(lib.pg_nice_scale_bwd(g.data_ptr(), z.data_ptr(), s.data_ptr(), _p(dy), _p(ds), n, f, ctx.sign, ws.data_ptr(), floats,
                                         _stream()), "pg_nice_scale_bwd")
        return dy, ret, None


def nice_scale(y, log_scale, sign=1):
    """NICE's scaling layer (nice.py:85-89): z = y * exp(sign * log_scale) for y (N, F) and F log-scales (any shape with F
    elements). Differentiable in both; the gradient of log_scale is a sum over samples in a fixed order."""
    return _NiceScale.apply(y, log_scale, int(sign))


class _LogisticLogProb(torch.autograd.Function):
    @staticmethod
    def forward(ctx, z):
        lib = _lib.load()
        z = _chk(z, "logistic_logprob.z")
        if z.dim() < 2:
            raise ValueError(f"logistic_logprob: expected (N, ...) with at least two dimensions, got {tuple(z.shape)}")
        n = z.shape[0]
        lp = torch.empty(n, device=z.device, dtype=torch.float32)
        _lib.check(lib.pg_logistic_logprob_fwd(z.data_ptr(), lp.data_ptr(), n, z.numel() // n, _stream()), "pg_logistic_logprob_fwd")
        ctx.save_for_backward(z)
        return lp

    @staticmethod
    def backward(ctx, g):
        lib = _lib.load()
        (z,) = ctx.saved_tensors
        g = _chk(g, "logistic_logprob.grad")
        n = z.shape[0]
        dz = torch.empty_like(z)
        _lib.check(lib.pg_logistic_logprob_bwd(z.data_ptr(), g.data_ptr(), dz.data_ptr(), n, z.numel() // n, _stream()),
                   "pg_logistic_logprob_bwd")
        return dz


def logistic_logprob(z):
    """Per-sample log-density of z (N, ...) under the standard logistic prior of NICE's recipe (nice.py:207):
    -(softplus(z) + softplus(-z)) summed over everything but the batch, in the overflow-safe form |z| + 2 log1p(exp(-|z|)).
    Returns (N,)."""
    return _LogisticLogProb.apply(z)
