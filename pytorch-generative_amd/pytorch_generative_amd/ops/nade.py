"""ops.nade — NADE's whole network (reference models/autoregressive/nade.py:42-68) as one autograd Function on the chunked
prefix-scan kernels of csrc/nade.hip: a_0 = in_b, l_i = h_b[i] + relu(a_i) . h_w[i, :], p_i = sigmoid(l_i),
a_{i+1} = a_i + x_i in_w[:, i].

Part of the operator layer (pytorch_generative_amd.ops): HIP kernels behind torch.autograd.Function, called through the C-ABI
with tensor.data_ptr() and the current stream. No CPU / ATen fallback: a missing library, a CPU tensor or an unsupported shape raises."""

import ctypes

import torch

from pytorch_generative_amd import _lib
from pytorch_generative_amd.ops._common import _chk, _sink, _stream, zeros

PLAN_INTS = 15  # PG_NADE_PLAN_INTS
_PLAN_FIELDS = ("chunk", "chunks", "units_per_thread", "samples_per_workgroup", "hidden_padded", "forward_workgroups",
                "backward_tile", "partial_rows", "tiles_per_row", "backward_workgroups", "lds_bytes", "checkpoint_floats",
                "workspace_floats", "max_partial_rows", "max_hidden")


def _plan(d, h, n, what="pg_nade_plan"):
    out = (ctypes.c_longlong * PLAN_INTS)()
    _lib.check(_lib.load().pg_nade_plan(int(d), int(h), int(n), out, PLAN_INTS), what)
    return dict(zip(_PLAN_FIELDS, out))


def nade_plan(D, H, N):
    """The planner's answer (pg_nade_plan, host only): None for a shape it refuses, else a dict with the chunk length over D and
    the number of chunks, the hidden units per forward thread and the samples per forward workgroup, H padded, the forward
    workgroups, the samples of a backward tile, the partial rows of the sums over samples (at most max_partial_rows) and the
    sample tiles a backward workgroup loops over, the backward workgroups, the LDS bytes, the floats of the checkpoints
    (chunks, N, H padded) and of the partial-row workspace, and the largest H of the domain."""
    out = (ctypes.c_longlong * PLAN_INTS)()
    if _lib.load().pg_nade_plan(int(D), int(H), int(N), out, PLAN_INTS):
        return None
    return dict(zip(_PLAN_FIELDS, out))


class _NADE(torch.autograd.Function):
    """(x, in_w, in_b, h_w, h_b) -> (probs, logits). The forward saves the pre-activations at the chunk starts; the backward
    recomputes inside a chunk from them by the forward's own additions. Gradients of the four parameters go straight into
    FlatAdam's gradient sinks when they exist; none with respect to x."""

    @staticmethod
    def forward(ctx, x, in_w, in_b, h_w, h_b):
        lib = _lib.load()
        for t, name in ((x, "x"), (in_w, "in_w"), (in_b, "in_b"), (h_w, "h_w"), (h_b, "h_b")):
            if _chk(t, f"nade.{name}") is not t:
                raise ValueError(f"nade: {name} must be contiguous")
        if x.dim() != 2 or in_w.dim() != 2:
            raise ValueError(f"nade: expected x (N, D) and in_w (H, D), got {tuple(x.shape)}, {tuple(in_w.shape)}")
        n, d = x.shape
        h = in_w.shape[0]
        for name, t, shape in (("in_w", in_w, (h, d)), ("in_b", in_b, (h,)), ("h_w", h_w, (d, h)), ("h_b", h_b, (d,))):
            if tuple(t.shape) != shape:
                raise ValueError(f"nade: {name} of shape {tuple(t.shape)}, expected {shape} (N = {n}, D = {d}, H = {h})")
        plan = _plan(d, h, n, "nade")
        ckpt = torch.empty(plan["checkpoint_floats"], device=x.device, dtype=torch.float32)
        probs, logits = torch.empty_like(x), torch.empty_like(x)
        _lib.check(lib.pg_nade_fwd(x.data_ptr(), in_w.data_ptr(), in_b.data_ptr(), h_w.data_ptr(), h_b.data_ptr(),
                                   ckpt.data_ptr(), probs.data_ptr(), logits.data_ptr(), n, d, h, _stream()), "pg_nade_fwd")
        ctx.plan = plan
        ctx.sinks = [_sink(p) for p in (in_w, in_b, h_w, h_b)]
        ctx.save_for_backward(x, in_w, h_w, logits, ckpt)
        ctx.mark_non_differentiable(logits)
        return probs, logits

    @staticmethod
    def backward(ctx, g, _g_logits):
        lib = _lib.load()
        x, in_w, h_w, logits, ckpt = ctx.saved_tensors
        g = _chk(g, "nade.grad")
        n, d = x.shape
        h = in_w.shape[0]
        shapes = ((h, d), (h,), (d, h), (d,))
        targets, ret = [], []
        for need, sink, shape in zip(ctx.needs_input_grad[1:], ctx.sinks, shapes):
            if not need:
                targets.append(None)
                ret.append(None)
            elif sink is not None:
                targets.append(sink)
                ret.append(None)
            else:
                z = zeros(shape, x.device)
                targets.append(z)
                ret.append(z)
        etot = torch.empty_like(ckpt)
        ws_floats = ctx.plan["workspace_floats"]
        ws = torch.empty(ws_floats, device=x.device, dtype=torch.float32)
        ptr = [0 if t is None else t.data_ptr() for t in targets]
        _lib.check(lib.pg_nade_bwd(x.data_ptr(), in_w.data_ptr(), h_w.data_ptr(), logits.data_ptr(), g.data_ptr(),
                                   ckpt.data_ptr(), etot.data_ptr(), ptr[0], ptr[1], ptr[2], ptr[3], n, d, h, ws.data_ptr(),
                                   ws_floats, _stream()), "pg_nade_bwd")
        return (None, *ret)


def nade(x, in_w, in_b, h_w, h_b, *, return_logits=False):
    """NADE's probabilities p (N, D) of x (N, D) under in_w (H, D), in_b (H), h_w (D, H), h_b (D); with return_logits:
    (p, logits), the logits outside autograd. x is used AS GIVEN (teacher forcing, any float): the reference draws the entries
    that are negative inside its forward, here only the model's sample() draws. Differentiable in the four parameters; the
    gradient with respect to x is not built, so an x that requires grad raises. Any N, D >= 1 and H in 1..8192 (ops.nade_plan).
    Two launches forward, four backward, no host synchronisation (capturable); outputs and gradients are bit-identical from run
    to run, a sample's row also for any N."""
    if x.requires_grad:
        raise ValueError("nade: the gradient with respect to x is not built (x.requires_grad is set)")
    probs, logits = _NADE.apply(x, in_w, in_b, h_w, h_b)
    return (probs, logits) if return_logits else probs
