"""ops.made_sample — a whole sample of a one-hidden-layer MADE in one launch on cached hidden sums (csrc/made_sample.hip): the
hidden pre-activation is kept per sample and updated by one weight column per dimension, the one logit a dimension needs is one
dot product.

Part of the operator layer (pytorch_generative_amd.ops): HIP kernels called through the C-ABI with tensor.data_ptr() and the
current stream. Inference only (sample() runs under no_grad). No CPU / ATen fallback: a missing library, a CPU tensor or an
unsupported shape raises."""

import ctypes

import torch

from pytorch_generative_amd import _lib
from pytorch_generative_amd.ops._common import _chk, _stream

PLAN_INTS = 8  # PG_MADE_SAMPLE_PLAN_INTS
_PLAN_FIELDS = ("samples_per_workgroup", "threads", "units_per_thread", "lds_bytes", "pack_floats", "row_floats", "workgroups",
                "max_hidden")


def made_sample_plan(D, H, N):
    """The planner's answer (pg_made_sample_plan, host only): None for a shape it refuses, else a dict with the samples and
    threads of a workgroup, the hidden units per thread, the LDS bytes, the floats of the weight pack and of one padded
    weight row inside it, the workgroups of the launch and the largest H of the domain."""
    out = (ctypes.c_int * PLAN_INTS)()
    rc = _lib.load().pg_made_sample_plan(int(D), int(H), int(N), out, PLAN_INTS)
    if rc:
        return None
    return dict(zip(_PLAN_FIELDS, out))


def made_sample_chain(canvas, w1, b1, w2, b2, order, uniforms, *, return_logits=False):
    """Fills canvas (N, D) in place and returns it (with return_logits: (canvas, logits (N, D))). Per sample, a = b1, then for
    i = order[0], order[1], ...: l = b2[i] + relu(a) . w2[i, :]; the entry i is kept when it is >= 0 (any float) and is
    (uniforms[n, i] < sigmoid(l)) otherwise; logits[n, i] = l; a += x_i * w1[:, i]. All fp32.

    w1 (H, D), w2 (D, H): the two layers' weights ALREADY masked (the kernel evaluates no mask); order: int32 (D), a permutation
    of 0..D-1; uniforms (N, D), indexed by dimension. One pack kernel and one launch on the current stream, no host
    synchronisation (capturable); a sample's row is bit-identical from run to run and for any N."""
    for t, name in ((canvas, "canvas"), (w1, "w1"), (b1, "b1"), (w2, "w2"), (b2, "b2"), (uniforms, "uniforms")):
        if _chk(t, f"made_sample_chain.{name}") is not t:
            raise ValueError(f"made_sample_chain: {name} must be contiguous")
    if not order.is_cuda:
        raise RuntimeError(f"made_sample_chain.order: expected a tensor on the MI355X (cuda) device, got {order.device}")
    if order.dtype != torch.int32:
        raise TypeError(f"made_sample_chain.order: expected int32, got {order.dtype}")
    if canvas.dim() != 2 or w1.dim() != 2:
        raise ValueError(f"made_sample_chain: expected canvas (N, D) and w1 (H, D), got {tuple(canvas.shape)}, {tuple(w1.shape)}")
    n, d = canvas.shape
    h = w1.shape[0]
    want = {"w1": (w1, (h, d)), "b1": (b1, (h,)), "w2": (w2, (d, h)), "b2": (b2, (d,)), "order": (order, (d,)),
            "uniforms": (uniforms, (n, d))}
    for name, (t, shape) in want.items():
        if tuple(t.shape) != shape:
            raise ValueError(f"made_sample_chain: {name} of shape {tuple(t.shape)}, expected {shape} (N = {n}, D = {d}, H = {h})")
    if not order.is_contiguous() or order.device != canvas.device:
        raise ValueError("made_sample_chain: order must be contiguous and on the canvas's device")
    lib = _lib.load()
    plan = (ctypes.c_int * PLAN_INTS)()
    _lib.check(lib.pg_made_sample_plan(d, h, n, plan, PLAN_INTS), "pg_made_sample_plan")
    pack = torch.empty(plan[4], device=canvas.device, dtype=torch.float32)
    logits = torch.empty_like(canvas) if return_logits else None
    _lib.check(lib.pg_made_sample_pack(w1.data_ptr(), w2.data_ptr(), pack.data_ptr(), d, h, _stream()), "pg_made_sample_pack")
    _lib.check(lib.pg_made_sample(pack.data_ptr(), b1.data_ptr(), b2.data_ptr(), order.data_ptr(), canvas.data_ptr(),
                                  uniforms.data_ptr(), None if logits is None else logits.data_ptr(), n, d, h, _stream()),
               "pg_made_sample")
    return (canvas, logits) if return_logits else canvas
