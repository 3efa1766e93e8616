"""ops.fvbn — the Fully Visible Belief Network (reference models/autoregressive/fvbn.py) as one autograd Function on the
packed-triangular kernels of csrc/fvbn.hip: logits = x tril(W, -1)^T + b with W stored packed.

Packed layout: row i of the strictly lower triangle holds max(1, i) values (row 0: the reference's dummy weight), then zeros up
to a multiple of 4 floats; the rows lie one after another (fvbn_offsets). The forward never reads the pads' values or row 0,
the weight gradient never writes them.

Part of the operator layer (pytorch_generative_amd.ops): HIP kernels behind torch.autograd.Function, called through the C-ABI
with tensor.data_ptr() and the current stream. No CPU / ATen fallback: a missing library, a CPU tensor or an unsupported shape raises."""

import ctypes
import functools

import torch

from pytorch_generative_amd import _lib
from pytorch_generative_amd.ops._common import _chk, _sink, _stream, zeros

PLAN_INTS = 22  # PG_FVBN_PLAN_INTS
TILES_FWD, TILES_WGRAD = 0, 1  # PG_FVBN_TILES_*
_PLAN_FIELDS = ("packed_floats", "tile", "k_chunk", "column_tiles", "forward_row_tiles", "forward_workgroups", "forward_weight_tiles",
                "wgrad_tiles", "wgrad_slices", "samples_per_slice", "wgrad_workgroups", "reduce_workgroups", "workspace_floats",
                "sampler_samples_per_workgroup", "sampler_workgroups", "sampler_lds_bytes", "max_dims", "forward_slice_chunks",
                "forward_slices", "forward_split", "forward_reduce_workgroups", "forward_workspace_floats")


def fvbn_plan_status(D, N):
    """(status, plan): the C-ABI status of pg_fvbn_plan (0, PG_ESHAPE = -2, PG_EINVAL = -1) and the plan dict (None on error)."""
    out = (ctypes.c_longlong * PLAN_INTS)()
    rc = _lib.load().pg_fvbn_plan(int(D), int(N), out, PLAN_INTS)
    return rc, (None if rc else dict(zip(_PLAN_FIELDS, out)))


def fvbn_plan(D, N):
    """The planner's answer (pg_fvbn_plan, host only): None for a shape it refuses, else a dict with the floats of the packed
    weight, the tile edge and the k chunk, the tiles along D, the forward's tiles along N, workgroups and (column tile, k chunk)
    pairs, the weight gradient's tiles, slices along N, samples per slice, workgroups, merge workgroups and workspace floats,
    the sampler's samples per workgroup, workgroups and LDS bytes, the largest D of the domain, and the forward's k slices: the
    chunks of a slice, the slices over all column tiles, whether they run as workgroups of their own (forward_split), and then
    the merge workgroups and the workspace floats."""
    return fvbn_plan_status(D, N)[1]


def fvbn_tiles(D, kind):
    """The rectangles (i0, i1, j0, j1) of W the forward (kind TILES_FWD) or the weight gradient (TILES_WGRAD) visits
    (pg_fvbn_tiles, host only): together they hold every (i, j < i) exactly once."""
    lib = _lib.load()
    count = ctypes.c_longlong(0)
    _lib.check(lib.pg_fvbn_tiles(int(D), int(kind), None, 0, ctypes.byref(count)), "pg_fvbn_tiles")
    out = (ctypes.c_longlong * max(1, 4 * count.value))()
    _lib.check(lib.pg_fvbn_tiles(int(D), int(kind), out, count.value, ctypes.byref(count)), "pg_fvbn_tiles")
    return [tuple(out[4 * t:4 * t + 4]) for t in range(count.value)]


@functools.lru_cache(maxsize=8)
def _offsets(d):
    lib = _lib.load()
    return tuple(lib.pg_fvbn_row_offset(i) for i in range(d + 1))


def fvbn_offsets(D):
    """int64 (D + 1): off(0), ..., off(D) = P(D), the start of every row in the packed weight (pg_fvbn_row_offset)."""
    if D < 0:
        raise ValueError(f"fvbn_offsets: D = {D}")
    return torch.tensor(_offsets(int(D)), dtype=torch.int64)


def _plan(d, n, what):
    rc, plan = fvbn_plan_status(d, n)
    _lib.check(rc, what)
    return plan


def fvbn_pack(dense):
    """The packed weight (P(D),) of a dense (D, D) matrix: its strict lower triangle, row 0's dummy value from [0, 0], zero pads."""
    if _chk(dense, "fvbn_pack.dense") is not dense:
        raise ValueError("fvbn_pack: dense must be contiguous")
    if dense.dim() != 2 or dense.shape[0] != dense.shape[1]:
        raise ValueError(f"fvbn_pack: expected a (D, D) matrix, got shape {tuple(dense.shape)}")
    d = dense.shape[0]
    plan = _plan(d, 1, "fvbn_pack")
    out = torch.empty(plan["packed_floats"], device=dense.device, dtype=torch.float32)
    _lib.check(_lib.load().pg_fvbn_pack(dense.data_ptr(), out.data_ptr(), d, _stream()), "pg_fvbn_pack")
    return out


def fvbn_unpack(packed, D):
    """The dense (D, D) matrix of a packed weight: zeros on and above the diagonal, except row 0's dummy value at [0, 0]."""
    if _chk(packed, "fvbn_unpack.packed") is not packed:
        raise ValueError("fvbn_unpack: packed must be contiguous")
    plan = _plan(D, 1, "fvbn_unpack")
    if tuple(packed.shape) != (plan["packed_floats"],):
        raise ValueError(f"fvbn_unpack: packed of shape {tuple(packed.shape)}, expected ({plan['packed_floats']},) for D = {D}")
    out = torch.empty((D, D), device=packed.device, dtype=torch.float32)
    _lib.check(_lib.load().pg_fvbn_unpack(packed.data_ptr(), out.data_ptr(), int(D), _stream()), "pg_fvbn_unpack")
    return out


def _check_operands(what, x, weight, bias):
    for t, name in ((x, "x"), (weight, "weight"), (bias, "bias")):
        if _chk(t, f"{what}.{name}") is not t:
            raise ValueError(f"{what}: {name} must be contiguous")
    if x.dim() != 2:
        raise ValueError(f"{what}: expected x (N, D), got {tuple(x.shape)}")
    n, d = x.shape
    plan = _plan(d, n, what)
    for name, t, shape in (("weight", weight, (plan["packed_floats"],)), ("bias", bias, (d,))):
        if tuple(t.shape) != shape:
            raise ValueError(f"{what}: {name} of shape {tuple(t.shape)}, expected {shape} (N = {n}, D = {d})")
    return n, d, plan


class _FVBN(torch.autograd.Function):
    """(x, packed weight, bias) -> logits. The gradients of weight and bias go straight into FlatAdam's gradient sinks when
    they exist; none with respect to x."""

    @staticmethod
    def forward(ctx, x, weight, bias):
        n, d, plan = _check_operands("fvbn", x, weight, bias)
        logits = torch.empty_like(x)
        ws_floats = plan["forward_workspace_floats"]
        ws = torch.empty(ws_floats, device=x.device, dtype=torch.float32) if ws_floats else None
        _lib.check(_lib.load().pg_fvbn_fwd(x.data_ptr(), weight.data_ptr(), bias.data_ptr(), logits.data_ptr(), n, d,
                                           None if ws is None else ws.data_ptr(), ws_floats, _stream()), "pg_fvbn_fwd")
        ctx.plan = plan
        ctx.sinks = [_sink(weight), _sink(bias)]
        ctx.shapes = (tuple(weight.shape), tuple(bias.shape))
        ctx.save_for_backward(x)
        return logits

    @staticmethod
    def backward(ctx, g):
        (x,) = ctx.saved_tensors
        g = _chk(g, "fvbn.grad")
        n, d = x.shape
        targets, ret = [], []
        for need, sink, shape in zip(ctx.needs_input_grad[1:], ctx.sinks, ctx.shapes):
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
        ws_floats = ctx.plan["workspace_floats"]
        ws = torch.empty(ws_floats, device=x.device, dtype=torch.float32) if ws_floats else None
        ptr = [None if t is None else t.data_ptr() for t in targets]
        _lib.check(_lib.load().pg_fvbn_wgrad(x.data_ptr(), g.data_ptr(), ptr[0], ptr[1], n, d, None if ws is None else ws.data_ptr(),
                                             ws_floats, _stream()), "pg_fvbn_wgrad")
        return (None, *ret)


def fvbn(x, weight, bias):
    """The FVBN's logits (N, D) of x (N, D): logits[n, i] = bias[i] + sum_{j < i} W[i, j] x[n, j], W given as the packed weight
    (P(D),) (ops.fvbn_pack, ops.fvbn_offsets), bias (D). x is used AS GIVEN and must be finite: an entry x[n, j] meets an exact zero
    for every i <= j, so a NaN or infinity would spread where the reference never reads. Differentiable in weight and bias (the
    pads and row 0 of the weight gradient are exactly zero); the gradient with respect to x is not built, so an x that requires
    grad raises. D in 1..8192 (ops.fvbn_plan). One or two launches forward and backward, no host synchronisation (capturable);
    outputs and gradients are bit-identical from run to run, a sample's row also for any N."""
    if x.requires_grad:
        raise ValueError("fvbn: the gradient with respect to x is not built (x.requires_grad is set)")
    return _FVBN.apply(x, weight, bias)


def fvbn_sample_chain(canvas, weight, bias, uniforms, *, return_logits=False):
    """Fills canvas (N, D) in place and returns it (with return_logits: (canvas, logits (N, D))). Per sample, for i = 0 .. D - 1:
    l = bias[i] + sum_{j < i} W[i, j] x_j; the entry i is kept when it is >= 0 (any float) and is (uniforms[n, i] < sigmoid(l))
    otherwise; logits[n, i] = l. W is the packed weight (P(D),). One launch on the current stream, no host synchronisation
    (capturable); a sample's row is bit-identical from run to run and for any N."""
    n, d, _ = _check_operands("fvbn_sample_chain", canvas, weight, bias)
    if _chk(uniforms, "fvbn_sample_chain.uniforms") is not uniforms:
        raise ValueError("fvbn_sample_chain: uniforms must be contiguous")
    if tuple(uniforms.shape) != (n, d):
        raise ValueError(f"fvbn_sample_chain: uniforms of shape {tuple(uniforms.shape)}, expected {(n, d)}")
    logits = torch.empty_like(canvas) if return_logits else None
    _lib.check(_lib.load().pg_fvbn_sample(weight.data_ptr(), bias.data_ptr(), canvas.data_ptr(), uniforms.data_ptr(),
                                          None if logits is None else logits.data_ptr(), n, d, _stream()), "pg_fvbn_sample")
    return (canvas, logits) if return_logits else canvas
