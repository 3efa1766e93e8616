"""ops.attention_row — the attention half of the row-cached sampler on K / V caches (csrc/attention_row.hip): the queries of
one image row against the cached rows above it, the row index taken from the host or from a device int.

Part of the operator layer (pytorch_generative_amd.ops): HIP kernels called through the C-ABI with tensor.data_ptr() and the
current stream. Inference only (sample() runs under no_grad). No CPU / ATen fallback: a missing library, a CPU tensor or an
unsupported shape raises."""

import ctypes

import torch

from pytorch_generative_amd import _lib
from pytorch_generative_amd.ops._common import _chk, _stream

PLAN_INTS = 6  # PG_ATTN_ROW_PLAN_INTS


def attention_row_plan(heads, dk, dv, height, width):
    """The planner's answer (pg_attn_row_plan, host only): None for a shape it refuses, else the launch geometry."""
    out = (ctypes.c_int * PLAN_INTS)()
    rc = _lib.load().pg_attn_row_plan(int(heads), int(dk), int(dv), int(height), int(width), out, PLAN_INTS)
    if rc:
        return None
    return {"threads": out[0], "lds_bytes": out[1], "key_tile": out[2], "grid": (out[3], out[4]), "queries": out[5]}


def attention_row_supported(heads, dk, dv, height, width):
    """Whether pg_attn_row runs the shape (per-head key / value widths, image size): asks the planner."""
    if min(int(heads), int(dk), int(dv), int(height), int(width)) <= 0:
        return False
    return attention_row_plan(heads, dk, dv, height, width) is not None


def _row_arg(row, name):
    """(host row, device pointer or None) of a row index given as an int or a one-element int32 device tensor."""
    if torch.is_tensor(row):
        if row.dtype != torch.int32 or not row.is_cuda or row.numel() != 1:
            raise ValueError(f"{name}: row must be an int or a one-element int32 device tensor")
        return 0, row.data_ptr()
    return int(row), None


def attention_row(q_row, kv_row, k_cache, v_cache, heads, mask_center, *, row, write_cache=True):
    """q_row (N, heads*dk, 1, W), kv_row (N, heads*dk + heads*dv, 1, W), keys first -> o (N, heads*dv, 1, W): attention of
    the row's queries over cache rows < row and the row's own keys up to each query (itself excluded with mask_center).
    k_cache (N, heads*dk, H, W) and v_cache (N, heads*dv, H, W) are used in place; with write_cache their row `row` receives
    kv_row. `row`: an int, or a one-element int32 device tensor (clamped to the image by the kernel: one captured graph
    replays for every row)."""
    if not (k_cache.is_contiguous() and v_cache.is_contiguous()):
        raise ValueError("attention_row: the caches are written in place and must be contiguous")
    q_row, kv_row, k_cache, v_cache = (_chk(t, "attention_row.operand") for t in (q_row, kv_row, k_cache, v_cache))
    heads = int(heads)
    if q_row.dim() != 4 or kv_row.dim() != 4 or k_cache.dim() != 4 or v_cache.dim() != 4 or heads <= 0:
        raise ValueError("attention_row: operands must be 4-D (N, C, H, W) tensors and heads positive")
    n, e, one, w = q_row.shape
    _, o, h, _ = v_cache.shape
    if (one != 1 or tuple(kv_row.shape) != (n, e + o, 1, w) or tuple(k_cache.shape) != (n, e, h, w)
            or tuple(v_cache.shape) != (n, o, h, w) or e % heads or o % heads):
        raise ValueError(f"attention_row: q_row {tuple(q_row.shape)}, kv_row {tuple(kv_row.shape)}, k_cache "
                         f"{tuple(k_cache.shape)}, v_cache {tuple(v_cache.shape)} disagree for {heads} heads")
    r, r_dev = _row_arg(row, "attention_row")
    out = torch.empty((n, o, 1, w), device=q_row.device, dtype=torch.float32)
    _lib.check(_lib.load().pg_attn_row(q_row.data_ptr(), kv_row.data_ptr(), k_cache.data_ptr(), v_cache.data_ptr(),
                                       out.data_ptr(), n, heads, e // heads, o // heads, h, w, r, int(bool(mask_center)),
                                       int(bool(write_cache)), r_dev, _stream()), "pg_attn_row")
    return out


def row_gather(src, row):
    """src (N, C, H, W) -> src[:, :, row:row + 1] as a new contiguous tensor; `row` as in attention_row."""
    src = _chk(src, "row_gather.src")
    if src.dim() != 4:
        raise ValueError("row_gather: src must be (N, C, H, W)")
    n, c, h, w = src.shape
    r, r_dev = _row_arg(row, "row_gather")
    out = torch.empty((n, c, 1, w), device=src.device, dtype=torch.float32)
    _lib.check(_lib.load().pg_row_gather(src.data_ptr(), out.data_ptr(), n, c, h, w, r, r_dev, _stream()), "pg_row_gather")
    return out
