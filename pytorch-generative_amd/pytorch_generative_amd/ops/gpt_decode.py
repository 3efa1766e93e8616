"""ops.gpt_decode — one raster position of all transformer blocks of ImageGPT in one launch (csrc/gpt_decode.hip): the block
part of the K/V-cached sampler at any width.

Part of the operator layer (pytorch_generative_amd.ops): a HIP kernel called through the C-ABI with tensor.data_ptr() and the
current stream. Inference only (sample() runs under no_grad). No CPU / ATen fallback: a missing library, a CPU tensor or an
unsupported shape raises."""

import ctypes

import torch

from pytorch_generative_amd import _lib
from pytorch_generative_amd.ops._common import _chk, _stream

FIELDS = ("ln1_w", "ln1_b", "wqkv", "bqkv", "wproj", "bproj", "ln2_w", "ln2_b", "w1", "b1", "w2", "b2")  # PG_GD_*
PLAN_INTS = 16  # PG_GPT_DECODE_PLAN_INTS


def gpt_decode_plan(channels, heads, blocks, seq_len):
    """The planner's answer (pg_gpt_decode_plan, host only): None for a shape it refuses, else a dict with the pack size and
    the floats per block, the LDS bytes and threads of a workgroup and the offset of every parameter inside a block."""
    out = (ctypes.c_int * PLAN_INTS)()
    rc = _lib.load().pg_gpt_decode_plan(int(channels), int(heads), int(blocks), int(seq_len), out, PLAN_INTS)
    if rc:
        return None
    return {"pack_floats": out[0], "block_floats": out[1], "lds_bytes": out[2], "threads": out[3],
            "offsets": dict(zip(FIELDS, out[4:4 + len(FIELDS)]))}


def _block_dims(blk):
    """(channels, heads, eps, strict) of a TransformerBlock the step kernel can run, None for any other module layout."""
    attn = getattr(blk, "_attn", None)
    try:
        q, kv, proj, fc1, fc2 = attn._q, attn._kv, attn._proj, blk._out[0], blk._out[2]
        c = q.weight.shape[1]
        ok = (attn._embed_channels == c and attn._out_channels == c
              and tuple(q.weight.shape) == (c, c, 1, 1) and tuple(kv.weight.shape) == (2 * c, c, 1, 1)
              and tuple(proj.weight.shape) == (c, c, 1, 1) and tuple(fc1.weight.shape) == (4 * c, c, 1, 1)
              and tuple(fc2.weight.shape) == (c, 4 * c, 1, 1)
              and all(m.bias is not None for m in (q, kv, proj, fc1, fc2))
              and all(tuple(ln.normalized_shape) == (c,) and ln.elementwise_affine and ln.bias is not None
                      for ln in (blk._ln1, blk._ln2))
              and blk._ln1.eps == blk._ln2.eps)
    except (AttributeError, IndexError, TypeError):
        return None
    return (c, attn._n_heads, float(blk._ln1.eps), int(bool(attn._mask_center))) if ok else None


def gpt_decode_supported(model_or_dims):
    """Whether the step kernel runs the block stack: asks the planner. `model_or_dims` is (channels, heads, blocks, seq_len)
    or an ImageGPT, whose blocks must then all have one layout (C -> C attention with biases, a 4C hidden layer)."""
    if isinstance(model_or_dims, (tuple, list)):
        c, heads, blocks, seq_len = model_or_dims
        return gpt_decode_plan(c, heads, blocks, seq_len) is not None
    model = model_or_dims
    dims = [_block_dims(blk) for blk in model._transformer]
    if not dims or dims[0] is None or any(d != dims[0] for d in dims):
        return False
    c, heads = dims[0][:2]
    if model._input.weight.shape[0] != c or heads <= 0 or c % heads:
        return False
    seq_len = model._pos.shape[2] * model._pos.shape[3]
    return gpt_decode_plan(c, heads, len(dims), seq_len) is not None


def gpt_decode_pack(blocks):
    """The parameters of `blocks` (TransformerBlocks of one layout) as the kernel's one float buffer: per block the fields
    of the plan, every weight matrix transposed to (in, out). Plain torch ops, once per sample() call."""
    blocks = list(blocks)
    dims = _block_dims(blocks[0])
    if dims is None or any(_block_dims(b) != dims for b in blocks):
        raise ValueError("gpt_decode_pack: blocks outside the step kernel's layout")
    c = dims[0]
    parts = []
    for blk in blocks:
        a = blk._attn
        t = lambda conv: conv.weight.detach().reshape(conv.weight.shape[0], -1).t()  # noqa: E731  (out, in) -> (in, out)
        parts += [blk._ln1.weight, blk._ln1.bias,
                  torch.cat((t(a._q), t(a._kv)), dim=1), torch.cat((a._q.bias, a._kv.bias)),
                  t(a._proj), a._proj.bias, blk._ln2.weight, blk._ln2.bias,
                  t(blk._out[0]), blk._out[0].bias, t(blk._out[2]), blk._out[2].bias]
    pack = torch.cat([p.detach().reshape(-1).float() for p in parts]).contiguous()
    if pack.numel() != len(blocks) * (12 * c * c + 13 * c):
        raise RuntimeError("gpt_decode_pack: pack size differs from the layout")
    return pack


def gpt_decode_step(x, pack, k_cache, v_cache, pos, *, heads, strict=0, eps=1e-5, out=None):
    """x (C, ld) -> the activations after the last block, same layout (`out`, default: x itself, in place). k_cache, v_cache:
    (blocks, n, C, L) with n <= ld; column `pos` of every block is written. `pos`: the raster position as an int, or a
    one-element int32 device tensor (clamped to the sequence by the kernel: one captured graph replays per position)."""
    out = x if out is None else out
    if not all(t.is_contiguous() for t in (x, out, k_cache, v_cache)):
        raise ValueError("gpt_decode_step: x, out and the caches are written or read in place and must be contiguous")
    x, out, pack, k_cache, v_cache = (_chk(t, "gpt_decode_step.operand") for t in (x, out, pack, k_cache, v_cache))
    c, ld = x.shape[-2] if x.dim() == 2 else x.shape[1], x.shape[-1]
    blocks, n, cc, seq_len = k_cache.shape
    if cc != c or k_cache.shape != v_cache.shape or x.numel() != c * ld or out.shape != x.shape:
        raise ValueError("gpt_decode_step: x, out and the caches disagree on their shapes")
    if pack.numel() != blocks * (12 * c * c + 13 * c):
        raise ValueError("gpt_decode_step: pack size differs from the plan's")
    on_device = torch.is_tensor(pos)
    if on_device and (pos.dtype != torch.int32 or not pos.is_cuda or pos.numel() != 1):
        raise ValueError("gpt_decode_step: pos must be an int or a one-element int32 device tensor")
    _lib.check(_lib.load().pg_gpt_decode_step(x.data_ptr(), out.data_ptr(), pack.data_ptr(), k_cache.data_ptr(),
                                              v_cache.data_ptr(), n, c, int(heads), blocks, seq_len, ld,
                                              0 if on_device else int(pos), int(strict), float(eps),
                                              pos.data_ptr() if on_device else None, _stream()), "pg_gpt_decode_step")
    return out
