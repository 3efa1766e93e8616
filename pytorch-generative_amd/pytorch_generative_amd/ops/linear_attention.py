"""ops.linear_attention — linear causal attention (O(L) memory) on the chunked-scan kernels of csrc/linear_attention.hip.

Part of the operator layer (pytorch_generative_amd.ops): HIP kernels behind torch.autograd.Function, called through the C-ABI
with tensor.data_ptr() and the current stream. No CPU / ATen fallback: a missing library, a CPU tensor or an unsupported shape raises."""

import torch

from pytorch_generative_amd import _lib
from pytorch_generative_amd.ops._common import _chk, _stream

FEATURE_IDENTITY, FEATURE_ELU1 = 0, 1  # include/pg_hip.h PG_FEATURE_*
_FEATURES = {"identity": FEATURE_IDENTITY, "elu1": FEATURE_ELU1}


def _workspace(lib, n, n_heads, L, dk, dv, backward, device):
    floats = int(lib.pg_linear_attn_workspace_floats(n, n_heads, L, dk, dv, int(backward)))
    return torch.empty(max(floats, 1), device=device, dtype=torch.float32), floats


class _LinearCausalAttention(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, kv, n_heads, embed, vdim, feature):
        lib = _lib.load()
        q = _chk(q, "linear_attention.q")
        kv = _chk(kv, "linear_attention.kv")
        n, e, h, w = q.shape
        if e != embed or kv.shape[1] != embed + vdim or tuple(kv.shape[2:]) != (h, w) or kv.shape[0] != n:
            raise ValueError("linear_attention: shape mismatch between q / kv and embed / value dims")
        if embed % n_heads or vdim % n_heads:
            raise ValueError("linear_attention: channels not divisible by n_heads")
        L = h * w
        dk, dv = embed // n_heads, vdim // n_heads
        out = torch.empty((n, vdim, h, w), device=q.device, dtype=torch.float32)
        den = torch.empty((n, n_heads, L), device=q.device, dtype=torch.float32)
        ws, ws_floats = _workspace(lib, n, n_heads, L, dk, dv, False, q.device)
        kvs = (embed + vdim) * L
        _lib.check(
            lib.pg_linear_attn_fwd(q.data_ptr(), kv.data_ptr(), kv.data_ptr() + 4 * embed * L, out.data_ptr(),
                                   den.data_ptr(), ws.data_ptr(), ws_floats, n, n_heads, L, dk, dv, embed * L, kvs,
                                   vdim * L, feature, _stream()),
            "pg_linear_attn_fwd",
        )
        ctx.save_for_backward(q, kv, out, den)
        ctx.cfg = (n_heads, embed, vdim, feature)
        return out

    @staticmethod
    def backward(ctx, g):
        lib = _lib.load()
        q, kv, out, den = ctx.saved_tensors
        n_heads, embed, vdim, feature = ctx.cfg
        g = _chk(g, "linear_attention.g")
        n, _, h, w = q.shape
        L = h * w
        dk, dv = embed // n_heads, vdim // n_heads
        dq = torch.empty_like(q)
        dkv = torch.empty_like(kv)
        ws, ws_floats = _workspace(lib, n, n_heads, L, dk, dv, True, q.device)
        kvs = (embed + vdim) * L
        _lib.check(
            lib.pg_linear_attn_bwd(q.data_ptr(), kv.data_ptr(), kv.data_ptr() + 4 * embed * L, out.data_ptr(),
                                   den.data_ptr(), g.data_ptr(), dq.data_ptr(), dkv.data_ptr(),
                                   dkv.data_ptr() + 4 * embed * L, ws.data_ptr(), ws_floats, n, n_heads, L, dk, dv,
                                   embed * L, kvs, vdim * L, feature, _stream()),
            "pg_linear_attn_bwd",
        )
        return dq, dkv, None, None, None, None


def linear_causal_attention(q, kv, n_heads, embed, vdim, feature="elu1"):
    """LinearCausalAttention's core (reference nn/attention.py:256-275) on q (N, embed, H, W) and kv = cat(k, v)
    (N, embed + vdim, H, W): out[l] = phi(q[l]) . sum_{j <= l} phi(k[j])^T v[j] * den[l], with the reference's
    denominator (cumsum of phi(k) over the HEADS axis, include/pg_hip.h). feature: "elu1" (phi = elu + 1, applied
    inside the kernels) or "identity" (q and k already mapped by the caller). Returns (N, vdim, H, W)."""
    if feature not in _FEATURES:
        raise ValueError(f"linear_attention: feature must be one of {sorted(_FEATURES)}, got {feature!r}")
    return _LinearCausalAttention.apply(q, kv, int(n_heads), int(embed), int(vdim), _FEATURES[feature])
