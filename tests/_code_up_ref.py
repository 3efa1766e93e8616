"""Float64 restatement of the upsampling code lookup (csrc/code_up.hip) and of an ImageGPT that takes a coarser code image
as context:

    out[n, co, i f + a, j f + b] = base[n, co, i f + a, j f + b] + w[code(n, i, j), co, a, b]        w (K, Cout, f, f)

i.e. base + F.conv_transpose2d(one_hot(codes), w, stride = f) with kernel = stride = f. A code image is (N, 1, h, w) integer
codes in 0..K-1 with -1 = no code (a zero row: nothing is added), or float32 levels j / (K - 1) with a negative value for -1
(tests/_code_conv_ref.py: to_levels / to_codes / one_hot)."""

import torch
import torch.nn.functional as F

from _code_conv_ref import one_hot, to_codes, to_levels  # noqa: F401  (re-exported)
from oracle import models as omodels
from oracle import ops as oops


def code_upsample_ref(codes, w, f, base=None):
    """base + conv_transpose2d(one_hot(codes), w, stride=f) in float64; codes (N, 1, h, w) int, -1 = a zero row."""
    k = w.shape[0]
    assert tuple(w.shape[2:]) == (f, f)
    out = F.conv_transpose2d(one_hot(codes, k), w.double(), stride=f)
    return out if base is None else base.double() + out


def code_upsample_loop(codes, w, f, base=None):
    """The formula index by index."""
    n, _, h, wd = codes.shape
    k, cout = w.shape[:2]
    out = torch.zeros(n, cout, h * f, wd * f, dtype=torch.float64) if base is None else base.double().clone()
    for i_n in range(n):
        for i in range(h):
            for j in range(wd):
                c = int(codes[i_n, 0, i, j])
                if c < 0:
                    continue
                for a in range(f):
                    for b in range(f):
                        out[i_n, :, i * f + a, j * f + b] += w[c, :, a, b].double()
    return out


def code_upsample_wgrad_ref(codes, dy, k, f):
    """dw[k, co, a, b] = sum of dy[n, co, i f + a, j f + b] over the top positions with code(n, i, j) = k, by autograd
    through conv_transpose2d in float64."""
    cout = dy.shape[1]
    w = torch.zeros(k, cout, f, f, dtype=torch.float64, requires_grad=True)
    F.conv_transpose2d(one_hot(codes, k), w, stride=f).backward(dy.double())
    return w.grad


def code_upsample_wgrad_loop(codes, dy, k, f):
    n, _, h, wd = codes.shape
    cout = dy.shape[1]
    dw = torch.zeros(k, cout, f, f, dtype=torch.float64)
    for i_n in range(n):
        for i in range(h):
            for j in range(wd):
                c = int(codes[i_n, 0, i, j])
                if c >= 0:
                    dw[c] += dy[i_n, :, i * f:(i + 1) * f, j * f:(j + 1) * f].double()
    return dw


def image_gpt_cond(p, x_onehot, cond_codes, n_heads, f):
    """oracle.models.image_gpt with the lookup of the context added after the stem: p holds `_cond.weight` (K, C, f, f),
    cond_codes (N, 1, H / f, W / f) int codes."""
    n_blocks = 1 + max(int(k.split(".")[1]) for k in p if k.startswith("_transformer."))
    c = p["_input.weight"].shape[0]
    h = omodels._cconv(x_onehot + p["_pos"], p, "_input", True, 1)
    h = h + F.conv_transpose2d(one_hot(cond_codes, p["_cond.weight"].shape[0]), p["_cond.weight"], stride=f)
    for i in range(n_blocks):
        pre = f"_transformer.{i}."
        b = h
        a = oops.nchw_layernorm(b, p[pre + "_ln1.weight"], p[pre + "_ln1.bias"])
        b = b + oops.causal_attention(a, None, p, pre + "_attn.", n_heads, c, False)
        m = oops.nchw_layernorm(b, p[pre + "_ln2.weight"], p[pre + "_ln2.bias"])
        m = omodels._conv(F.gelu(omodels._conv(m, p, pre + "_out.0")), p, pre + "_out.2")
        h = h + (b + m)
    return omodels._conv(oops.nchw_layernorm(h, p["_ln.weight"], p["_ln.bias"]), p, "_out")
