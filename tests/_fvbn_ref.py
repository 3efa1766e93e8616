"""The FVBN in closed form, float64 on the CPU (the yardstick of tests/test_fvbn_cpu.py and tests/test_gpu_fvbn.py):

    logits = x tril(W, -1)^T + b,   dW = tril(G^T x, -1),   db = sum_n G        (G = dL/dlogits)

on a dense (D, D) matrix W, the packed layout restated in Python (off, pad, packed_floats, pack, unpack), the translation
between the packed pair and the reference's `_net.i.*` keys, and the sequential sampling chain."""

import torch


def row_len(i):
    return max(1, i)


def pad(i):
    return (row_len(i) + 3) // 4 * 4


def off(i):
    """Start of row i in the packed weight: sum_{k < i} pad(k)."""
    return sum(pad(k) for k in range(i))


def offsets(d):
    """[off(0), ..., off(d)] by one running sum."""
    out, total = [0], 0
    for k in range(d):
        total += pad(k)
        out.append(total)
    return out


def packed_floats(d):
    return offsets(d)[-1]


def pack(dense):
    """Packed weight of a dense (D, D) matrix: strict lower triangle, row 0's dummy value from [0, 0], zero pads."""
    d = dense.shape[0]
    offs = offsets(d)
    out = torch.zeros(offs[-1], dtype=dense.dtype)
    for i in range(d):
        out[offs[i]:offs[i] + row_len(i)] = dense[i, :row_len(i)]
    return out


def unpack(packed, d):
    """Dense (D, D) matrix of a packed weight: zeros on and above the diagonal except [0, 0]."""
    offs = offsets(d)
    out = torch.zeros(d, d, dtype=packed.dtype)
    for i in range(d):
        out[i, :row_len(i)] = packed[offs[i]:offs[i] + row_len(i)]
    return out


def pad_mask(d):
    """bool (P(D),): True at the pads."""
    offs = offsets(d)
    m = torch.ones(offs[-1], dtype=torch.bool)
    for i in range(d):
        m[offs[i]:offs[i] + row_len(i)] = False
    return m


def forward(x, w, b):
    """logits in float64 from the dense w (D, D): only its strict lower triangle is used."""
    return x.double() @ torch.tril(w.double(), -1).t() + b.double()


def grads(x, g):
    """(dW dense (D, D) with zeros on and above the diagonal, db) in float64 from g = dL/dlogits."""
    return torch.tril(g.double().t() @ x.double(), -1), g.double().sum(0)


def recipe_loss(x, logits):
    """binary_cross_entropy_with_logits summed per sample, averaged over the batch, and its gradient w.r.t. the logits."""
    n = x.shape[0]
    x, l = x.double().reshape(n, -1), logits.double().reshape(n, -1)
    loss = (l.clamp_min(0) - l * x + torch.log1p(torch.exp(-l.abs()))).sum(1).mean()
    return loss, (torch.sigmoid(l) - x) / n


def sample(canvas, w, b, uniforms):
    """The chain in float64: entries >= 0 are kept, the others are (u_i < sigmoid(l_i)). Returns (sample, logits)."""
    x = canvas.double().clone()
    w, b = torch.tril(w.double(), -1), b.double()
    logits = torch.empty_like(x)
    for i in range(x.shape[1]):
        logits[:, i] = b[i] + x[:, :i] @ w[i, :i]
        drawn = (uniforms[:, i].double() < torch.sigmoid(logits[:, i])).double()
        x[:, i] = torch.where(x[:, i] < 0, drawn, x[:, i])
    return x, logits


def state_to_dense(state, d):
    """(W dense (D, D) with row 0's dummy weight at [0, 0], b (D)) from the reference's `_net.i.*` keys."""
    w, b = torch.zeros(d, d, dtype=state["_net.0.weight"].dtype), torch.zeros(d, dtype=state["_net.0.bias"].dtype)
    for i in range(d):
        w[i, :row_len(i)] = state[f"_net.{i}.weight"][0]
        b[i] = state[f"_net.{i}.bias"][0]
    return w, b


def packed_to_keys(weight, bias, d):
    """{`_net.i.weight` (1, max(1, i)), `_net.i.bias` (1)} from the packed pair (values of any tensors of those layouts)."""
    offs = offsets(d)
    out = {}
    for i in range(d):
        out[f"_net.{i}.weight"] = weight[offs[i]:offs[i] + row_len(i)].reshape(1, -1)
        out[f"_net.{i}.bias"] = bias[i:i + 1]
    return out
