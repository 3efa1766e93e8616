"""NADE in closed form, float64 on the CPU (the yardstick of tests/test_nade_cpu.py and tests/test_gpu_nade.py):

    a_i = in_b + sum_{j < i} x_j in_w[:, j]      (exclusive cumulative sum)
    l_i = h_b[i] + relu(a_i) . h_w[i, :],  p_i = sigmoid(l_i)

and the gradients of the four parameters from G = dL/dp by the formulas of the model's derivation (no autograd):
delta = G p (1 - p); d_h_b = sum_n delta; d_h_w[i] = sum_n delta_i relu(a_i); e_i = delta_i h_w[i] [a_i > 0];
S_j = sum_{i > j} e_i; d_in_w[:, j] = sum_n x_j S_j; d_in_b = sum_n sum_i e_i."""

import torch

KEYS = ("_in_W", "_in_b", "_h_W", "_h_b")


def preact(x, in_w, in_b, dtype=torch.float64):
    """a (N, D, H): the pre-activation dimension i sees, by the exclusive cumulative sum."""
    x, in_w, in_b = x.to(dtype), in_w.to(dtype), in_b.to(dtype)
    terms = x[:, :, None] * in_w.t()[None]
    return in_b + torch.cumsum(terms, 1) - terms


def recurrence(x, in_w, in_b, dtype):
    """a (N, D, H) by the sequential recurrence a_{i+1} = a_i + x_i in_w[:, i] in `dtype` (what the kernels walk)."""
    x, in_w = x.to(dtype), in_w.to(dtype)
    a = in_b.to(dtype).expand(x.shape[0], -1).clone()
    out = []
    for i in range(x.shape[1]):
        out.append(a.clone())
        a = a + x[:, i:i + 1] * in_w[:, i][None]
    return torch.stack(out, 1)


def forward(x, in_w, in_b, h_w, h_b):
    """(p, logits, a) in float64."""
    a = preact(x, in_w, in_b)
    logits = h_b.double() + (torch.relu(a) * h_w.double()[None]).sum(-1)
    return torch.sigmoid(logits), logits, a


def grads(x, in_w, in_b, h_w, h_b, g):
    """{key: gradient} of the four parameters from g = dL/dp, float64."""
    p, _, a = forward(x, in_w, in_b, h_w, h_b)
    x, g = x.double(), g.double()
    delta = g * p * (1 - p)
    e = delta[:, :, None] * h_w.double()[None] * (a > 0)
    s = torch.flip(torch.cumsum(torch.flip(e, [1]), 1), [1]) - e
    return {"_h_b": delta.sum(0), "_h_W": torch.einsum("ni,nih->ih", delta, torch.relu(a)),
            "_in_W": torch.einsum("nj,njh->hj", x, s), "_in_b": e.sum((0, 1))}


def recipe_loss(x, p):
    """The recipe's loss and its gradient with respect to p: binary_cross_entropy_with_logits applied to the probabilities
    (the reference's quirk), summed per sample, averaged over the batch."""
    x, p = x.double().reshape(x.shape[0], -1), p.double().reshape(x.shape[0], -1)
    loss = (p.clamp_min(0) - p * x + torch.log1p(torch.exp(-p.abs()))).sum(1).mean()
    return loss, (torch.sigmoid(p) - x) / x.shape[0]


def adam_first_step(param, grad, lr=1e-3, eps=1e-8):
    """torch.optim.Adam's first step from zero moments: the bias corrections cancel the (1 - beta) factors."""
    grad = grad.double()
    return param.double() - lr * grad / (grad.abs() + eps)


def sample(canvas, in_w, in_b, h_w, h_b, uniforms):
    """The chain in float64: entries >= 0 are kept, the others are (u_i < p_i). Returns (sample, logits)."""
    x = canvas.double().clone()
    in_w, h_w, h_b = in_w.double(), h_w.double(), h_b.double()
    a = in_b.double().expand(x.shape[0], -1).clone()
    logits = torch.empty_like(x)
    for i in range(x.shape[1]):
        logits[:, i] = h_b[i] + torch.relu(a) @ h_w[i]
        drawn = (uniforms[:, i].double() < torch.sigmoid(logits[:, i])).double()
        x[:, i] = torch.where(x[:, i] < 0, drawn, x[:, i])
        a = a + x[:, i:i + 1] * in_w[:, i][None]
    return x, logits
