"""Float64 restatement, in plain torch, of the one-launch MADE sampler (csrc/made_sample.hip, ops.made_sample_chain): the chain
on cached hidden sums, the full masked forward it must agree with, and the distance of every draw from its threshold."""

import numpy as np
import torch


def chain(canvas, w1, b1, w2, b2, order, uniforms, dtype=torch.float64):
    """canvas, uniforms (N, D); w1 (H, D), w2 (D, H) ALREADY masked; order: the dimension of each step. Returns (sample, logits)
    in `dtype`: per sample a = b1, then for i in order: l = b2[i] + relu(a) . w2[i]; x_i = canvas[:, i] where that is >= 0, else
    (u_i < sigmoid(l)); a += x_i w1[:, i]."""
    x = canvas.to(dtype).clone()
    w1, b1, w2, b2, u = (t.to(dtype) for t in (w1, b1, w2, b2, uniforms))
    n, d = x.shape
    a = b1[None, :].repeat(n, 1)
    logits = torch.zeros(n, d, dtype=dtype)
    for i in (int(v) for v in order):
        l = b2[i] + torch.relu(a) @ w2[i]
        p = 1.0 / (1.0 + torch.exp(-l))
        xi = torch.where(x[:, i] >= 0, x[:, i], (u[:, i] < p).to(dtype))
        x[:, i] = xi
        logits[:, i] = l
        a += xi[:, None] * w1[:, i][None, :]
    return x, logits


def forward(x, w1, b1, w2, b2, dtype=torch.float64):
    """One full forward of the masked network: relu(x w1^T + b1) w2^T + b2."""
    x, w1, b1, w2, b2 = (t.to(dtype) for t in (x, w1, b1, w2, b2))
    return torch.relu(x @ w1.t() + b1) @ w2.t() + b2


def draw_margin(canvas, logits, uniforms):
    """min |u - sigmoid(l)| over the DRAWN entries (canvas < 0) in float64; inf when everything is given."""
    drawn = canvas < 0
    if not bool(drawn.any()):
        return float("inf")
    p = 1.0 / (1.0 + torch.exp(-logits.double()))
    return float((uniforms.double() - p).abs()[drawn].min())


def masked_net(d, h, seed, mask_index=0, scale=1.0):
    """A random one-hidden-layer MADE as the kernel sees it: (w1 (H, D), b1, w2 (D, H), b2) float32 with the masks of
    `mask_index` applied (exact zeros), and the int32 order argsort(ordering) of that index."""
    from pytorch_generative_amd.models.autoregressive import made

    g = torch.Generator().manual_seed(seed)
    w1 = torch.randn(h, d, generator=g) * (scale / max(d, 1) ** 0.5)
    b1 = torch.randn(h, generator=g) * 0.3
    w2 = torch.randn(d, h, generator=g) * (2.0 * scale / max(h, 1) ** 0.5)
    b2 = torch.randn(d, generator=g) * 0.5
    if d == 1:  # the reference cannot draw degrees for one dimension (randint(0, 0)): the only autoregressive choice by hand
        conn = [np.zeros(1, dtype=np.int64), np.zeros(h, dtype=np.int64), np.zeros(1, dtype=np.int64)]
    else:
        conn = made.connectivity(d, [d, h, d], mask_index)
    m1, m2 = (m.float() for m in made.masks_from_connectivity(conn))
    order = torch.from_numpy(np.argsort(conn[-1]).astype(np.int32))
    return w1 * m1, b1, w2 * m2, b2, order


GIVENS = ("none", "some", "all")


def start_canvas(n, d, givens, seed):
    """(canvas, uniforms): nothing given, about 30 % given (half of those real values in [0, 1], the rest 0 / 1), or everything."""
    g = torch.Generator().manual_seed(seed + 7919)
    uniforms = torch.rand(n, d, generator=g)
    values = torch.where(torch.rand(n, d, generator=g) < 0.5, torch.rand(n, d, generator=g),
                         torch.bernoulli(torch.full((n, d), 0.5), generator=g))
    keep = {"none": torch.zeros(n, d, dtype=torch.bool), "some": torch.rand(n, d, generator=g) < 0.3,
            "all": torch.ones(n, d, dtype=torch.bool)}[givens]
    return torch.where(keep, values, torch.full((n, d), -1.0)), uniforms
