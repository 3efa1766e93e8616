"""Float64 restatement of the code-index convolution (csrc/code_conv.hip), written out as loops: the forward is a gather,
the weight gradient a scatter over ALL kh * kw taps (the reference's weight gradient is unmasked).

A code image is (N, 1, H, W) integer codes in 0..K-1 with -1 = no code (the all-zero one-hot vector), or the same as
float32 levels j / (K - 1) with any negative value for -1."""

import torch
import torch.nn.functional as F


def causal_mask(kh, kw, mask_center):
    """The 0 / 1 mask of CausalConv2d over one (kh, kw) kernel."""
    m = torch.zeros(kh, kw, dtype=torch.float64)
    m[: kh // 2, :] = 1.0
    m[kh // 2, : kw // 2 + (0 if mask_center else 1)] = 1.0
    return m


def to_levels(codes, k):
    """int codes (-1 allowed) -> fp32 levels j / (K - 1), -1 stays -1."""
    lv = codes.to(torch.float32) / float(k - 1)
    return torch.where(codes < 0, torch.full_like(lv, -1.0), lv)


def to_codes(levels, k):
    """fp32 levels -> int64 codes as the kernels decode them: negative = -1, else clamp(rint(x (K - 1)), 0, K - 1)."""
    c = torch.clamp(torch.round(levels.float() * float(k - 1)), 0, k - 1).long()
    return torch.where(levels < 0, torch.full_like(c, -1), c)


def one_hot(codes, k):
    """(N, 1, H, W) int codes -> (N, K, H, W) float64, all-zero where the code is -1."""
    n, _, h, w = codes.shape
    oh = torch.zeros(n, k, h, w, dtype=torch.float64)
    valid = codes >= 0
    oh.scatter_(1, codes.clamp_min(0), valid.to(torch.float64))
    return oh


def forward(codes, weight, bias, pad, mask=None, out_hw=None):
    """out[n, :, y, x] = b + sum_{(u, v): mask[u, v] != 0} W[:, code(n, y + u - ph, x + v - pw), u, v]. float64."""
    n, _, h, w = codes.shape
    cout, k, kh, kw = weight.shape
    ph, pw = pad
    oh, ow = out_hw if out_hw is not None else (h + 2 * ph - kh + 1, w + 2 * pw - kw + 1)
    wd = weight.double()
    out = torch.zeros(n, cout, oh, ow, dtype=torch.float64)
    if bias is not None:
        out += bias.double().view(1, cout, 1, 1)
    for i in range(n):
        for y in range(oh):
            for x in range(ow):
                for u in range(kh):
                    for v in range(kw):
                        if mask is not None and mask[u, v] == 0:
                            continue
                        iy, ix = y + u - ph, x + v - pw
                        if 0 <= iy < h and 0 <= ix < w:
                            c = int(codes[i, 0, iy, ix])
                            if c >= 0:
                                out[i, :, y, x] += wd[:, c, u, v]
    return out


def wgrad(codes, dy, k, kernel, pad):
    """(dW (Cout, K, kh, kw), db (Cout)) in float64: a scatter of dY rows by code, every tap."""
    n, _, h, w = codes.shape
    _, cout, oh, ow = dy.shape
    kh, kw = kernel
    ph, pw = pad
    d = dy.double()
    dw = torch.zeros(cout, k, kh, kw, dtype=torch.float64)
    for i in range(n):
        for y in range(oh):
            for x in range(ow):
                for u in range(kh):
                    for v in range(kw):
                        iy, ix = y + u - ph, x + v - pw
                        if 0 <= iy < h and 0 <= ix < w:
                            c = int(codes[i, 0, iy, ix])
                            if c >= 0:
                                dw[:, c, u, v] += d[i, :, y, x]
    return dw, d.sum(dim=(0, 2, 3))


def dense(codes, weight, bias, pad, mask=None, out_hw=None):
    """The same numbers from F.conv2d(one_hot, weight * mask) in float64, with autograd for the gradients (the weight
    gradient of the MASKED product with respect to the product, i.e. unmasked, is what wgrad() restates)."""
    k = weight.shape[1]
    w = weight.double() if mask is None else weight.double() * mask.view(1, 1, *mask.shape)
    out = F.conv2d(one_hot(codes, k), w, None if bias is None else bias.double(), padding=pad)
    if out_hw is not None:
        out = out[:, :, : out_hw[0], : out_hw[1]]
    return out


def dense_wgrad(codes, dy, k, kernel, pad):
    """wgrad() by autograd through F.conv2d(one_hot, w) in float64 (fast at the larger test shapes)."""
    cout = dy.shape[1]
    w = torch.zeros(cout, k, *kernel, dtype=torch.float64, requires_grad=True)
    out = F.conv2d(one_hot(codes, k), w, None, padding=pad)[:, :, : dy.shape[2], : dy.shape[3]]
    out.backward(dy.double())
    return w.grad, dy.double().sum(dim=(0, 2, 3))
