"""Plain-torch float64 restatement of the fused head + categorical likelihood (csrc/linear_categorical.hip):
logits = conv1x1(transform(h)), then tests/_categorical_ref.py for the loss, lse, the per-sample sums and dlogits, then
dW, db, dh, dln_w, dln_b by the chain rule written out by hand. tests/test_linear_categorical_cpu.py pins it against torch
autograd.

h (N, Cin, H, W); w (K * C, Cin) class-major; b (K * C) or None; images (N, C, H, W) at the levels j / (K - 1);
transform "none" | "relu" | "ln" (LayerNorm over the Cin channels, biased variance, eps inside the root)."""

import torch
import torch.nn.functional as F

import _categorical_ref as cref

TRANSFORMS = ("none", "relu", "ln")


def _stats(h, eps):
    mu = h.mean(dim=1, keepdim=True)
    var = ((h - mu) ** 2).mean(dim=1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + eps)
    return (h - mu) * rstd, rstd


def transformed(h, transform, ln_w=None, ln_b=None, eps=1e-5):
    h = h.double()
    if transform == "relu":
        return torch.clamp_min(h, 0.0)
    if transform == "ln":
        xhat, _ = _stats(h, eps)
        return xhat * ln_w.double().view(1, -1, 1, 1) + ln_b.double().view(1, -1, 1, 1)
    return h


def logits(h, w, b, transform, ln_w=None, ln_b=None, eps=1e-5):
    """(N, K * C, H, W) float64."""
    z = torch.einsum("oc,nchw->nohw", w.double(), transformed(h, transform, ln_w, ln_b, eps))
    return z if b is None else z + b.double().view(1, -1, 1, 1)


def everything(h, w, b, images, k, transform, ln_w=None, ln_b=None, eps=1e-5, grad_output=1.0):
    """dict of float64 tensors: loss, lse, per_sample, dh, dW, and db / dln_w / dln_b where they apply."""
    y = transformed(h, transform, ln_w, ln_b, eps)
    z = logits(h, w, b, transform, ln_w, ln_b, eps)
    loss, dz = cref.loss_and_grad(z, images, k, grad_output)
    out = {"loss": loss, "lse": cref.lse(z, k), "per_sample": cref.nll_per_sample(z, images, k).detach(),
           "dW": torch.einsum("nohw,nchw->oc", dz, y)}
    if b is not None:
        out["db"] = dz.sum(dim=(0, 2, 3))
    dy = torch.einsum("oc,nohw->nchw", w.double(), dz)
    if transform == "relu":
        out["dh"] = dy * (h.double() > 0)
    elif transform == "ln":
        xhat, rstd = _stats(h.double(), eps)
        out["dln_w"] = (dy * xhat).sum(dim=(0, 2, 3))
        out["dln_b"] = dy.sum(dim=(0, 2, 3))
        dxhat = dy * ln_w.double().view(1, -1, 1, 1)
        out["dh"] = rstd * (dxhat - dxhat.mean(dim=1, keepdim=True) - xhat * (dxhat * xhat).mean(dim=1, keepdim=True))
    else:
        out["dh"] = dy
    return out


def by_autograd(h, w, b, images, k, transform, ln_w=None, ln_b=None, eps=1e-5, grad_output=1.0):
    """The same quantities from torch's own operators and autograd in float64: F.layer_norm / relu -> F.conv2d ->
    F.cross_entropy on logits.view(N, K, C, H, W)."""
    leaf = lambda t: None if t is None else t.detach().double().requires_grad_(True)  # noqa: E731
    h, w, b, ln_w, ln_b = leaf(h), leaf(w), leaf(b), leaf(ln_w), leaf(ln_b)
    y = h
    if transform == "relu":
        y = F.relu(h)
    elif transform == "ln":
        y = F.layer_norm(h.permute(0, 2, 3, 1), (h.shape[1],), ln_w, ln_b, eps).permute(0, 3, 1, 2)
    z = F.conv2d(y, w.view(w.shape[0], w.shape[1], 1, 1), b)
    n, kc, hh, ww = z.shape
    zz = z.view(n, k, kc // k, hh, ww)
    ce = F.cross_entropy(zz, cref.classes(images, k), reduction="none")
    per_sample = ce.sum(dim=(1, 2, 3))
    loss = per_sample.mean()
    (loss * grad_output).backward()
    out = {"loss": loss.detach(), "lse": torch.logsumexp(zz, dim=1).detach(), "per_sample": per_sample.detach(),
           "dh": h.grad, "dW": w.grad}
    if b is not None:
        out["db"] = b.grad
    if transform == "ln":
        out["dln_w"], out["dln_b"] = ln_w.grad, ln_b.grad
    return out


def _draw_case(shape, transform, variant, bias, attempt):
    n, cin, k, c, hh, ww = shape
    seed = 100003 * n + 1009 * cin + 7 * k + 31 * c + 3 * hh * ww + 11 * TRANSFORMS.index(transform) + len(variant) + 2 * bias
    g = torch.Generator().manual_seed(seed + 7919 * attempt)
    h = torch.randn(n, cin, hh, ww, generator=g)
    w = torch.randn(k * c, cin, generator=g) * 1.5 / cin ** 0.5
    b = torch.randn(k * c, generator=g) * 0.5 if bias else None
    ln_w = ln_b = None
    if transform == "ln":
        ln_w = 1.0 + 0.3 * torch.randn(cin, generator=g)
        ln_b = 0.2 * torch.randn(cin, generator=g)
    if variant == "wide":
        w = w * 30
    elif variant == "equal":
        assert bias
        if c > 1:
            rows = w.view(k, c, cin)
            rows[:, ::2, :] = 0.0
            b.view(k, c)[:, ::2] = 5.0
        else:
            h.view(n, cin, hh * ww)[:, :, ::2] = 0.0
            if transform == "ln":
                ln_b = torch.zeros(cin)
            b[:] = 5.0
    t = torch.randint(0, k, (n, c, hh, ww), generator=g)
    t.view(-1)[0] = 0
    t.view(-1)[-1] = k - 1
    images = cref.to_level(t, k)
    assert torch.equal(cref.classes(images, k), t)
    return {"h": h, "w": w, "b": b, "ln_w": ln_w, "ln_b": ln_b, "eps": 1e-5, "images": images, "k": k, "transform": transform}


def well_posed(case):
    """A sub-pixel's term lse - z_t comes out of fp32 arithmetic on numbers of the logits' size: it carries an absolute error
    of a few ulp of max|z| (4 * 6e-8 * max|z|), whatever the kernel. The gate on the loss is 1e-5 RELATIVE to the loss, so a
    case tests the kernel rather than the number format only if that error is a fraction of the gate: a fifth of it needs
    loss >= 0.12 * max|z|. A one-sub-pixel image whose target happens to be near-certain has a loss near 0 and fails this."""
    z = logits(case["h"], case["w"], case["b"], case["transform"], case["ln_w"], case["ln_b"], case["eps"])
    loss = cref.nll_per_sample(z, case["images"], case["k"]).mean()
    return float(loss) >= 0.12 * float(z.abs().max())


def make_case(shape, transform, variant="plain", bias=True):
    """fp32 inputs of one case. shape = (N, Cin, K, C, H, W). variant: "plain"; "wide" (weights times 30: exp overflows without
    the max subtraction); "equal" (half the sub-pixels have K equal logits: for C > 1 the even channels have zero weight
    rows and a constant bias, for C = 1 the even pixels have zero transformed features and the bias is constant).
    Targets include class 0 and class K - 1. The first draw of the case's seed sequence that is well_posed() — a property
    of the float64 reference alone. Returns a dict: h, w, b, ln_w, ln_b, eps, images, k, transform."""
    for attempt in range(32):
        case = _draw_case(shape, transform, variant, bias, attempt)
        if well_posed(case):
            return case
    raise AssertionError(f"no well-posed draw for {shape} {transform} {variant}")


def reference(case, grad_output=1.0, fn=everything):
    return fn(case["h"], case["w"], case["b"], case["images"], case["k"], case["transform"], case["ln_w"], case["ln_b"],
              case["eps"], grad_output)
