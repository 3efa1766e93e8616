"""The log marginal likelihood of the Gaussian process restated for the tests in float64: the closed forms of the value and of
its gradients with respect to std, lengthscale, noise_var and the constant mean; the same through autograd; the triangular
inverse, its product and the three sums of the reduction from given operands; and the Adam loop on the log-hyperparameters
that GaussianProcess.optimize_hyperparameters runs."""

import math

import torch

import _gp_ref as gref

NAMES = ("std", "lengthscale", "noise_var", "value")


def sq_dists(x):
    x = x.double()
    return ((x[:, None, :] - x[None, :, :]) ** 2).sum(-1)


def log_evidence(train_x, train_y, std, lengthscale, noise_var, value):
    """log p(y) in float64 from torch.linalg.cholesky; the hyperparameters may be float64 tensors that require grad."""
    x, y = train_x.double(), train_y.double()
    n, p = y.shape
    k = std ** 2 * torch.exp(-sq_dists(x) / (2.0 * lengthscale ** 2)) + noise_var * torch.eye(n, dtype=torch.float64)
    l = torch.linalg.cholesky(k)
    z = torch.linalg.solve_triangular(l, y - value, upper=False)
    return -0.5 * (z ** 2).sum() - p * torch.log(torch.diagonal(l)).sum() - 0.5 * n * p * math.log(2.0 * math.pi)


def closed_form(train_x, train_y, std, lengthscale, noise_var, value):
    """(log p(y), {name: gradient}) by the closed forms: G = alpha alpha^T - p K^-1, d/d std = sum G K_f / std,
    d/d lengthscale = sum G K_f D2 / (2 l^3), d/d noise_var = tr G / 2, d/d value = sum alpha."""
    x, y = train_x.double(), train_y.double()
    n, p = y.shape
    d2 = sq_dists(x)
    kf = std ** 2 * torch.exp(-d2 / (2.0 * lengthscale ** 2))
    l = torch.linalg.cholesky(kf + noise_var * torch.eye(n, dtype=torch.float64))
    z = torch.linalg.solve_triangular(l, y - value, upper=False)
    alpha = torch.linalg.solve_triangular(l.t(), z, upper=True)
    value_ = -0.5 * (z ** 2).sum() - p * torch.log(torch.diagonal(l)).sum() - 0.5 * n * p * math.log(2.0 * math.pi)
    g = alpha @ alpha.t() - p * torch.cholesky_inverse(l)
    grads = {"std": (g * kf).sum() / std, "lengthscale": (g * kf * d2).sum() / (2.0 * lengthscale ** 3), "noise_var": 0.5 * torch.trace(g),
             "value": alpha.sum()}
    return value_, grads


def autograd_form(train_x, train_y, std, lengthscale, noise_var, value):
    """The same pair from float64 autograd through torch.linalg.cholesky."""
    leaves = [torch.tensor(float(v), dtype=torch.float64, requires_grad=True) for v in (std, lengthscale, noise_var, value)]
    out = log_evidence(train_x, train_y, *leaves)
    out.backward()
    return out.detach(), dict(zip(NAMES, (leaf.grad for leaf in leaves)))


def tri_inverse_t(l):
    """l^-T of the lower triangle of l, float64 (upper triangular)."""
    l = l.double().tril()
    return torch.linalg.solve_triangular(l, torch.eye(l.shape[0], dtype=torch.float64), upper=False).t()


def gram_upper(x):
    x = x.double().triu()
    return x @ x.t()


def se_sums(x, std, lengthscale, h, alpha_t):
    """(sums, magnitudes): the three outputs of ops.se_mll_sums in float64 from the given operands (h is read on its lower
    triangle and mirrored), and for each the sum of the absolute values of its terms, the magnitude before cancellation."""
    d2 = sq_dists(x)
    kf = std ** 2 * torch.exp(-d2 / (2.0 * lengthscale ** 2))
    h = h.double().tril()
    h = h + h.tril(-1).t()
    a = alpha_t.double()
    g = a.t() @ a - a.shape[0] * h
    terms = (g * kf / std, g * kf * d2 / (2.0 * lengthscale ** 3), 0.5 * torch.diagonal(g))
    return torch.stack([t.sum() for t in terms]), torch.stack([t.abs().sum() for t in terms])


def value_sums(l, zt, alpha_t):
    """(log p(y), sum alpha) from a factor, z^T and alpha^T, float64."""
    l, zt = l.double(), zt.double()
    p, n = zt.shape
    return torch.stack([-0.5 * (zt ** 2).sum() - p * torch.log(torch.diagonal(l)).sum() - 0.5 * n * p * math.log(2.0 * math.pi),
                        alpha_t.double().sum()])


def adam_loop(train_x, train_y, start, n_steps=50, lr=0.05, learn_noise=True, learn_mean=True):
    """torch.optim.Adam ascending log p(y) on log std, log lengthscale, log noise_var and value, float64, from
    start = (std, lengthscale, noise_var, value). Returns (the values seen, the final hyperparameters in that order)."""
    std, lengthscale, noise_var, value = (float(v) for v in start)
    logs = [torch.tensor(math.log(v), dtype=torch.float64, requires_grad=True) for v in (std, lengthscale)]
    log_noise = torch.tensor(math.log(noise_var), dtype=torch.float64, requires_grad=True) if learn_noise and noise_var > 0 else None
    mean = torch.tensor(value, dtype=torch.float64, requires_grad=learn_mean)
    params = logs + ([log_noise] if log_noise is not None else []) + ([mean] if learn_mean else [])
    opt = torch.optim.Adam(params, lr=lr)
    seen = []
    for _ in range(n_steps):
        opt.zero_grad()
        noise = log_noise.exp() if log_noise is not None else noise_var
        out = log_evidence(train_x, train_y, logs[0].exp(), logs[1].exp(), noise, mean)
        (-out).backward()
        opt.step()
        seen.append(float(out.detach()))
    with torch.no_grad():
        final = (float(logs[0].exp()), float(logs[1].exp()), float(log_noise.exp()) if log_noise is not None else noise_var,
                 float(mean.detach()))
    return seen, final
