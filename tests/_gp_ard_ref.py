"""The stationary kernels of the Gaussian process with per-dimension (ARD) lengthscales restated for the tests in float64: the
covariances of the three kinds, log p(y), the closed forms of its gradients (every d/d l_c with the magnitude of its terms before
cancellation), the operand-level sums of ops.ard_mll_sums and ops.stationary_mll_sums, the posterior, the Adam loop on the
log-hyperparameters that GaussianProcess.optimize_hyperparameters runs, and the data generator both test tiers share.

With w_c = 1 / l_c and r^2 = sum_c ((a_c - b_c) w_c)^2: k = std^2 phi(r), omega = -phi'(r) / r (finite at 0), so
d k / d l_c = std^2 omega(r) ((a_c - b_c) w_c)^2 / l_c. Nothing here differentiates through sqrt at 0: the closed forms use omega,
and log_evidence (for autograd) takes the root of the off-diagonal distances only."""

import math

import torch

KINDS = ("se", "matern32", "matern52")
NAMES = ("std", "lengthscale", "noise_var", "value")
STD, NOISE_VAR, VALUE = 1.3, 0.1, 0.2
# (n, d, p) of the model tests; the seed of each (kind, shape) is chosen in SEEDS so that no d/d l_c is a cancellation to
# nothing (tests/test_gp_ard_cpu.py::test_model_cases_are_well_conditioned holds the condition)
MODEL_SHAPES = ((1, 1, 1), (64, 2, 2), (65, 2, 1), (130, 3, 2), (321, 17, 1), (130, 33, 3))
SEEDS = {("matern32", 321, 17, 1): 5, ("matern32", 130, 33, 3): 2, ("matern52", 130, 3, 2): 1, ("matern52", 321, 17, 1): 5,
         ("matern52", 130, 33, 3): 2}  # every other case: 0
# the squared exponential is smoother than the Matern kinds: at their lengthscales it sits so near its optimum in some columns that
# d/d l_c is 1e-4 of its terms; at half of them it is as far from it as they are
LS_SCALE = {"se": 0.5, "matern32": 1.0, "matern52": 1.0}


def _ls(lengthscale, d):
    """The lengthscale as a float64 tensor broadcastable over the d columns (a scalar stays a scalar)."""
    if torch.is_tensor(lengthscale):
        return lengthscale if lengthscale.dtype == torch.float64 else lengthscale.double()
    if isinstance(lengthscale, (tuple, list)):
        return torch.tensor(lengthscale, dtype=torch.float64)
    return torch.tensor(float(lengthscale), dtype=torch.float64)


def scaled_sq_terms(a, b, lengthscale):
    """((a_ic - b_jc) / l_c)^2, (n, m, d), float64, difference first."""
    a, b = a.double(), b.double()
    return ((a[:, None, :] - b[None, :, :]) / _ls(lengthscale, a.shape[1])) ** 2


def phi_omega(kind, r2):
    """(phi, omega) of r^2 >= 0, elementwise. The root is taken of the positive entries only (r = 0 where r^2 = 0), so
    autograd through phi meets no sqrt at 0."""
    if kind == "se":
        e = torch.exp(-0.5 * r2)
        return e, e
    positive = r2 > 0
    r = torch.where(positive, torch.sqrt(torch.where(positive, r2, torch.ones_like(r2))), torch.zeros_like(r2))
    if kind == "matern32":
        s = math.sqrt(3.0) * r
        e = torch.exp(-s)
        return (1.0 + s) * e, 3.0 * e
    if kind == "matern52":
        s = math.sqrt(5.0) * r
        e = torch.exp(-s)
        return (1.0 + s + s * s / 3.0) * e, (5.0 / 3.0) * (1.0 + s) * e
    raise ValueError(kind)


def covariance(a, b, std, lengthscale, kind):
    """std^2 phi(r) of the rows of a and b, float64; lengthscale a float or d values."""
    return std ** 2 * phi_omega(kind, scaled_sq_terms(a, b, lengthscale).sum(-1))[0]


def log_evidence(train_x, train_y, std, lengthscale, noise_var, value, kind):
    """log p(y) in float64 from torch.linalg.cholesky; the hyperparameters may be float64 tensors that require grad."""
    x, y = train_x.double(), train_y.double()
    n, p = y.shape
    k = covariance(x, x, std, lengthscale, kind) + noise_var * torch.eye(n, dtype=torch.float64)
    l = torch.linalg.cholesky(k)
    z = torch.linalg.solve_triangular(l, y - value, upper=False)
    return -0.5 * (z ** 2).sum() - p * torch.log(torch.diagonal(l)).sum() - 0.5 * n * p * math.log(2.0 * math.pi)


def _lengthscale_sums(g, std, lengthscale, terms, omega, shared):
    """(d/d lengthscale, the sum of the absolute values of its terms): per column for ARD, one number for a shared one."""
    coef = (g * std ** 2 * omega).reshape(-1)  # the terms are coef_ij ((x_ic - x_jc) w_c)^2, and the squares are >= 0
    ls = _ls(lengthscale, terms.shape[-1])
    flat = terms.reshape(-1, terms.shape[-1])
    if shared:
        flat = flat.sum(-1, keepdim=True)
    sums, sizes = coef @ flat / (2.0 * ls), coef.abs() @ flat / (2.0 * ls)
    return (sums[0], sizes[0]) if shared else (sums, sizes)


def closed_form(train_x, train_y, std, lengthscale, noise_var, value, kind):
    """(log p(y), {name: gradient}, the magnitude of d/d lengthscale's terms) by the closed forms: G = alpha alpha^T - p K^-1,
    d/d std = sum G K_f / std, d/d l_c = sum_ij G_ij std^2 omega_ij ((x_ic - x_jc) / l_c)^2 / (2 l_c) (a float lengthscale: the
    sum over c), d/d noise_var = tr G / 2, d/d value = sum alpha. The magnitude is sum |terms_c| / (2 l_c)."""
    x, y = train_x.double(), train_y.double()
    n, p = y.shape
    shared = not (torch.is_tensor(lengthscale) and lengthscale.dim() == 1) and not isinstance(lengthscale, (tuple, list))
    terms = scaled_sq_terms(x, x, lengthscale)
    phi, omega = phi_omega(kind, terms.sum(-1))
    kf = std ** 2 * phi
    l = torch.linalg.cholesky(kf + noise_var * torch.eye(n, dtype=torch.float64))
    z = torch.linalg.solve_triangular(l, y - value, upper=False)
    alpha = torch.linalg.solve_triangular(l.t(), z, upper=True)
    value_ = -0.5 * (z ** 2).sum() - p * torch.log(torch.diagonal(l)).sum() - 0.5 * n * p * math.log(2.0 * math.pi)
    g = alpha @ alpha.t() - p * torch.cholesky_inverse(l)
    grad_ls, size_ls = _lengthscale_sums(g, std, lengthscale, terms, omega, shared)
    grads = {"std": (g * kf).sum() / std, "lengthscale": grad_ls, "noise_var": 0.5 * torch.trace(g), "value": alpha.sum()}
    return value_, grads, size_ls


def autograd_form(train_x, train_y, std, lengthscale, noise_var, value, kind):
    """The value and the gradients from float64 autograd through torch.linalg.cholesky."""
    ls = _ls(lengthscale, train_x.shape[1]).clone().requires_grad_()
    leaves = [torch.tensor(float(v), dtype=torch.float64, requires_grad=True) for v in (std, noise_var, value)]
    out = log_evidence(train_x, train_y, leaves[0], ls, leaves[1], leaves[2], kind)
    out.backward()
    return out.detach(), {"std": leaves[0].grad, "lengthscale": ls.grad, "noise_var": leaves[1].grad, "value": leaves[2].grad}


def _g_of(h, alpha_t):
    h = h.double().tril()
    h = h + h.tril(-1).t()
    a = alpha_t.double()
    return a.t() @ a - a.shape[0] * h


def ard_sums(x, std, lengthscale, h, alpha_t, kind, terms=None):
    """(sums, magnitudes): the d + 2 outputs of ops.ard_mll_sums in float64 from the given operands (h is read on its lower
    triangle and mirrored) — d/d std, d/d noise_var, d/d l_0 .. — and for each the sum of the absolute values of its terms.
    terms: scaled_sq_terms(x, x, lengthscale), if the caller has it."""
    terms = scaled_sq_terms(x, x, lengthscale) if terms is None else terms
    phi, omega = phi_omega(kind, terms.sum(-1))
    g = _g_of(h, alpha_t)
    grad_ls, size_ls = _lengthscale_sums(g, std, lengthscale, terms, omega, shared=False)
    first = (g * std ** 2 * phi / std, 0.5 * torch.diagonal(g))
    return (torch.cat([torch.stack([t.sum() for t in first]), grad_ls]), torch.cat([torch.stack([t.abs().sum() for t in first]), size_ls]))


def stat_sums(x, std, lengthscale, h, alpha_t, kind):
    """(sums, magnitudes) of ops.stationary_mll_sums for one shared lengthscale: d/d std, d/d lengthscale, d/d noise_var."""
    terms = scaled_sq_terms(x, x, float(lengthscale))
    phi, omega = phi_omega(kind, terms.sum(-1))
    g = _g_of(h, alpha_t)
    grad_ls, size_ls = _lengthscale_sums(g, std, float(lengthscale), terms, omega, shared=True)
    first, last = g * std ** 2 * phi / std, 0.5 * torch.diagonal(g)
    return torch.stack([first.sum(), grad_ls, last.sum()]), torch.stack([first.abs().sum(), size_ls, last.abs().sum()])


def posterior(train_x, train_y, x, std, lengthscale, value, noise_var, kind):
    """(mu, sig) of the posterior in float64 through a Cholesky solve."""
    n = train_x.shape[0]
    kt = covariance(train_x, train_x, std, lengthscale, kind) + noise_var * torch.eye(n, dtype=torch.float64)
    kx = covariance(x, train_x, std, lengthscale, kind)
    l = torch.linalg.cholesky(kt)
    alpha = torch.cholesky_solve(train_y.double() - value, l)
    w = torch.linalg.solve_triangular(l, kx.t(), upper=False).t()
    return value + kx @ alpha, covariance(x, x, std, lengthscale, kind) - w @ w.t()


def adam_loop(train_x, train_y, start, kind, n_steps=50, lr=0.05, learn_noise=True, learn_mean=True):
    """torch.optim.Adam ascending log p(y) on log std, log l_c (every entry), log noise_var and value, float64, from
    start = (std, lengthscale (d values), noise_var, value). Returns (the values seen, the final hyperparameters in that order,
    the lengthscale a tuple)."""
    std, lengthscale, noise_var, value = start
    log_std = torch.tensor(math.log(float(std)), dtype=torch.float64, requires_grad=True)
    log_ls = _ls(lengthscale, train_x.shape[1]).log().clone().requires_grad_()
    log_noise = torch.tensor(math.log(noise_var), dtype=torch.float64, requires_grad=True) if learn_noise and noise_var > 0 else None
    mean = torch.tensor(float(value), dtype=torch.float64, requires_grad=learn_mean)
    params = [log_std, log_ls] + ([log_noise] if log_noise is not None else []) + ([mean] if learn_mean else [])
    opt = torch.optim.Adam(params, lr=lr)
    seen = []
    for _ in range(n_steps):
        opt.zero_grad()
        noise = log_noise.exp() if log_noise is not None else noise_var
        out = log_evidence(train_x, train_y, log_std.exp(), log_ls.exp(), noise, mean, kind)
        (-out).backward()
        opt.step()
        seen.append(float(out.detach()))
    with torch.no_grad():
        final = (float(log_std.exp()), tuple(log_ls.exp().tolist()), float(log_noise.exp()) if log_noise is not None else noise_var,
                 float(mean.detach()))
    return seen, final


# ---------------------------------------------------------------------------------------------
# the data both tiers use
def model_case(kind, n, d, p):
    """x ~ N(0, I) (n, d), one lengthscale per column in LS_SCALE[kind] [0.7, 2.0] sqrt(d), y = sin(sum x / sqrt(d)) + 0.1 eps (n, p): fp32
    tensors and the lengthscales as an fp32 tensor, away from the optimum of (STD, NOISE_VAR, VALUE)."""
    g = torch.Generator().manual_seed(SEEDS.get((kind, n, d, p), 0) * 100003 + 1000 * n + 10 * d + p)
    x = torch.randn(n, d, generator=g)
    lengthscale = (LS_SCALE[kind] * (0.7 + 1.3 * torch.rand(d, generator=g)) * math.sqrt(d)).float()
    y = torch.sin(x.sum(1, keepdim=True) / math.sqrt(d)) + 0.1 * torch.randn(n, p, generator=g)
    return x, y, lengthscale


def relevance_case(n=130, seed=2025):
    """Three input columns of which the third is pure noise: y = sin(2 x_0) + cos(x_1) + 0.1 eps. A learner of per-dimension
    lengthscales must end with the third the largest."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, 3, generator=g)
    y = torch.sin(2.0 * x[:, :1]) + torch.cos(x[:, 1:2]) + 0.1 * torch.randn(n, 1, generator=g)
    return x, y
