"""The Gaussian process restated for the tests: float64 closed forms (covariance, Cholesky, both right-hand solves, the
posterior), and a float32 emulation of the blocked algorithm of csrc/gp.hip (panels of 64 at absolute positions, right-looking,
the appended factorisation and the solve that completes columns) that is used to CHOOSE cases and to check the drivers' index
arithmetic on the CPU, never as a reference for the GPU results."""

import numpy as np
import torch

TILE = 64


# ---------------------------------------------------------------------------------------------
# float64 closed forms
def se(a, b, std, lengthscale):
    """std^2 exp(-|a_i - b_j|^2 / (2 l^2)) by exact differences, float64."""
    a, b = a.double(), b.double()
    sq = ((a[:, None, :] - b[None, :, :]) ** 2).sum(-1)
    return std ** 2 * torch.exp(-sq / (2.0 * lengthscale ** 2))


def cholesky(a):
    return torch.linalg.cholesky(a.double())


def solve_right(l, b, transposed=False):
    """x with x l^T = b (transposed: x l = b), l lower triangular, float64."""
    l, b = l.double().tril(), b.double()
    if transposed:  # x l = b  <=>  l^T x^T = b^T
        return torch.linalg.solve_triangular(l.t(), b.t(), upper=True).t()
    return torch.linalg.solve_triangular(l, b.t(), upper=False).t()  # l x^T = b^T


def posterior(train_x, train_y, x, std, lengthscale, value, noise_var, kernel=None):
    """(mu, sig) of the posterior in float64 through a Cholesky solve; kernel: another covariance function of (a, b)."""
    k = kernel or (lambda a, b: se(a, b, std, lengthscale))
    n = train_x.shape[0]
    kt = k(train_x, train_x) + noise_var * torch.eye(n, dtype=torch.float64)
    kx = k(x, train_x)
    l = cholesky(kt)
    alpha = torch.cholesky_solve(train_y.double() - value, l)
    w = solve_right(l, kx)
    return value + kx @ alpha, k(x, x) - w @ w.t()


def prior(x, std, lengthscale, value):
    return torch.full((x.shape[0], 1), float(value), dtype=torch.float64), se(x, x, std, lengthscale)


def spd(n, seed):
    """A = B B^T / n + I for a random (n, n) B: cond <= about 5, float32 values (exactly representable inputs for both sides)."""
    g = torch.Generator().manual_seed(seed)
    b = torch.randn(n, n, generator=g, dtype=torch.float64)
    return (b @ b.t() / n + torch.eye(n, dtype=torch.float64)).float()


# ---------------------------------------------------------------------------------------------
# float32 emulation of the blocked algorithm (numpy, in place on float32 arrays)
def emu_gemm(c, a, b, lower=False, diag_off=0, plus=False):
    prod = (a.astype(np.float32) @ b.astype(np.float32).T).astype(np.float32)
    new = c + prod if plus else c - prod
    if lower:
        r, cc = np.indices(c.shape)
        keep = cc <= r + diag_off
        c[keep] = new[keep]
    else:
        c[...] = new


def emu_potrf_diag(a, done=0, base=0, info=None):
    jb = a.shape[0]
    for j in range(jb):
        for i in range(max(j, done), jb):
            v = np.float32(a[i, j])
            for k in range(j):
                v = np.float32(v - np.float32(a[i, k] * a[j, k]))
            if i == j:
                if not v > 0 and info is not None and info[0] == 0:
                    info[0] = base + j + 1
                with np.errstate(invalid="ignore"):
                    a[i, j] = np.sqrt(v, dtype=np.float32)
            else:
                a[i, j] = np.float32(v / a[j, j])


def emu_trsm_diag(l, x, done=0, transposed=False):
    jb = l.shape[0]
    order = range(jb - 1, -1, -1) if transposed else range(done, jb)
    for j in order:
        ks = range(j + 1, jb) if transposed else range(j)
        v = x[:, j].copy()
        for k in ks:
            v = (v - x[:, k] * (l[k, j] if transposed else l[j, k])).astype(np.float32)
        x[:, j] = v / l[j, j]


def emu_potrf(a, n_done=0, info=None):
    n = a.shape[0]
    first = n_done // TILE
    for k in range(first):
        j0 = k * TILE
        emu_trsm_diag(a[j0:j0 + TILE, j0:j0 + TILE], a[n_done:, j0:j0 + TILE])
        emu_gemm(a[n_done:, j0 + TILE:], a[n_done:, j0:j0 + TILE], a[j0 + TILE:, j0:j0 + TILE], lower=True,
                 diag_off=n_done - (j0 + TILE))
    for k in range(first, -(-n // TILE)):
        j0 = k * TILE
        jb = min(TILE, n - j0)
        emu_potrf_diag(a[j0:j0 + jb, j0:j0 + jb], done=max(0, n_done - j0), base=j0, info=info)
        if n - j0 - jb > 0:
            emu_trsm_diag(a[j0:j0 + jb, j0:j0 + jb], a[j0 + TILE:, j0:j0 + TILE])
            emu_gemm(a[j0 + TILE:, j0 + TILE:], a[j0 + TILE:, j0:j0 + TILE], a[j0 + TILE:, j0:j0 + TILE], lower=True)


def emu_trsm_right(l, x, col_done=0, transposed=False):
    n = l.shape[0]
    panels = -(-n // TILE)
    if transposed:
        for k in range(panels - 1, -1, -1):
            j0 = k * TILE
            jb = min(TILE, n - j0)
            emu_trsm_diag(l[j0:j0 + jb, j0:j0 + jb], x[:, j0:j0 + jb], transposed=True)
            if j0:
                emu_gemm(x[:, :j0], x[:, j0:j0 + jb], l[j0:j0 + jb, :j0].T)
        return
    first = col_done // TILE
    if first:
        emu_gemm(x[:, col_done:], x[:, :first * TILE], l[col_done:, :first * TILE])
    for k in range(first, panels):
        j0 = k * TILE
        jb = min(TILE, n - j0)
        emu_trsm_diag(l[j0:j0 + jb, j0:j0 + jb], x[:, j0:j0 + jb], done=max(0, col_done - j0))
        if n - j0 - jb > 0:
            emu_gemm(x[:, j0 + TILE:], x[:, j0:j0 + TILE], l[j0 + TILE:, j0:j0 + TILE])
