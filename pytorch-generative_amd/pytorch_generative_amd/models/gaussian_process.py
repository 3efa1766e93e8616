"""The Gaussian process model on the MI355X path (reference models/gaussian_process.py).

p(f) = N(f | mean(x), kernel(x, x')); observations carry independent noise of variance noise_var. Same constructor, `fit`,
`predict` and `sample` as the reference, and the same `noise_var` buffer. The reference solves the full (n, n) training
covariance with an LU factorisation inside every `predict`; here the covariance is factored ONCE by a blocked fp32 Cholesky
(ops.cholesky_, csrc/gp.hip) into a buffer that grows, and a `fit` of further points only completes the new rows of the factor
(`incremental`, below): O(n^2) per added point instead of O(n^3), as the Bayesian-optimisation loop of the reference's notebook
(fit one point, predict, sample, repeat) wants it.

With K = kernel(train, train) + noise_var I = L L^T, r = y - mean(train), z = L^-1 r and alpha = L^-T z, `predict(x)` is
    Kx^T = kernel(x, train)                (m, n): the training rows stay where they lie
    mu   = mean(x) + Kx^T alpha            (ops.gemm_nt_)
    W    = Kx^T L^-T                       (ops.trsm_right_, one forward solve)
    sig  = kernel(x, x) - W W^T            (ops.gemm_nt_, lower triangle only, mirrored: exactly symmetric)

Stated deviations from the reference:
  * Cholesky replaces LU. Where the training covariance is numerically singular (noise_var = 0 on dense data) the reference
    returns noise; this raises torch.linalg.LinAlgError naming the failed pivot.
  * `predict` and `sample` carry no gradient, and an input that requires grad raises: there are no gradients with respect to
    x or y.
  * The reference has no marginal likelihood. Here `log_marginal_likelihood()` gives log p(y) of the fitted data from the
    cached factor, as an autograd node over std, lengthscale, the constant mean and noise_var (every route but "callable"),
    and `optimize_hyperparameters()` runs Adam on their logarithms. With
    G = alpha alpha^T - p K^-1 the gradients are sum G K_f / std, sum G K_f D2 / (2 l^3), tr G / 2 and sum alpha;
    K^-1 = X X^T comes from the triangular inverse X = L^-T (ops.tri_inverse_t, ops.gram_upper_) and the sums from one fused
    reduction that writes no derivative matrix (ops.stationary_mll_sums, csrc/gp_mll.hip). The inverse is made for the call and freed;
    it is not appended to after a `fit`.
  * The reference has one kernel, in its notebook. Here SquaredExponential also takes one lengthscale PER INPUT COLUMN (ARD) and
    Matern (nu = 3/2, 5/2) stands beside it; every stationary kernel runs on ops.stationary_kernel, one code path with the
    appended factor, the evidence, its gradients (d/d l_c = S_c / (2 l_c) from ops.ard_mll_sums, up to 256 columns) and the
    optimiser.
  * `sample` draws on the GPU from torch's generator and returns fp32 on the device (the reference: float64 from numpy).
SquaredExponential and Const restate the two callables the reference defines only in its notebook."""

import math

import torch
from torch import nn

from pytorch_generative_amd import ops
from pytorch_generative_amd.models import base

_TILE = 64
JITTER_LADDER = (0.0, 1e-6, 1e-5, 1e-4, 1e-3, 1e-2)


def _host_value(owner, name):
    """The hyperparameter `name` of `owner` as a Python float, or as a tuple of floats if it is a 1-D tensor (one lengthscale
    per input column). A tensor is read (a host synchronisation if it lives on the GPU) only when it is another tensor, lies
    elsewhere or was modified in place since the last look, so a `predict` with unchanged hyperparameters synchronises nothing.
    A change made through `.data` is not seen: call GaussianProcess.reset_cache()."""
    value = getattr(owner, name)
    if not torch.is_tensor(value):
        return float(value)
    cache = owner.__dict__.setdefault("_host_cache", {})
    key = (id(value), value._version, value.data_ptr())
    hit = cache.get(name)
    if hit is None or hit[0] != key:
        host = tuple(float(v) for v in value.detach().tolist()) if value.dim() == 1 else float(value.detach())
        hit = (key, host, {})
        cache[name] = hit
    return hit[1]


def _device_inverse(owner, name, device):
    """1 / (the 1-D hyperparameter `name` of `owner`) as an fp32 tensor on `device`, made from the host values of _host_value
    and kept beside them: the same key, so it is made again exactly when they are read again."""
    host = _host_value(owner, name)
    made = owner.__dict__["_host_cache"][name][2]
    device = torch.device(device)
    if device not in made:
        made[device] = torch.tensor(host, dtype=torch.float32).reciprocal().to(device)
    return made[device]


class _Stationary(nn.Module):
    """k(a, b) = std^2 phi(r), r^2 = sum_c ((a_c - b_c) / lengthscale_c)^2: what SquaredExponential and Matern share. std: a
    float, a tensor, or (default) a Parameter initialised to 1. lengthscale: the same (one shared lengthscale), or a 1-D tensor
    or Parameter of d entries, one per input column (ARD); with n_dims = d and no lengthscale, a Parameter of d ones."""

    kind = None  # the key of ops.GP_KINDS

    def __init__(self, std=None, lengthscale=None, n_dims=None):
        super().__init__()
        self.std = nn.Parameter(torch.tensor(1.0)) if std is None else std
        if lengthscale is None:
            lengthscale = nn.Parameter(torch.tensor(1.0) if n_dims is None else torch.ones(int(n_dims)))
        if torch.is_tensor(lengthscale) and lengthscale.dim() > 1:
            raise ValueError(f"lengthscale: a scalar or a 1-D tensor with one entry per input column, got shape {tuple(lengthscale.shape)}")
        self.lengthscale = lengthscale
        if n_dims is not None:
            self.check_dims(int(n_dims))

    @property
    def ard(self):
        """One lengthscale per input column (a 1-D tensor) rather than one shared scalar."""
        return torch.is_tensor(self.lengthscale) and self.lengthscale.dim() == 1

    def check_dims(self, d):
        if self.ard and self.lengthscale.numel() != d:
            raise ValueError(f"{type(self).__name__}: the lengthscale has {self.lengthscale.numel()} entries, the inputs have {d} columns")

    def hyperparameters(self):
        """(std, lengthscale) as host values: floats, the lengthscale a tuple of floats if it is per dimension."""
        return _host_value(self, "std"), _host_value(self, "lengthscale")

    def covariance(self, left, right, noise_var=0.0, **form):
        """ops.stationary_kernel of the two matrices under the current hyperparameters; `form`: its out, mirror, diag_offset."""
        self.check_dims(left.shape[1])
        std, lengthscale = self.hyperparameters()
        inverse = _device_inverse(self, "lengthscale", left.device) if self.ard and left.is_cuda else None
        if self.ard and inverse is None:
            lengthscale = self.lengthscale.detach()
        return ops.stationary_kernel(left, right, std, lengthscale, noise_var, kind=self.kind, inv_lengthscale=inverse, **form)

    def forward(self, left, right):
        return self.covariance(left, right)


class SquaredExponential(_Stationary):
    """k(a, b) = std^2 exp(-|a - b|^2 / (2 lengthscale^2)). std and lengthscale: floats, tensors, or (default) Parameters
    initialised to 1. Called on 2-D GPU tensors it returns the (rows of left, rows of right) covariance from
    ops.stationary_kernel; `kernel(x, x)` (the same tensor twice) is exactly symmetric with the diagonal exactly std^2. A 1-D
    lengthscale of d entries (or n_dims = d: a Parameter of d ones) gives every input column its own,
    k = std^2 exp(-sum_c ((a_c - b_c) / l_c)^2 / 2)."""

    kind = "se"


class Matern(_Stationary):
    """The Matern kernel with nu = 1.5, k = std^2 (1 + sqrt(3) r) exp(-sqrt(3) r), or nu = 2.5 (default),
    k = std^2 (1 + sqrt(5) r + 5 r^2 / 3) exp(-sqrt(5) r), r^2 = sum_c ((a_c - b_c) / lengthscale_c)^2. std, lengthscale and
    n_dims as SquaredExponential's. Called on 2-D GPU tensors it returns the covariance from ops.stationary_kernel."""

    def __init__(self, nu=2.5, std=None, lengthscale=None, n_dims=None):
        if nu not in (1.5, 2.5):
            raise ValueError(f"Matern: nu = {nu!r} is neither 1.5 nor 2.5 (nu = 0.5 has no finite -phi'(r) / r at r = 0 and is not built)")
        super().__init__(std, lengthscale, n_dims)
        self.nu = float(nu)
        self.kind = "matern32" if nu == 1.5 else "matern52"


class Const(nn.Module):
    """mean(x) = value for every row: (rows of x, 1) on x's device. value: a float, a tensor, or (default) a Parameter
    initialised to 0."""

    def __init__(self, value=None):
        super().__init__()
        self.value = nn.Parameter(torch.tensor(0.0)) if value is None else value

    def hyperparameters(self):
        return (_host_value(self, "value"),)

    def forward(self, x):
        return torch.full((x.shape[0], 1), self.hyperparameters()[0], device=x.device, dtype=torch.float32)


class _LogEvidence(torch.autograd.Function):
    """log p(y) as an autograd node over the hyperparameter tensors that require grad. The forward is handed the value and
    the gradient vector the kernels made — (d/d value, d/d std, d/d lengthscale, d/d noise_var), or with per-dimension
    lengthscales the 3 + d entries (d/d value, d/d std, d/d noise_var, d/d l_0 ..) — and `which` names the entry (an index, or
    the slice of a 1-D lengthscale) of each tensor. The backward only scales the stored gradients by grad_output."""

    @staticmethod
    def forward(ctx, value, grads, which, *hypers):
        ctx.save_for_backward(grads)
        ctx.targets = [(k, h.shape, h.device, h.dtype) for k, h in zip(which, hypers)]
        return value.clone()

    @staticmethod
    def backward(ctx, grad_output):
        (grads,) = ctx.saved_tensors
        scaled = grad_output * grads
        return (None, None, None, *(scaled[k].reshape(shape).to(device=device, dtype=dtype) for k, shape, device, dtype in ctx.targets))


class GaussianProcess(base.GenerativeModel):
    """The Gaussian process model.

    incremental (class attribute, default True; set it on the class or an instance): a `fit` of further points completes
    only the new rows of the cached factor (`_factor_route == "append"`; the factor has the bits of a full factorisation).
    The factor is made afresh (`"full"`) when incremental is False, when a hyperparameter value (std, lengthscale, value,
    noise_var) differs from the one the factor was made with, and when the kernel or the mean is a callable other than
    SquaredExponential / Const: the model cannot see such a callable's state, so it never appends with it, and after CHANGING
    that state call reset_cache() — otherwise a cached factor keeps serving `predict` (a SquaredExponential or Const beside such a
    callable is still watched: a change of its values makes the factor afresh). incremental = False is always safe.

    `_kernel_route` is a label for what was built, not a code path: "se" (SquaredExponential kernel with one shared
    lengthscale and Const mean) and "stationary" (a Matern kernel, or a SquaredExponential with one lengthscale per input
    column, and Const mean) run the same code — covariances straight from kernel.covariance (ops.stationary_kernel), the
    appended factor, the evidence and the optimiser; the code asks only whether the route is "callable" (the callables are
    called on the device tensors; a square result kernel(t, t) is copied as it is, but only its lower triangle is read: the
    factorisation and the covariance update never look above the diagonal, the output is mirrored)."""

    incremental = True

    def __init__(self, mean, kernel, noise_var=None):
        """mean: prior mean function mu(x) -> (rows, 1) or (rows, p). kernel: prior covariance function K(x, x').
        noise_var: the variance of the observation noise (None: noiseless observations)."""
        super().__init__()
        self.mean = mean
        self.kernel = kernel
        self.register_buffer("noise_var", torch.tensor(noise_var or 0.0))
        self.train_x = None
        self.train_y = None
        self._kernel_route = "callable"
        if isinstance(kernel, _Stationary) and isinstance(mean, Const):
            self._kernel_route = "se" if isinstance(kernel, SquaredExponential) and not kernel.ard else "stationary"
        self._factor_route = None
        self._sample_jitter = None
        self._sample_factor = None
        self.reset_cache()

    def reset_cache(self):
        """Drops the cached factor: the next `predict` factors the whole training covariance."""
        self._factor = None    # (cap, cap): the lower factor of the leading (_n_factored, _n_factored) block
        self._zt = None        # (p, cap): rows of z^T = (L^-1 (y - mean))^T
        self._alpha_t = None   # (p, cap): rows of alpha^T
        self._n_factored = 0
        self._factor_key = None

    def fit(self, x, y):
        """Appends (x (rows, d), y (rows, p)) to the training data, as the reference does; the factor follows at the next
        `predict`."""
        if x.dim() != 2 or y.dim() != 2 or x.shape[0] != y.shape[0]:
            raise ValueError(f"fit: expected x (rows, d) and y (rows, p), got {tuple(x.shape)} and {tuple(y.shape)}")
        if x.requires_grad or y.requires_grad:
            raise ValueError("fit: the Gaussian process builds no gradients (a training tensor requires grad)")
        if isinstance(self.kernel, _Stationary):
            self.kernel.check_dims(x.shape[1])
        first = self.train_x is None
        self.train_x = x if first else torch.cat((self.train_x, x))
        self.train_y = y if first else torch.cat((self.train_y, y))

    # -- covariances and means ----------------------------------------------------------------------------------------------
    def _hyper(self):
        """What the cached factor depends on besides the data, as host values."""
        seen = tuple(part.hyperparameters() if isinstance(part, (_Stationary, Const)) else None for part in (self.kernel, self.mean))
        return (self._kernel_route, *seen, _host_value(self, "noise_var"))

    def _cross(self, x):
        """kernel(x, train), (m, n), in memory of its own (the solve overwrites it)."""
        if self._kernel_route != "callable":
            return self.kernel.covariance(x, self.train_x)
        out = self.kernel(x, self.train_x)
        return out.clone() if out.is_contiguous() else out.contiguous()

    def _prior(self, x, mirror):
        """kernel(x, x), (m, m), in memory of its own; with mirror=False only its lower triangle is promised."""
        if self._kernel_route != "callable":
            return self.kernel.covariance(x, x, mirror=mirror)
        return self.kernel(x, x).clone(memory_format=torch.contiguous_format)

    def _train_rows(self, lo, hi, out, noise):
        """Rows lo .. hi of kernel(train, train) + noise I into out (hi - lo, hi): columns 0 .. their own."""
        x = self.train_x
        if self._kernel_route != "callable":
            if lo == 0:
                self.kernel.covariance(x, x, noise, out=out, mirror=False)
            else:
                self.kernel.covariance(x[lo:hi], x, noise, out=out, diag_offset=lo)
        else:
            out.copy_(self.kernel(x, x))
            ops.add_diag_(out, noise)

    # -- the factor -----------------------------------------------------------------------------------------------------------
    def _grow(self, n, p, keep):
        """Buffers for n rows: the capacity is a multiple of 64 and doubles when full; `keep` rows of the old factor and of
        z are carried over by plain tensor copies."""
        cap = 0 if self._factor is None else self._factor.shape[0]
        if n <= cap and self._zt.shape[0] == p:
            return
        new_cap = max(cap, _TILE)
        while new_cap < n:
            new_cap *= 2
        dev = self.train_x.device
        factor = torch.zeros((new_cap, new_cap), device=dev, dtype=torch.float32)
        zt = torch.zeros((p, new_cap), device=dev, dtype=torch.float32)
        if keep:
            factor[:keep, :keep].copy_(self._factor[:keep, :keep])
            zt[:, :keep].copy_(self._zt[:, :keep])
        self._factor, self._zt = factor, zt
        self._alpha_t = torch.zeros((p, new_cap), device=dev, dtype=torch.float32)

    def _ensure_factor(self):
        n, p = self.train_y.shape
        key = self._hyper()
        same = (self._factor is not None and key == self._factor_key and self._factor.device == self.train_x.device
                and self._zt.shape[0] == p)
        if same and self._n_factored == n:
            return
        done = self._n_factored if (same and self.incremental and self._kernel_route != "callable" and 0 < self._n_factored < n) else 0
        self._factor_route = "append" if done else "full"
        noise = key[-1]
        try:
            self._grow(n, p, done)
            lower = self._factor[:n, :n]
            self._train_rows(done, n, self._factor[done:n, :n], noise)
            info = ops.cholesky_(lower, n_done=done)
            resid = self.train_y[done:] - self.mean(self.train_x[done:])
            self._zt[:, done:n].copy_(resid.t())
            ops.trsm_right_(lower, self._zt[:, :n], col_done=done)
            self._alpha_t[:, :n].copy_(self._zt[:, :n])
            ops.trsm_right_(lower, self._alpha_t[:, :n], transposed=True)
            failed = int(info)  # the one host synchronisation of a factorisation
        except Exception:
            self.reset_cache()
            raise
        if failed:
            self.reset_cache()
            raise torch.linalg.LinAlgError(
                f"GaussianProcess: the training covariance is not positive definite in fp32: the pivot at index {failed - 1} of {n} "
                f"is not > 0 (noise_var = {noise:g}). Pass a positive noise_var (or a larger one), or remove duplicate points.")
        self._n_factored, self._factor_key = n, key

    # -- the reference's interface ----------------------------------------------------------------------------------------
    @torch.no_grad()
    def predict(self, x):
        """The predicted mean (m, p) and covariance (m, m) at x (m, d): the posterior after `fit`, else the prior
        mean(x), kernel(x, x). fp32 on the GPU, no gradient. With an unchanged factor nothing synchronises with the host (the
        call can be captured into a graph); the `predict` after a `fit` reads one int32 back."""
        if x.requires_grad:
            raise ValueError("predict: the Gaussian process builds no gradients (x requires grad)")
        if self.train_x is None:
            return self.mean(x), self._prior(x, mirror=True)
        self._ensure_factor()
        n, p = self.train_y.shape
        lower = self._factor[:n, :n]
        w = self._cross(x)
        mu = self.mean(x).expand(x.shape[0], p).clone(memory_format=torch.contiguous_format)
        ops.gemm_nt_(mu, w, self._alpha_t[:, :n], add=True)
        ops.trsm_right_(lower, w)
        sig = self._prior(x, mirror=False)
        ops.gemm_nt_(sig, w, w, lower=True, mirror=True)
        return mu, sig

    @torch.no_grad()
    def sample(self, x, n_samples, generator=None):
        """n_samples draws (n_samples, m) of the process at x (m, d), from the posterior after `fit`, else from the prior:
        mu^T + Z L_s^T with Z = torch.randn((n_samples, m), generator=generator) on the GPU, drawn once, and L_s the Cholesky
        factor of sig + j mean(diag(kernel(x, x))) I, j the first of 0, 1e-6, 1e-5, ..., 1e-2 that factors
        (torch.linalg.LinAlgError if none does). The jitter is scaled by the PRIOR diagonal: the rounding noise of sig is
        eps cond times the prior scale, however small the posterior variance. Needs p = 1, as the reference's squeeze.
        `_sample_jitter` holds the j taken and `_sample_factor` L_s (strict upper triangle zero)."""
        mu, sig = self.predict(x)
        if mu.shape[1] != 1:
            raise ValueError(f"sample: needs one output column, the mean has shape {tuple(mu.shape)}")
        m = x.shape[0]
        if self._kernel_route != "callable":
            scale = self.kernel.hyperparameters()[0] ** 2
        else:
            scale = float(self.kernel(x, x).diagonal().mean())
        factor = None
        for jitter in JITTER_LADDER:
            factor = sig.clone()
            if jitter:
                ops.add_diag_(factor, jitter * scale)
            if int(ops.cholesky_(factor)) == 0:
                break
        else:
            raise torch.linalg.LinAlgError(
                f"GaussianProcess.sample: the predicted covariance ({m} points) does not factor in fp32 even with a jitter of "
                f"{JITTER_LADDER[-1]:g} of the prior variance; pass a positive noise_var or fewer, better separated points")
        self._sample_jitter, self._sample_factor = jitter, factor.tril_()
        z = torch.randn((n_samples, m), device=x.device, dtype=torch.float32, generator=generator)
        out = mu.t().expand(n_samples, m).clone(memory_format=torch.contiguous_format)
        return ops.gemm_nt_(out, z, self._sample_factor, add=True)

    # -- the marginal likelihood -------------------------------------------------------------------------------------------
    def _hyper_slots(self):
        """(entry of the gradient vector, owner, attribute, positive) of the hyperparameters: the four entries 0 .. 3 of one
        shared lengthscale; with d per-dimension lengthscales the vector has 3 + d entries, noise_var
        at 2 and the lengthscales in the slice 3 .. 3 + d."""
        if self.kernel.ard:
            d = self.kernel.lengthscale.numel()
            return ((0, self.mean, "value", False), (1, self.kernel, "std", True), (slice(3, 3 + d), self.kernel, "lengthscale", True),
                    (2, self, "noise_var", True))
        return ((0, self.mean, "value", False), (1, self.kernel, "std", True), (2, self.kernel, "lengthscale", True),
                (3, self, "noise_var", True))

    def _require_evidence(self, what):
        if self._kernel_route == "callable":
            raise NotImplementedError(f"{what}: built for a SquaredExponential or Matern kernel with a Const mean only; a callable kernel "
                                      "or mean has no marginal-likelihood kernels here")
        if self.train_x is None:
            raise ValueError(f"{what}: no training data; call fit first")

    @torch.no_grad()
    def _evidence(self, want_grads):
        """(log p(y), gradients): a 0-dim fp32 tensor on the device and, if want_grads, the 1-D tensor (d/d value, d/d std,
        d/d lengthscale, d/d noise_var) — with d per-dimension lengthscales (d/d value, d/d std, d/d noise_var, d/d l_0 ..
        d/d l_{d-1}) — else None. The value alone is one launch on the cached factor; the gradients add the triangular inverse,
        X X^T and the fused reduction, in two (n, n) workspaces that live for this call only."""
        ard = self.kernel.ard
        if want_grads and ard:
            self._require_ard_domain()
        self._ensure_factor()
        n, d = self.train_x.shape
        lower, zt, alpha_t = self._factor[:n, :n], self._zt[:, :n], self._alpha_t[:, :n]
        out = torch.empty(4 + d if ard and want_grads else 5, device=self.train_x.device, dtype=torch.float32)
        ops.mll_value(lower, zt, alpha_t, out=out[:2])
        if not want_grads:
            return out[0], None
        std, lengthscale = self.kernel.hyperparameters()
        inverse_t = torch.empty((n, n), device=out.device, dtype=torch.float32)
        precision = torch.empty((n, n), device=out.device, dtype=torch.float32)
        ops.tri_inverse_t(lower, out=inverse_t)
        ops.gram_upper_(precision, inverse_t)
        del inverse_t
        if ard:
            ops.ard_mll_sums(self.train_x, std, None, precision, alpha_t, kind=self.kernel.kind, out=out[2:],
                             inv_lengthscale=_device_inverse(self.kernel, "lengthscale", out.device))
        else:
            ops.stationary_mll_sums(self.train_x, std, lengthscale, precision, alpha_t, kind=self.kernel.kind, out=out[2:])
        return out[0], out[1:]

    def _require_ard_domain(self):
        """Per-dimension lengthscale gradients hold up to ops.gp_ard_plan's largest d; the planner's refusal, before any launch."""
        n, d = self.train_x.shape
        limit = ops.gp_ard_plan(1, 1, 1)["max_d"]
        if d > limit:
            raise ValueError(f"log_marginal_likelihood: the gradients of per-dimension lengthscales are built for at most {limit} input "
                             f"columns, the inputs have {d}; the value (under torch.no_grad()) works")

    def log_marginal_likelihood(self):
        """log p(y) of the fitted data under the current hyperparameters, a 0-dim fp32 tensor on the GPU, from the cached
        factor (made or appended to first, as in `predict`: the same error for a covariance that is not positive definite, the
        same one host synchronisation, none with an unchanged factor).

        With grad enabled the result is an autograd node over those of kernel.std, kernel.lengthscale, mean.value and
        noise_var that are tensors requiring grad (noise_var is a buffer: `gp.noise_var.requires_grad_()` opts it in; a
        hyperparameter held as a Python float gets no gradient). The forward then also makes the gradients — the inverse of
        the factor, K^-1 and the fused reduction, O(n^3) and two (n, n) workspaces that are freed before it returns — and
        the backward only scales them by grad_output. Under no_grad, or when nothing requires grad, the value alone is
        computed. No gradients with respect to x or y. NotImplementedError for a callable kernel or mean (the "callable"
        route). A 1-D lengthscale receives a gradient of its own shape, (d,), for d <= 256 (ValueError above)."""
        self._require_evidence("log_marginal_likelihood")
        wanted = []
        if torch.is_grad_enabled():
            for k, owner, name, _ in self._hyper_slots():
                t = getattr(owner, name)
                if torch.is_tensor(t) and t.requires_grad:
                    wanted.append((k, t))
        value, grads = self._evidence(bool(wanted))
        if not wanted:
            return value.clone()
        return _LogEvidence.apply(value, grads, [k for k, _ in wanted], *[t for _, t in wanted])

    def optimize_hyperparameters(self, n_steps=50, lr=0.05, learn_noise=True, learn_mean=True):
        """n_steps of torch.optim.Adam ascending log p(y) on log std, log lengthscale (every entry of a per-dimension one), log
        noise_var (when learn_noise and noise_var > 0) and the constant mean (when learn_mean); the positive ones by the chain
        rule theta d/d theta. Only hyperparameters held as tensors are learned (a Python float stays as it is), whether or not
        they require grad. After each step the new values are written back in place, which the cached factor sees: the next evaluation, and a `predict`
        afterwards, factor the covariance afresh (`_factor_route == "full"`). Returns the list of the values of log p(y) seen,
        one per step, each from before its step."""
        self._require_evidence("optimize_hyperparameters")
        learned = []
        for k, owner, name, positive in self._hyper_slots():
            if not torch.is_tensor(getattr(owner, name)):
                continue
            if (name == "noise_var" and not (learn_noise and _host_value(owner, name) > 0)) or (name == "value" and not learn_mean):
                continue
            start = _host_value(owner, name)
            start = list(start) if isinstance(start, tuple) else [start]
            if positive and not min(start) > 0:
                raise ValueError(f"optimize_hyperparameters: {name} = {min(start):g} must be > 0 to be learned on its logarithm")
            entries = list(range(k.start, k.stop)) if isinstance(k, slice) else [k]
            learned.append((entries, owner, name, positive, start))
        if not learned or n_steps < 1:
            return []
        dev = self.train_x.device
        # one entry of phi per learned number: a per-dimension lengthscale contributes one per column
        phi = torch.tensor([math.log(s) if pos else s for _, _, _, pos, start in learned for s in start], device=dev, dtype=torch.float32,
                           requires_grad=True)
        entries = torch.tensor([k for ks, _, _, _, _ in learned for k in ks], device=dev)
        positive = torch.tensor([pos for ks, _, _, pos, _ in learned for _k in ks], device=dev)
        optimizer = torch.optim.Adam([phi], lr=lr)
        seen = []
        for _ in range(n_steps):
            value, grads = self._evidence(True)
            with torch.no_grad():
                theta = torch.where(positive, phi.exp(), phi)
                phi.grad = -grads[entries] * torch.where(positive, theta, torch.ones_like(theta))
            optimizer.step()
            with torch.no_grad():
                theta = torch.where(positive, phi.exp(), phi)
                j = 0
                for ks, owner, name, _, _ in learned:
                    target = getattr(owner, name)
                    target.copy_(theta[j:j + len(ks)].reshape(target.shape))  # in place: bumps _version, so _host_value and the factor key see it
                    j += len(ks)
            seen.append(value)
        return torch.stack(seen).tolist()
