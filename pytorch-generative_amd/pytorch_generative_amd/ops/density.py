"""ops.density — log-densities of the mixture models and of kernel density estimation (reference
models/mixture_models.py, models/kde.py) on the streaming log-density kernels of csrc/density.hip.

Part of the operator layer (pytorch_generative_amd.ops): HIP kernels behind torch.autograd.Function, called through the C-ABI
with tensor.data_ptr() and the current stream. No CPU / ATen fallback: a missing library, a CPU tensor or an unsupported shape raises."""

import numpy as np
import torch

from pytorch_generative_amd import _lib
from pytorch_generative_amd.ops._common import _chk, _p, _sink, _stream, zeros

MIXTURE_BERNOULLI, MIXTURE_GAUSSIAN = 0, 1  # include/pg_hip.h PG_MIXTURE_*
_KINDS = {"bernoulli": (MIXTURE_BERNOULLI, 1), "gaussian": (MIXTURE_GAUSSIAN, 2)}


def _workspace(floats, device):
    # never empty: the kernels' prepared operands always live in it
    return torch.empty(max(int(floats), 1), device=device, dtype=torch.float32), int(floats)


class _MixtureLogProb(torch.autograd.Function):
    """lse[n] = logsumexp_k (log_softmax(mixture_logits)_k + log p_k(x_n)); backward recomputes the responsibilities
    from x and the saved per-row (max, sum) of the logsumexp. Parameter gradients go straight into FlatAdam's gradient sinks when they exist."""

    @staticmethod
    def forward(ctx, kind, x, mixture_logits, *params):
        lib = _lib.load()
        x = _chk(x, "mixture_log_prob.x")
        if x.dim() != 2:
            raise ValueError(f"mixture_log_prob: expected x of shape (N, n_features), got {tuple(x.shape)}")
        n, f = x.shape
        k = mixture_logits.numel()
        checked = [_chk(mixture_logits, "mixture_log_prob.mixture_logits")]
        if checked[0].dim() != 1:
            raise ValueError(f"mixture_log_prob: mixture_logits must be a vector, got {tuple(mixture_logits.shape)}")
        for p in params:
            p = _chk(p, "mixture_log_prob.parameter")
            if tuple(p.shape) != (k, f):
                raise ValueError(f"mixture_log_prob: parameter {tuple(p.shape)} != (n_components, n_features) = "
                                 f"({k}, {f})")
            checked.append(p)
        lse = torch.empty((n,), device=x.device, dtype=torch.float32)
        stats = torch.empty((n, 2), device=x.device, dtype=torch.float32)  # per row (max, sum) relative to component 0
        ws, floats = _workspace(lib.pg_mixture_workspace_floats(kind, n, k, f, 0), x.device)
        _lib.check(lib.pg_mixture_fwd(kind, x.data_ptr(), checked[0].data_ptr(), checked[1].data_ptr(),
                                      _p(checked[2]) if len(checked) > 2 else 0, lse.data_ptr(), stats.data_ptr(), n, k, f,
                                      ws.data_ptr(), floats, _stream()),
                   "pg_mixture_fwd")
        ctx.kind = kind
        ctx.sinks = [_sink(mixture_logits)] + [_sink(p) for p in params]
        ctx.save_for_backward(x, stats, *checked)
        return lse

    @staticmethod
    def backward(ctx, g):
        lib = _lib.load()
        x, stats, *pars = ctx.saved_tensors
        n, f = x.shape
        k = pars[0].numel()
        g = _chk(g, "mixture_log_prob.grad")
        need = ctx.needs_input_grad[2:]
        outs, ptrs = [], []
        for p, sink, wanted in zip(pars, ctx.sinks, need):
            if not wanted:
                outs.append(None)
                ptrs.append(0)
            elif sink is not None:
                outs.append(None)
                ptrs.append(sink.data_ptr())
            else:
                d = zeros(tuple(p.shape), x.device)
                outs.append(d)
                ptrs.append(d.data_ptr())
        ptrs += [0] * (3 - len(ptrs))
        if any(ptrs):
            ws, floats = _workspace(lib.pg_mixture_workspace_floats(ctx.kind, n, k, f, 1), x.device)
            _lib.check(lib.pg_mixture_bwd(ctx.kind, x.data_ptr(), pars[0].data_ptr(), pars[1].data_ptr(),
                                          pars[2].data_ptr() if len(pars) > 2 else 0, stats.data_ptr(), g.data_ptr(),
                                          ptrs[0], ptrs[1], ptrs[2], n, k, f, ws.data_ptr(), floats, _stream()),
                       "pg_mixture_bwd")
        return (None, None, *outs)


def mixture_log_prob(kind, x, mixture_logits, *params):
    """log p(x_n) = logsumexp_k (log_softmax(mixture_logits)_k + log p_k(x_n)) for x (N, n_features); returns (N,).

    kind "bernoulli": params = (logits (K, F),), log p_k(x) = sum_d x l - softplus(l), the reference's
    -binary_cross_entropy_with_logits, so real-valued x is accepted. kind "gaussian": params = (mean, log_std), both
    (K, F), diagonal normals. Differentiable in mixture_logits and the parameters; the input gradient is not
    implemented: an x that requires grad raises. mixture_logits that are all -inf give -inf (torch: NaN)."""
    if kind not in _KINDS:
        raise ValueError(f"mixture_log_prob: kind must be one of {sorted(_KINDS)}, got {kind!r}")
    kind_id, n_params = _KINDS[kind]
    if len(params) != n_params:
        raise ValueError(f"mixture_log_prob: kind {kind!r} takes {n_params} parameter tensor(s), got {len(params)}")
    if x.requires_grad and torch.is_grad_enabled():
        raise RuntimeError("mixture_log_prob: the gradient with respect to x is not implemented; pass x.detach()")
    return _MixtureLogProb.apply(kind_id, x, mixture_logits, *params)


def _kde_args(test, train, bandwidth, name):
    test, train = _chk(test, f"{name}.test"), _chk(train, f"{name}.train")
    if test.dim() != 2 or train.dim() != 2 or test.shape[1] != train.shape[1]:
        raise ValueError(f"{name}: expected test (M, d) and train (N, d), got {tuple(test.shape)} and "
                         f"{tuple(train.shape)}")
    if test.requires_grad or train.requires_grad:
        raise RuntimeError(f"{name}: no gradient is implemented; pass detached tensors")
    h = float(bandwidth)
    if not (h > 0 and np.isfinite(h)):
        raise ValueError(f"{name}: bandwidth must be positive and finite, got {bandwidth}")
    return test, train, h


def kde_gaussian(test, train, bandwidth):
    """log p(x) under a Gaussian kernel density estimate (kde.py GaussianKernel.forward): test (M, d), train (N, d) ->
    (M,). Memory: the output and a workspace of O(N + M * splits) floats; nothing of size M x N."""
    lib = _lib.load()
    test, train, h = _kde_args(test, train, bandwidth, "kde_gaussian")
    m, d = test.shape
    n = train.shape[0]
    out = torch.empty((m,), device=test.device, dtype=torch.float32)
    ws, floats = _workspace(lib.pg_kde_workspace_floats(m, n, d), test.device)
    _lib.check(lib.pg_kde_gaussian(test.data_ptr(), train.data_ptr(), h, out.data_ptr(), m, n, d, ws.data_ptr(), floats,
                                   _stream()),
               "pg_kde_gaussian")
    return out


def kde_parzen(test, train, bandwidth):
    """log p(x) under a Parzen window estimate (kde.py ParzenWindowKernel.forward): log(coef * count / N) with
    coef = 1 / bandwidth**d and count the training rows whose window contains the test row; -inf when none does.

    When coef overflows fp32 (e.g. bandwidth 0.1 at d = 784) the reference's `(coef * inside).mean()` is NaN unless
    every window contains the row (then +inf); the same values are returned here."""
    test, train, h = _kde_args(test, train, bandwidth, "kde_parzen")
    m, d = test.shape
    n = train.shape[0]
    with np.errstate(all="ignore"):
        coef = float(1 / np.float64(h) ** np.int64(d))  # as the reference: a double, rounded to fp32 where it is used
    out = torch.empty((m,), device=test.device, dtype=torch.float32)
    _lib.check(_lib.load().pg_kde_parzen(test.data_ptr(), train.data_ptr(), h, coef, out.data_ptr(), m, n, d, _stream()),
               "pg_kde_parzen")
    return out
