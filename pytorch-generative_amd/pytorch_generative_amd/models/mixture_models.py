"""Mixture models on the MI355X path (reference models/mixture_models.py).

Same constructors, parameter names, shapes and initialisers as the reference, so its state_dicts load with strict=True,
and the same shape conventions: `__call__` views x as (n, 1, n_features) and remembers `_original_shape`;
GaussianMixtureModel.forward returns (n, 1), BernoulliMixtureModel.forward returns (n,). What differs is the arithmetic:
the reference materialises an (n, n_components, n_features) tensor per elementwise op, forward and backward; here
log_softmax(mixture_logits) + the component log-likelihoods + logsumexp are one streaming kernel chain
(ops.mixture_log_prob, csrc/density.hip) whose backward recomputes the responsibilities tile by tile. The gradient
with respect to x is not implemented (an x that requires grad raises)."""

import abc

import torch
from torch import distributions, nn

from pytorch_generative_amd import ops
from pytorch_generative_amd.models import base


class MixtureModel(base.GenerativeModel):
    """Base class of the mixture models: a generic `forward()` (log likelihood of the input) and `sample()`;
    subclasses define `_log_prob()` and `_component_sample()`."""

    def __init__(self, n_components, n_features):
        """n_components: number of component distributions; n_features: dimensions of each component."""
        super().__init__()
        self.n_components = n_components
        self.n_features = n_features
        self.mixture_logits = nn.Parameter(torch.ones((n_components,)))

    @abc.abstractmethod
    def _log_prob(self, x):
        """log p(x) of the (n, n_features) batch as an (n,) vector."""

    def __call__(self, *args, **kwargs):
        x = args[0]
        self._original_shape = x.shape
        x = x.view(self._original_shape[0], 1, self.n_features)
        args = (x, *args[1:])
        return super().__call__(*args, **kwargs)

    def forward(self, x):
        return self._log_prob(x.reshape(x.shape[0], self.n_features))

    @abc.abstractmethod
    def _component_sample(self, idxs):
        """Returns samples from the component distributions conditioned on idxs."""

    @torch.no_grad()
    def sample(self, n_samples):
        shape = (n_samples,)
        idxs = distributions.Categorical(logits=self.mixture_logits).sample(shape)
        sample = self._component_sample(idxs)
        return sample.view(n_samples, *self._original_shape[1:])


class GaussianMixtureModel(MixtureModel):
    """A categorical mixture of Gaussian distributions with diagonal covariance."""

    def __init__(self, n_components, n_features):
        super().__init__(n_components, n_features)
        self.mean = nn.Parameter(torch.randn(n_components, n_features) * 0.01)
        # var = 1 <=> log(sqrt(var)) = 0
        self.log_std = nn.Parameter(torch.zeros(n_components, n_features))

    def _log_prob(self, x):
        # the reference broadcasts (n, 1, 1, F) against (K, F) and reduces the last two axes: (n, 1)
        return ops.mixture_log_prob("gaussian", x, self.mixture_logits, self.mean, self.log_std).view(-1, 1)

    def _component_sample(self, idxs):
        mean, std = self.mean[idxs], self.log_std[idxs].exp()
        return distributions.Normal(mean, std).sample()


class BernoulliMixtureModel(MixtureModel):
    """A categorical mixture of Bernoulli distributions."""

    def __init__(self, n_components, n_features):
        super().__init__(n_components, n_features)
        self.logits = nn.Parameter(torch.rand(n_components, n_features))

    def _log_prob(self, x):
        # (n, 1, F) against (K, F) broadcasts to (n, K, F) in the reference: (n,)
        return ops.mixture_log_prob("bernoulli", x, self.mixture_logits, self.logits)

    def _component_sample(self, idxs):
        logits = self.logits[idxs]
        return distributions.Bernoulli(logits=logits).sample()
