"""Kernel density estimation on the MI355X path (reference models/kde.py).

p(x) = 1 / |D| sum_{x_i in D} K(u(x, x_i)) with a kernel K placed on every point of a "training" set D. Same classes
and constructors as the reference. The reference's forward materialises the (test, train, d) difference tensor (its
TODO: "consumes O(train_Xs * x) memory"); here the Gaussian kernel is a GEMM with a streaming logsumexp and the Parzen
window a counting kernel with an early exit per pair (ops.kde_gaussian, ops.kde_parzen, csrc/density.hip): memory is
the inputs, the output and a workspace of O(train + test * splits) floats. Both kernels take 2-D inputs."""

import abc

import numpy as np
import torch
from torch import nn

from pytorch_generative_amd import ops
from pytorch_generative_amd.models import base


class Kernel(abc.ABC, nn.Module):
    """Base class which defines the interface for all kernels."""

    def __init__(self, bandwidth=1.0):
        """bandwidth: the kernel's (band)width."""
        super().__init__()
        self.bandwidth = bandwidth

    @abc.abstractmethod
    def forward(self, test_Xs, train_Xs):
        """Computes log p(x) for each x in test_Xs given train_Xs."""

    @abc.abstractmethod
    def sample(self, train_Xs):
        """Generates samples from the kernel distribution."""


class ParzenWindowKernel(Kernel):
    """The Parzen window kernel. Where 1 / bandwidth**d overflows fp32 the reference returns NaN (+inf if every window
    contains the point); so does this (ops.kde_parzen)."""

    def forward(self, test_Xs, train_Xs):
        return ops.kde_parzen(test_Xs, train_Xs, self.bandwidth)

    @torch.no_grad()
    def sample(self, train_Xs):
        device = train_Xs.device
        noise = (torch.rand(train_Xs.shape, device=device) - 0.5) * self.bandwidth
        return train_Xs + noise


class GaussianKernel(Kernel):
    """The Gaussian kernel."""

    def forward(self, test_Xs, train_Xs):
        return ops.kde_gaussian(test_Xs, train_Xs, self.bandwidth)

    @torch.no_grad()
    def sample(self, train_Xs):
        device = train_Xs.device
        noise = torch.randn(train_Xs.shape, device=device) * self.bandwidth
        return train_Xs + noise


class KernelDensityEstimator(base.GenerativeModel):
    """The KernelDensityEstimator model."""

    def __init__(self, train_Xs, kernel=None):
        """train_Xs: the "training" data to use when estimating probabilities (a plain attribute: the state_dict is
        empty); kernel: the kernel to place on each of the train_Xs (default: GaussianKernel())."""
        super().__init__()
        self.kernel = kernel or GaussianKernel()
        self.train_Xs = train_Xs
        assert len(self.train_Xs.shape) == 2, "Input cannot have more than two axes."

    @property
    def device(self):
        return self.train_Xs.device

    def forward(self, x):
        return self.kernel(x, self.train_Xs)

    @torch.no_grad()
    def sample(self, n_samples):
        idxs = np.random.choice(range(len(self.train_Xs)), size=n_samples)
        return self.kernel.sample(self.train_Xs[idxs])
