"""Non-linear Independent Components Estimation (NICE) on the MI355X path (reference models/flow/nice.py).

Same constructors, defaults, initialisation (nn.Linear's, `log_scale` zeros) and state_dict keys as the reference
(`net.{b}.net.{0,2,..}.weight/bias`, `scaling.log_scale`, plus `_c/_h/_w` once a 4-D batch was seen), so reference checkpoints
load with strict=True.

A coupling block is one autograd node (ops.coupling) over the dense fp32-MFMA GEMMs of csrc/dense_linear.hip: the network reads
one half of the (N, F) activation in place through a row stride, the last layer's epilogue adds its result to the other half
(y2 = x2 + m(x1)), ReLU and its derivative ride in the epilogues; no torch.cat, no slicing copy. The scaling layer and the
logistic prior are streaming kernels (ops.nice_scale, ops.logistic_logprob). `_inverse` is the same kernels with sign = -1 and
the blocks reversed. Everything is fp32-exact, free of float atomics and bit-identical from run to run, and the training step
captures into a hipGraph.

The class lives in `models.flows.nice` (package `flows`, plural). There is no top-level `models.NICE` and nothing named
`models.flow`: the drop-in alias keeps the reference's two names as raising placeholders (compat.py).

sample() keeps the reference's distribution (standard normal times `temp`, nice.py:149-154) but draws on the device, i.e. from
another random stream than the reference's CPU draw.
"""

import torch
from torch import nn

from pytorch_generative_amd import ops
from pytorch_generative_amd.models import base


class AdditiveCouplingBlock(nn.Module):
    """One additive coupling step over the two halves (a, b) of the features: `forward` leaves a as it is and shifts b by
    m(a), m being the block's ReLU network; `inverse` shifts back by the same m(a). With `reverse` the halves swap roles."""

    def __init__(self, n_features, n_hidden_layers, n_hidden_features, reverse):
        """n_features: number of input and output features (even); n_hidden_layers: hidden layers of the coupling network;
        n_hidden_features: features of each hidden layer; reverse: whether to reverse which half the network transforms."""
        super().__init__()
        if n_features % 2 or n_features < 2:
            raise ValueError(f"AdditiveCouplingBlock: n_features = {n_features} must be even (the halves are coupled one to one)")
        self.reverse = reverse
        half_features = n_features // 2
        net = [nn.Linear(in_features=half_features, out_features=n_hidden_features), nn.ReLU()]
        for _ in range(n_hidden_layers - 1):
            net.append(nn.Linear(in_features=n_hidden_features, out_features=n_hidden_features))
            net.append(nn.ReLU())
        net.append(nn.Linear(in_features=n_hidden_features, out_features=half_features))
        self.net = nn.Sequential(*net)

    def _couple(self, x, sign):
        layers = [(m.weight, m.bias) for m in self.net if isinstance(m, nn.Linear)]
        return ops.coupling(x.contiguous(), layers, self.reverse, sign)

    def forward(self, x):
        """Data towards the prior: the transformed half + m(the other half)."""
        return self._couple(x, 1)

    def inverse(self, y):
        """Prior towards the data: the transformed half - m(the other half)."""
        return self._couple(y, -1)


class ScalingLayer(nn.Module):
    """Multiplies feature j by exp(log_scale[j]): a diagonal, hence invertible, linear map."""

    def __init__(self, n_features):
        super().__init__()
        self.log_scale = nn.Parameter(torch.zeros((1, n_features)))

    def log_det_J(self):
        """The map is diagonal, so the log-determinant of its Jacobian is the sum of the log-scales."""
        return torch.sum(self.log_scale)

    def _couple(self, x, sign):
        original_shape = x.shape
        h = ops.nice_scale(x.contiguous().view(original_shape[0], -1), self.log_scale, sign)
        return h.view(original_shape)

    def forward(self, x):
        """Data towards the prior: times exp(log_scale)."""
        return self._couple(x, 1)

    def inverse(self, y):
        """Prior towards the data: times exp(-log_scale)."""
        return self._couple(y, -1)


class NICE(base.GenerativeModel):
    """The NICE flow: coupling blocks that alternate the half they transform, then one scaling layer."""

    def __init__(self, n_features, n_coupling_blocks=4, n_hidden_layers=5, n_hidden_features=1000):
        """n_features: number of input and output features (even: the reference's forward fails on odd widths, here the
        constructor raises ValueError); n_coupling_blocks: should be at least 3 for all dimensions to influence one another;
        n_hidden_layers: hidden layers per coupling block; n_hidden_features: features of each hidden layer."""
        super().__init__()
        if n_features % 2 or n_features < 2:
            raise ValueError(f"NICE: n_features = {n_features} must be even (the halves are coupled one to one)")
        net = []
        reverse = False
        for _ in range(n_coupling_blocks):
            net.append(AdditiveCouplingBlock(n_features=n_features, n_hidden_layers=n_hidden_layers,
                                             n_hidden_features=n_hidden_features, reverse=reverse))
            reverse = not reverse
        self.net = nn.Sequential(*net)
        self.scaling = ScalingLayer(n_features)

    def forward(self, x):
        """Maps a batch to the prior's space: returns (z shaped like x, log_det_J of the whole map, a scalar)."""
        return self._forward(x), self.scaling.log_det_J()

    @base.auto_reshape
    def _forward(self, x):
        y = self.net(x)
        return self.scaling(y)

    @torch.no_grad()
    def sample(self, n_samples, temp=1.0, generator=None):
        """See the base class. temp: the temperature, i.e. the scale of the standard-normal draw (the reference samples from the
        normal for both priors, nice.py:149-151). generator (extension): the torch.Generator of the draw (one of the model's
        device). The draw is made on the device: the reference's distribution on another random stream."""
        if getattr(self, "_c", None) is None:
            raise RuntimeError("NICE.sample: no image shape registered yet (call the model on a 4-D batch or load a checkpoint)")
        shape = (n_samples, int(self._c), int(self._h), int(self._w))
        x = torch.randn(shape, device=self.device, generator=generator) * temp
        return self._inverse(x)

    @base.auto_reshape
    def _inverse(self, x):
        x = self.scaling.inverse(x)
        for block in reversed(self.net):
            x = block.inverse(x)
        return x


def reproduce(n_epochs=150, batch_size=1024, log_dir="/tmp/run", n_gpus=1, device_id=0, debug_loader=None):
    """The reference's training recipe for this model (nice.py:164-226: NICE(784, 4 blocks, 5 hidden layers of 1000), Adam at
    lr 1e-3, dequantized MNIST, the logistic prior) on the MI355X path. Arguments as the reference; `debug_loader` replaces
    both loaders (any iterable of (x, y) batches). Returns the Trainer."""
    from pytorch_generative_amd import recipes

    return recipes.run(
        lambda: NICE(n_features=784, n_coupling_blocks=4, n_hidden_layers=5, n_hidden_features=1000),
        loaders=recipes.dequantized_mnist, loss_fn=recipes.nice_loss, lr=1e-3,
        n_epochs=n_epochs, batch_size=batch_size, log_dir=log_dir, n_gpus=n_gpus,
        device_id=device_id, debug_loader=debug_loader)
