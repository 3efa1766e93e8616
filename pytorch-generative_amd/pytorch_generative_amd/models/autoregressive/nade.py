"""Neural Autoregressive Distribution Estimator (NADE) on the MI355X path (reference models/autoregressive/nade.py).

Same constructor, initialisation (kaiming_normal_ on both weights, zero biases) and state_dict keys as the reference (`_in_W`
(H, D), `_in_b` (H), `_h_W` (D, H), `_h_b` (D)), so reference checkpoints load with strict=True.

forward is one autograd Function over the whole model (ops.nade, csrc/nade.hip): the reference's Python loop over the D
dimensions — a_0 = _in_b, p_i = sigmoid(_h_b[i] + relu(a_i) . _h_W[i, :]), a_{i+1} = a_i + x_i _in_W[:, i] — runs as a chunked
prefix scan, two launches forward and four backward, and the training step captures into a hipGraph. forward returns the
PROBABILITIES p in the shape of x, as the reference does. It uses x as given (teacher forcing): the reference draws the entries
of x that are negative inside its forward; here only sample() draws.

The reference's recipe feeds these probabilities to binary_cross_entropy_with_logits, i.e. it treats p as if it were a logit.
reproduce() keeps that quirk: recipes.bce_loss on what forward returns.

Sampling: the reference walks the dimensions once, drawing x_i ~ Bernoulli(p_i) where it is not given. That is what the
one-launch sampler of a one-hidden-layer MADE does with the identity order (ops.made_sample_chain, csrc/made_sample.hip):
sample() runs it with w1 = _in_W, w2 = _h_W, order = arange(D) and uniforms u = torch.rand((n, D), generator=generator),
x_i = (u_i < p_i) — Bernoulli(probs=p_i) on another random stream (route "chain"). `incremental=False`, or a shape
ops.made_sample_plan refuses, runs the reference's per-dimension procedure in eager torch (route "full"); `_sample_route`
tells which one the last call took.
"""

import torch
from torch import nn

from pytorch_generative_amd import ops
from pytorch_generative_amd.models import base


class NADE(base.AutoregressiveModel):
    """The Neural Autoregressive Distribution Estimator (NADE) model."""

    def __init__(self, input_dim, hidden_dim, sample_fn=None):
        """input_dim: dimensionality D of the input; hidden_dim: units of the one hidden layer; sample_fn: see the base class
        (unused, as in the reference: NADE draws from Bernoulli(probs=p_i))."""
        super().__init__(sample_fn)
        self._input_dim = input_dim
        self._in_W = nn.Parameter(torch.zeros(hidden_dim, self._input_dim))
        self._in_b = nn.Parameter(torch.zeros(hidden_dim))
        self._h_W = nn.Parameter(torch.zeros(self._input_dim, hidden_dim))
        self._h_b = nn.Parameter(torch.zeros(self._input_dim))
        nn.init.kaiming_normal_(self._in_W)
        nn.init.kaiming_normal_(self._h_W)
        self._orders = {}  # device -> int32 arange(D)
        self._sample_route = None  # "chain" or "full": what the last sample() call ran

    @base.auto_reshape
    def forward(self, x):
        """x: (n, input_dim) vectors or (n, 1, h, w) images with h * w = input_dim; returns the probabilities in x's shape."""
        self._no_input_codes()
        return ops.nade(x.contiguous(), self._in_W, self._in_b, self._h_W, self._h_b)

    def _start_canvas(self, n_samples, conditioned_on):
        """As the base class; a model that has seen no image batch (no recorded shape) starts from (n_samples, input_dim)."""
        if conditioned_on is None and n_samples is not None and getattr(self, "_c", None) is None:
            return torch.full((n_samples, self._input_dim), -1.0, device=self.device)
        return super()._start_canvas(n_samples, conditioned_on)

    def _route(self, n, incremental):
        """"chain" when the one-launch sampler applies: asked for, and a shape its plan accepts."""
        if incremental and ops.made_sample_plan(self._input_dim, self._in_W.shape[0], n) is not None:
            return "chain"
        return "full"

    @staticmethod
    def _uniforms(shape, device, generator):
        return torch.rand(shape, device=device, generator=generator)

    @staticmethod
    def _draw(p):
        return torch.bernoulli(p)

    @torch.no_grad()
    def sample(self, n_samples=None, conditioned_on=None, *, incremental=True, return_logits=False, generator=None):
        """Fills the entries of `conditioned_on` that are < 0 (nade.py:54-66), dimension by dimension, each from the
        probability its predecessors give it. `conditioned_on` is not modified.

        incremental (extension): the whole batch is drawn in one launch on cached hidden sums (ops.made_sample_chain with the
        identity order): x_i = (u_i < p_i) from uniforms u = torch.rand((n, D), generator=generator) made once per call — the
        reference's Bernoulli(probs=p_i) on another random stream, so a seeded run differs from incremental=False.
        `_sample_route` is "chain" or "full" afterwards.
        return_logits (extension, "chain" only): also returns logits shaped like the sample, logits[n, i] being the logit
        dimension i was decided from (for a given entry: the one it would have been drawn from).
        generator (extension): the torch.Generator of the uniforms (one of the model's device); the "full" route draws with
        torch.bernoulli and ignores it."""
        self._no_input_codes()
        canvas = self._start_canvas(n_samples, conditioned_on)
        self._sample_route = self._route(canvas.shape[0], incremental)
        if self._sample_route == "chain":
            return self._sample_chain(canvas, return_logits, generator)
        if return_logits:
            raise ValueError("NADE.sample: return_logits needs the one-launch route (incremental=True)")
        return self._sample_full(canvas)

    def _order(self, device):
        order = self._orders.get(str(device))
        if order is None:
            order = self._orders[str(device)] = torch.arange(self._input_dim, dtype=torch.int32, device=device)
        return order

    def _sample_chain(self, canvas, return_logits, generator):
        shape = canvas.shape
        x = canvas.contiguous().view(shape[0], -1)
        uniforms = self._uniforms(x.shape, x.device, generator)
        got = ops.made_sample_chain(x, self._in_W.data, self._in_b.data, self._h_W.data, self._h_b.data, self._order(x.device),
                                    uniforms, return_logits=return_logits)
        if return_logits:
            return got[0].view(shape), got[1].view(shape)
        return got.view(shape)

    @base.auto_reshape
    def _sample_full(self, x):
        """The reference's procedure (nade.py:49-68) in eager torch."""
        if not x.is_cuda:
            raise RuntimeError(f"NADE.sample: expected a tensor on the MI355X (cuda) device, got {x.device}")
        a = self._in_b.expand(x.shape[0], -1)
        out = []
        for i in range(self._input_dim):
            p_i = torch.sigmoid(torch.relu(a) @ self._h_W[i:i + 1, :].t() + self._h_b[i:i + 1])
            x_i = x[:, i:i + 1]
            x_i = torch.where(x_i < 0, self._draw(p_i), x_i)
            out.append(x_i)
            a = a + x_i @ self._in_W[:, i:i + 1].t()
        return torch.cat(out, dim=1)


def reproduce(n_epochs=50, batch_size=512, log_dir="/tmp/run", n_gpus=1, device_id=0, debug_loader=None):
    """The reference's training recipe for this model (nade.py:93-146: NADE(784, 500), Adam at its defaults, dynamically
    binarized MNIST, binary_cross_entropy_with_logits applied to the PROBABILITIES forward returns, summed per image and
    averaged over the batch) on the MI355X path. Arguments as the reference; `debug_loader` replaces both loaders (any iterable
    of (x, y) batches). Returns the Trainer."""
    from pytorch_generative_amd import recipes

    return recipes.run(
        lambda: NADE(input_dim=784, hidden_dim=500),
        loaders=recipes.binarized_mnist, loss_fn=recipes.bce_loss, lr=1e-3,
        n_epochs=n_epochs, batch_size=batch_size, log_dir=log_dir, n_gpus=n_gpus,
        device_id=device_id, debug_loader=debug_loader)
