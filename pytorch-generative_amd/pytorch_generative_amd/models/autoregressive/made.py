"""Masked Autoencoder Distribution Estimator (MADE) on the MI355X path (reference models/autoregressive/made.py).

Same constructor, module layout and state_dict as the reference (`_net.{2i}.weight|bias|mask`, ReLU modules between
the MaskedLinear layers), so reference checkpoints load with strict=True. The masks are the reference's, drawn with
numpy's RandomState(mask_seed % n_masks) in `_sample_masks()`; what differs is where they live:

* the "degrees" (connectivity vectors) of each mask index are drawn once and cached on the device, D + sum(hidden)
  int32 per index (at most n_masks sets); the kernels evaluate the masks from them (csrc/masked_linear.hip), no dense
  mask is rebuilt on the host per forward;
* the `mask` buffers are written on the device from the degrees whenever the current mask index changes (or a buffer
  was overwritten from outside), so the state_dict holds the reference's masks;
* forward is one autograd Function over the whole network (ops.masked_mlp): masked GEMMs with the ReLU fused into
  the epilogues, `weight.data *= mask` done by the forward kernel, the reference's UNMASKED weight gradient.

Sampling: the reference (made.py:125-141) runs one full masked forward per dimension and uses one logit of it. With exactly one
hidden layer the work per dimension collapses to what NADE does: the hidden pre-activation a = b1 + W1m x changes by the rank-1
update a += x_i W1m[:, i] when dimension i is fixed, and the one logit needed is b2[i] + relu(a) . W2m[i, :]. sample() then
draws the whole batch in ONE launch (ops.made_sample_chain, csrc/made_sample.hip; route "chain"), from uniforms drawn once
per call: x_i = (u_i < sigmoid(l_i)). Same distribution as Bernoulli(logits=l_i), another random stream. Every other case —
`incremental=False`, a user `sample_fn`, no or several hidden layers, a shape the kernel's plan refuses — runs the reference's
procedure (route "full"); `_sample_route` tells which one the last call took.

hipGraph capture: with n_masks == 1 the mask never changes and the training step captures and replays
(graph.GraphedTrainStep, trainer.Trainer). With n_masks > 1 a captured step would freeze one mask, so forward RAISES
while a capture is open; `graph_capture_refusal()` tells the Trainer before it starts its warm-up steps, and it
trains eagerly instead (every forward then advances the mask index exactly as the reference's does).
"""

import numpy as np
import torch
from torch import nn

from pytorch_generative_amd import ops
from pytorch_generative_amd.models import base


class MaskedLinear(nn.Linear):
    """A Linear layer with masks that turn off some of the layer's weights (made.py:21-33)."""

    def __init__(self, in_features, out_features, bias=True):
        super().__init__(in_features, out_features, bias)
        self.register_buffer("mask", torch.ones((out_features, in_features)))

    def set_mask(self, mask):
        self.mask.data.copy_(mask)

    def forward(self, x):
        # weight.data *= mask (any float mask), then the plain linear layer; autograd never sees the mask
        ops.mul_mask_(self.weight, self.mask)
        return ops.masked_linear(x, self.weight, self.bias)


def connectivity(input_dim, dims, seed):
    """The reference's connectivity vectors for one mask seed (made.py:87-97), including its look-back of two layers
    for the lower bound of hidden layer i > 0 (`np.min(conn[i - 1])`)."""
    rng = np.random.RandomState(seed=seed)
    conn = [rng.permutation(input_dim)]
    for i, dim in enumerate(dims[1:-1]):
        low = 0 if i == 0 else np.min(conn[i - 1])
        high = input_dim - 1
        conn.append(rng.randint(low, high, size=dim))
    conn.append(np.copy(conn[0]))
    return conn


def masks_from_connectivity(conn):
    """The reference's uint8 masks of a connectivity (made.py:99-104)."""
    masks = [conn[i - 1][None, :] <= conn[i][:, None] for i in range(1, len(conn) - 1)]
    masks.append(conn[-2][None, :] < conn[-1][:, None])
    return [torch.from_numpy(mask.astype(np.uint8)) for mask in masks]


class MADE(base.AutoregressiveModel):
    """The Masked Autoencoder Distribution Estimator (MADE) model."""

    def __init__(self, input_dim, hidden_dims=None, n_masks=1, sample_fn=None):
        """input_dim: dimensionality D of the input; hidden_dims: units of each hidden layer; n_masks: number of
        distinct masks rotated through (one per forward); sample_fn: see the base class."""
        super().__init__(sample_fn)
        self._input_dim = input_dim
        self._dims = [self._input_dim] + (hidden_dims or []) + [self._input_dim]
        self._n_masks = n_masks
        self._mask_seed = 0

        layers = []
        for i in range(len(self._dims) - 1):
            in_dim, out_dim = self._dims[i], self._dims[i + 1]
            layers.append(MaskedLinear(in_dim, out_dim))
            layers.append(nn.ReLU())
        self._net = nn.Sequential(*layers[:-1])
        self._conn = {}      # mask index -> connectivity (host numpy)
        self._degrees = {}   # (mask index, device) -> int32 device vector conn[0] | conn[1] | ... | conn[-2]
        self._orders = {}    # (mask index, device) -> int32 device vector argsort(conn[-1]): the dimension drawn at each step
        self._sample_route = None  # "chain" or "full": what the last sample() call ran
        self._mask_index = None  # mask index whose masks the `mask` buffers hold
        self._mask_versions = None  # the buffers' version counters right after that write

    # ---- masks --------------------------------------------------------------------------------
    def _connectivity(self, index):
        conn = self._conn.get(index)
        if conn is None:
            conn = self._conn[index] = connectivity(self._input_dim, self._dims, index)
        return conn

    def _sample_masks(self):
        """Advances the mask seed and returns (uint8 masks, ordering) exactly as the reference (made.py:71-104)."""
        index = self._mask_seed % self._n_masks
        self._mask_seed += 1
        conn = self._connectivity(index)
        return masks_from_connectivity(conn), conn[-1]

    def graph_capture_refusal(self):
        """Why a training step of this model must not be captured into a hipGraph (None: it may be)."""
        if self._n_masks > 1:
            return (f"MADE with n_masks={self._n_masks} changes its mask every forward; a captured step would "
                    "replay one mask")
        return None

    def _next_mask_index(self):
        if self._n_masks > 1 and torch.cuda.is_available() and torch.cuda.is_current_stream_capturing():
            raise RuntimeError(self.graph_capture_refusal())
        index = self._mask_seed % self._n_masks
        self._mask_seed += 1
        return index

    def _masked_layers(self):
        return [m for m in self._net if isinstance(m, MaskedLinear)]

    def _layer_specs(self, index, device):
        """[(weight, bias, deg_in, deg_out, strict)] of every layer for mask `index`; writes the `mask` buffers on the
        device when the index changed."""
        key = (index, str(device))
        flat = self._degrees.get(key)
        conn = self._connectivity(index)
        if flat is None:
            flat = torch.from_numpy(np.concatenate(conn[:-1]).astype(np.int32)).to(device)
            self._degrees[key] = flat
        views, off = [], 0
        for c in conn[:-1]:
            views.append(flat[off:off + len(c)])
            off += len(c)
        views.append(views[0])  # conn[-1] is a copy of conn[0]
        layers = self._masked_layers()
        specs = []
        for i, layer in enumerate(layers):
            specs.append((layer.weight, layer.bias, views[i], views[i + 1], i == len(layers) - 1))
        # rewritten when the index changed or a buffer was written from outside (load_state_dict, set_mask, the
        # buffer rollback of GraphedTrainStep(preserve_state=True): a capture after it then carries the rewrite)
        if self._mask_index != key or self._mask_versions != [m.mask._version for m in layers]:
            for layer, (_, _, din, dout, strict) in zip(layers, specs):
                ops.mask_from_degrees(layer.mask, din, dout, strict)
            self._mask_index = key
            self._mask_versions = [m.mask._version for m in layers]
        return specs

    def _forward(self, x, index):
        self._no_input_codes()  # forward() and sample() both pass here
        return ops.masked_mlp(x, self._layer_specs(index, x.device))

    def _apply(self, fn, *args, **kwargs):
        self._mask_index = None
        return super()._apply(fn, *args, **kwargs)

    # ---- model --------------------------------------------------------------------------------
    @base.auto_reshape
    def forward(self, x):
        """x: (n, input_dim) vectors or (n, 1, h, w) images with h * w = input_dim; returns logits of x's shape."""
        return self._forward(x.contiguous(), self._next_mask_index())

    def _start_canvas(self, n_samples, conditioned_on):
        """As the base class; a model that has seen no image batch (no recorded shape) starts from (n_samples, input_dim)."""
        if conditioned_on is None and n_samples is not None and getattr(self, "_c", None) is None:
            return torch.full((n_samples, self._input_dim), -1.0, device=self.device)
        return super()._start_canvas(n_samples, conditioned_on)

    def _route(self, n, incremental):
        """"chain" when the one-launch sampler applies: asked for, exactly one hidden layer, the base class's Bernoulli draw
        (a user `sample_fn` sees every logit vector, so it keeps the reference's procedure) and a shape the plan accepts."""
        if (incremental and len(self._dims) == 3 and self._sample_fn is base._bernoulli_from_logits
                and ops.made_sample_plan(self._input_dim, self._dims[1], n) is not None):
            return "chain"
        return "full"

    @torch.no_grad()
    def sample(self, n_samples=None, conditioned_on=None, *, incremental=True, return_logits=False, generator=None):
        """Fills the entries of `conditioned_on` that are < 0 (made.py:125-141): one mask draw, then the dimensions in the
        order argsort(ordering), each from the logit its predecessors give it. `conditioned_on` is not modified.

        incremental (extension): a network with one hidden layer and the default Bernoulli `sample_fn` is drawn in one launch
        on cached hidden sums (ops.made_sample_chain) instead of one full forward per dimension. That route draws
        x_i = (u_i < sigmoid(l_i)) from uniforms u = torch.rand((n, D), generator=generator) made once per call: the same
        distribution as the reference's Bernoulli(logits), but another random stream, so a seeded run differs from
        incremental=False (as with the other incremental samplers). Mask rotation, the `mask` buffers and the in-place masking
        of both weights are what one forward would leave. `_sample_route` is "chain" or "full" afterwards.
        return_logits (extension, "chain" only): also returns logits shaped like the sample, logits[n, i] being the logit
        dimension i was decided from (for a given entry: the one it would have been drawn from).
        generator (extension): the torch.Generator of the uniforms (one of the model's device); the "full" route draws through
        `sample_fn` and ignores it."""
        canvas = self._start_canvas(n_samples, conditioned_on)
        self._sample_route = self._route(canvas.shape[0], incremental)
        if self._sample_route == "chain":
            return self._sample_chain(canvas, return_logits, generator)
        if return_logits:
            raise ValueError("MADE.sample: return_logits needs the one-launch route (one hidden layer, the default sample_fn, "
                             "incremental=True)")
        return self._sample(canvas)

    def _order(self, index, device):
        key = (index, str(device))
        order = self._orders.get(key)
        if order is None:
            order = torch.from_numpy(np.argsort(self._connectivity(index)[-1]).astype(np.int32)).to(device)
            self._orders[key] = order
        return order

    def _sample_chain(self, canvas, return_logits, generator):
        index = self._next_mask_index()
        self._no_input_codes()
        shape = canvas.shape
        x = canvas.contiguous().view(shape[0], -1)
        self._layer_specs(index, x.device)  # the `mask` buffers of this index
        hidden, out = self._masked_layers()
        for layer in (hidden, out):  # weight.data *= mask, as the forward leaves it: the kernel evaluates no mask
            ops.mul_mask_(layer.weight, layer.mask)
        uniforms = torch.rand(x.shape, device=x.device, generator=generator)
        got = ops.made_sample_chain(x, hidden.weight.data, hidden.bias.data, out.weight.data, out.bias.data,
                                    self._order(index, x.device), uniforms, return_logits=return_logits)
        if return_logits:
            return got[0].view(shape), got[1].view(shape)
        return got.view(shape)

    @base.auto_reshape
    def _sample(self, x):
        index = self._next_mask_index()
        ordering = np.argsort(self._connectivity(index)[-1])
        for dim in ordering:
            out = self._forward(x, index)[:, dim]
            out = self._sample_fn(out)
            x[:, dim] = torch.where(x[:, dim] < 0, out, x[:, dim])
        return x


def reproduce(n_epochs=85, batch_size=64, log_dir="/tmp/run", n_gpus=1, device_id=0, debug_loader=None):
    """The reference's training recipe for this model (made.py:144-205: MADE(784, [8000], n_masks=1), Adam at its
    defaults, BCE with logits summed per image and averaged over the batch) on the MI355X path. Arguments as the
    reference; `debug_loader` replaces both loaders (any iterable of (x, y) batches). Returns the Trainer."""
    from pytorch_generative_amd import recipes

    return recipes.run(
        lambda: MADE(input_dim=784, hidden_dims=[8000], n_masks=1),
        loaders=recipes.binarized_mnist, loss_fn=recipes.bce_loss, lr=1e-3,
        n_epochs=n_epochs, batch_size=batch_size, log_dir=log_dir, n_gpus=n_gpus,
        device_id=device_id, debug_loader=debug_loader)
