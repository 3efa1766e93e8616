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

    @torch.no_grad()
    def sample(self, n_samples=None, conditioned_on=None):
        """Fills the entries of `conditioned_on` that are < 0 (made.py:125-141): one mask draw, then one full forward
        per dimension in the order argsort(ordering)."""
        conditioned_on = self._start_canvas(n_samples, conditioned_on)
        return self._sample(conditioned_on)

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
