"""Fully Visible Belief Network (FVBN) on the MI355X path (reference models/autoregressive/fvbn.py).

The reference holds D separate `nn.Linear(max(1, i), 1)` modules and runs them in a Python loop; the mathematics is one strictly
lower-triangular product, logits = x tril(W, -1)^T + b. Here the model holds exactly two parameters:

  `_weight` (P(D),): the rows of the strictly lower triangle one after another. Row i holds max(1, i) values, the reference's
      `_net.i.weight` (row 0: the dummy weight the reference multiplies by a zero input), followed by zeros up to a multiple of
      4 floats; row i starts at ops.fvbn_offsets(D)[i]. The pads are zero at construction, receive exactly zero gradient and
      therefore stay zero under Adam; so does the gradient of row 0.
  `_bias` (D,): `_bias[i]` is `_net.i.bias`.

state_dict() / load_state_dict() speak the reference's language: the keys are `_net.0.weight`, `_net.0.bias`, `_net.1.weight`, ...
with the reference's shapes (plus `_c`, `_h`, `_w` once an image batch was seen), so reference checkpoints load with strict=True
and round-trip; `_weight` and `_bias` never appear as keys. Initialisation follows nn.Linear's default distribution: row i and
bias i uniform in +-1/sqrt(max(1, i)) (another random stream than the reference's).

Stated deviation: parameters() yields 2 tensors, not 1568, so an optimiser state_dict of the reference does not load. Adam is
elementwise, so the trajectory of every weight is the reference's.

forward is one autograd Function (ops.fvbn, csrc/fvbn.hip): a triangular fp32-MFMA GEMM on the packed weight, its weight
gradient written straight into the packed layout (FlatAdam's sink); the training step captures into a hipGraph.

Sampling: the reference runs one full forward per dimension. sample() draws the whole batch in one launch
(ops.fvbn_sample_chain) from uniforms u = torch.rand((n, D), generator=generator), x_i = (u_i < sigmoid(l_i)) — the reference's
Bernoulli(logits) on another random stream (route "chain"). `incremental=False`, a user `sample_fn` or a shape ops.fvbn_plan
refuses runs the reference's procedure, one forward per dimension through `sample_fn` (route "full"); `_sample_route` tells
which one the last call took.
"""

import math

import torch
from torch import nn

from pytorch_generative_amd import ops
from pytorch_generative_amd.models import base


class FullyVisibleBeliefNetwork(base.AutoregressiveModel):
    """The Fully Visible Belief Network."""

    def __init__(self, n_dims, sample_fn=None):
        """n_dims: number of input (and output) dimensions D; sample_fn: see the base class (a user sample_fn selects the
        "full" sampling route)."""
        super().__init__(sample_fn)
        self._default_sample_fn = sample_fn is None
        self.n_dims = n_dims
        off = ops.fvbn_offsets(n_dims)
        self._offsets = off.tolist()
        row = torch.repeat_interleave(torch.arange(n_dims), off[1:] - off[:-1])  # the row of every packed element
        col = torch.arange(int(off[-1])) - off[row]
        length = row.clamp_min(1)
        bound = length.float().rsqrt()
        weight = (torch.rand(int(off[-1])) * 2 - 1) * bound * (col < length)
        bias = (torch.rand(n_dims) * 2 - 1) * torch.arange(n_dims).clamp_min(1).float().rsqrt()
        self._weight = nn.Parameter(weight)
        self._bias = nn.Parameter(bias)
        self._sample_route = None  # "chain" or "full": what the last sample() call ran

    @staticmethod
    def _row_len(i):
        return max(1, i)

    # ---- the reference's state_dict: _net.i.weight (1, max(1, i)), _net.i.bias (1) ----------------------------------------
    def _save_to_state_dict(self, destination, prefix, keep_vars):
        for name, buf in self._buffers.items():
            if buf is not None and name not in self._non_persistent_buffers_set:
                destination[prefix + name] = buf if keep_vars else buf.detach()
        weight = self._weight if keep_vars else self._weight.detach()
        bias = self._bias if keep_vars else self._bias.detach()
        for i in range(self.n_dims):
            o, n = self._offsets[i], self._row_len(i)
            destination[f"{prefix}_net.{i}.weight"] = weight[o:o + n].view(1, n)
            destination[f"{prefix}_net.{i}.bias"] = bias[i:i + 1]

    def _load_from_state_dict(self, state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs):
        expected = set()
        weight = self._weight.detach().cpu().clone()
        bias = self._bias.detach().cpu().clone()
        for i in range(self.n_dims):
            o, n = self._offsets[i], self._row_len(i)
            for kind, shape, target in (("weight", (1, n), weight[o:o + n]), ("bias", (1,), bias[i:i + 1])):
                key = f"{prefix}_net.{i}.{kind}"
                expected.add(key)
                value = state_dict.get(key)
                if value is None:
                    missing_keys.append(key)
                elif tuple(value.shape) != shape:
                    error_msgs.append(f"size mismatch for {key}: copying a param with shape {tuple(value.shape)} from checkpoint, "
                                      f"the shape in current model is {shape}.")
                else:
                    target.copy_(value.detach().reshape(-1))
        with torch.no_grad():
            self._weight.copy_(weight)  # the pads were zero and no row writes them
            self._bias.copy_(bias)
            for name, buf in self._buffers.items():
                key = prefix + name
                expected.add(key)
                if key not in state_dict:
                    missing_keys.append(key)
                elif tuple(state_dict[key].shape) != tuple(buf.shape):
                    error_msgs.append(f"size mismatch for {key}: copying a param with shape {tuple(state_dict[key].shape)} from "
                                      f"checkpoint, the shape in current model is {tuple(buf.shape)}.")
                else:
                    buf.copy_(state_dict[key])
        unexpected_keys.extend(k for k in state_dict if k.startswith(prefix) and k not in expected)

    # ---- forward ------------------------------------------------------------------------------------------------------------
    @base.auto_reshape
    def forward(self, x):
        """x: (n, n_dims) vectors or (n, 1, h, w) images with h * w = n_dims; returns the logits in x's shape."""
        self._no_input_codes()
        return ops.fvbn(x.contiguous(), self._weight, self._bias)

    # ---- sampling -----------------------------------------------------------------------------------------------------------
    def _start_canvas(self, n_samples, conditioned_on):
        """As the base class; a model that has seen no image batch (no recorded shape) starts from (n_samples, n_dims)."""
        if conditioned_on is None and n_samples is not None and getattr(self, "_c", None) is None:
            return torch.full((n_samples, self.n_dims), -1.0, device=self.device)
        return super()._start_canvas(n_samples, conditioned_on)

    def _route(self, n, incremental):
        """"chain" when the one-launch sampler applies: asked for, the default sample_fn, and a shape the plan accepts."""
        if incremental and self._default_sample_fn and ops.fvbn_plan(self.n_dims, n) is not None:
            return "chain"
        return "full"

    @staticmethod
    def _uniforms(shape, device, generator):
        return torch.rand(shape, device=device, generator=generator)

    @torch.no_grad()
    def sample(self, n_samples=None, conditioned_on=None, *, incremental=True, return_logits=False, generator=None):
        """Fills the entries of `conditioned_on` that are < 0, dimension by dimension, each from the logit its predecessors
        give it (reference models/base.py:97-120). `conditioned_on` is not modified.

        incremental (extension): the whole batch is drawn in one launch (ops.fvbn_sample_chain): x_i = (u_i < sigmoid(l_i))
        from uniforms u = torch.rand((n, D), generator=generator) made once per call — the reference's Bernoulli(logits) on
        another random stream. Taken when `sample_fn` is the default and ops.fvbn_plan accepts the shape; otherwise, and with
        incremental=False, the reference's one forward per dimension through `sample_fn` runs. `_sample_route` is "chain" or
        "full" afterwards.
        return_logits (extension, "chain" only): also returns logits shaped like the sample, logits[n, i] being the logit
        dimension i was decided from (for a given entry: the one it would have been drawn from).
        generator (extension): the torch.Generator of the uniforms (one of the model's device); the "full" route ignores it."""
        self._no_input_codes()
        canvas = self._start_canvas(n_samples, conditioned_on)
        self._sample_route = self._route(canvas.shape[0], incremental)
        if self._sample_route == "chain":
            shape = canvas.shape
            x = canvas.contiguous().view(shape[0], -1)
            uniforms = self._uniforms(x.shape, x.device, generator)
            got = ops.fvbn_sample_chain(x, self._weight.data, self._bias.data, uniforms, return_logits=return_logits)
            if return_logits:
                return got[0].view(shape), got[1].view(shape)
            return got.view(shape)
        if return_logits:
            raise ValueError("FullyVisibleBeliefNetwork.sample: return_logits needs the one-launch route (incremental=True, "
                             "the default sample_fn)")
        return self._sample_full(canvas)

    @base.auto_reshape
    def _sample_full(self, x):
        """The reference's procedure: one full forward per dimension, `sample_fn` on that dimension's logits."""
        x = x.contiguous()
        for i in range(self.n_dims):
            drawn = self._sample_fn(ops.fvbn(x, self._weight, self._bias)[:, i])
            x[:, i] = torch.where(x[:, i] < 0, drawn, x[:, i])
        return x


def reproduce(n_epochs=50, batch_size=512, log_dir="/tmp/run", n_gpus=1, device_id=0, debug_loader=None):
    """The reference's training recipe for this model (fvbn.py:48-97: FullyVisibleBeliefNetwork(784), Adam at its defaults,
    dynamically binarized MNIST, binary_cross_entropy_with_logits summed per image and averaged over the batch) on the MI355X
    path. Arguments as the reference; `debug_loader` replaces both loaders (any iterable of (x, y) batches). Returns the
    Trainer."""
    from pytorch_generative_amd import recipes

    return recipes.run(
        lambda: FullyVisibleBeliefNetwork(n_dims=784),
        loaders=recipes.binarized_mnist, loss_fn=recipes.bce_loss, lr=1e-3,
        n_epochs=n_epochs, batch_size=batch_size, log_dir=log_dir, n_gpus=n_gpus,
        device_id=device_id, debug_loader=debug_loader)
