"""Model base classes (behavioural mirror of the reference's models/base.py:28-120).

* GenerativeModel remembers the (C, H, W) of the first 4-D batch it is called with in lazily
  registered `_c/_h/_w` buffers (they are part of the state_dict, base.py:41-61).
* AutoregressiveModel.sample() fills pixels in raster order, one full forward per pixel,
  replacing only entries < 0 of `conditioned_on` (base.py:97-120).
"""

import abc
import functools

import torch
from torch import distributions, nn


def auto_reshape(fn):
    """Flattens (N, ...) inputs to (N, -1) for `fn` and gives its result the input's shape back (reference
    models/base.py:13-25): non-convolutional models (MADE) then take (N, 1, H, W) images as they are."""

    @functools.wraps(fn)
    def wrapped_fn(self, x, *args, **kwargs):
        original_shape = x.shape
        x = x.view(original_shape[0], -1)
        y = fn(self, x, *args, **kwargs)
        return y.view(original_shape)

    return wrapped_fn


def dense_head(fn):
    """Decorator of sample(): it always sees dense logits, so `defer_head` is off for the duration of the call."""

    @functools.wraps(fn)
    def wrapped_fn(self, *args, **kwargs):
        saved = self.defer_head
        self.defer_head = False
        try:
            return fn(self, *args, **kwargs)
        finally:
            self.defer_head = saved

    return wrapped_fn


def _bernoulli_from_logits(logits):
    return distributions.Bernoulli(logits=logits).sample()


class GenerativeModel(abc.ABC, nn.Module):
    def __call__(self, x, *args, **kwargs):
        if getattr(self, "_c", None) is None and x.dim() == 4:
            self._register_shape(*x.shape[1:])
        return super().__call__(x, *args, **kwargs)

    def _register_shape(self, c, h, w):
        for name, value in (("_c", c), ("_h", h), ("_w", w)):
            self.register_buffer(name, value if torch.is_tensor(value) else torch.tensor(value))

    def load_state_dict(self, state_dict, strict=True):
        if "_c" in state_dict and not getattr(self, "_c", None):
            self._register_shape(state_dict["_c"], state_dict["_h"], state_dict["_w"])
        return super().load_state_dict(state_dict, strict)

    @property
    def device(self):
        return next(self.parameters()).device

    @abc.abstractmethod
    def sample(self, n_samples):
        ...


class AutoregressiveModel(GenerativeModel):
    def __init__(self, sample_fn=None):
        """sample_fn: fn(logits) -> sample; defaults to Bernoulli(logits)."""
        super().__init__()
        self._sample_fn = sample_fn or _bernoulli_from_logits

    def _start_canvas(self, n_samples, conditioned_on):
        assert (
            n_samples is not None or conditioned_on is not None
        ), 'Must provided one, and only one, of "n_samples" or "conditioned_on"'
        if conditioned_on is not None:
            return conditioned_on.clone()
        # a code image has one channel, whatever channel count a checkpoint trained on one-hot input recorded
        shape = (n_samples, 1 if self.input_codes is not None else int(self._c), int(self._h), int(self._w))
        return torch.full(shape, -1.0, device=self.device)

    # Models whose every layer is row-causal set this: sample() then evaluates one image ROW per step
    # against per-layer caches of the rows above (ops.RowDecode) instead of the whole image.
    _row_decode = False
    _row_graph = False            # the row step is identical for every row (attention: row index from the device): hipGraph it
    _row_decode_min_batch = 1     # below this batch the per-pixel full forward is used (launch-bound row steps)

    # True (extension; an attribute, not a constructor argument: signatures and state_dict stay the reference's): the models
    # with a K-way softmax head return ops.DeferredLogits from forward() instead of running their last 1x1 convolution, and
    # ops.categorical_nll_* run it inside the loss kernels (ops.linear_categorical): the (N, K C, H, W) logits are never written.
    defer_head = False

    # K (extension; an attribute like defer_head): forward() takes a code image (N, 1, H, W) at the levels j / (K - 1) — the
    # target layout of ops.categorical_nll_* and what nn.CategoricalSampler returns — in place of the (N, K, H, W) one-hot
    # tensor, and the stem runs as a table lookup (Conv2d.forward_codes). Parameters, state_dict and results are those of the
    # model on one_hot(codes); a negative level is an undrawn position. ImageGPT and PixelCNN take it; the others raise.
    input_codes = None

    def _no_input_codes(self):
        if self.input_codes is not None:
            raise ValueError(f"{type(self).__name__} does not support input_codes (ImageGPT and PixelCNN do)")

    # A condition module (extension; nn.CodeUpsample): forward(x, cond=...) and sample(cond=...) take a second, coarser code
    # image as context. It is the submodule `_cond`, so state_dict gains `_cond.weight` — only then: a model that never calls
    # set_condition keeps the reference's keys, signatures and bits. ImageGPT with `input_codes` takes it; the others raise.
    _accepts_condition = False

    def set_condition(self, module):
        """Registers `module` as the condition module `_cond` (before the optimizer is built: its weight is a parameter);
        None removes it."""
        if module is None:
            if "_cond" in self._modules:
                del self._modules["_cond"]
            return
        if not self._accepts_condition:
            raise ValueError(f"{type(self).__name__} does not support a condition module (ImageGPT with input_codes does)")
        if self.input_codes is None:
            raise ValueError(f"{type(self).__name__}: a condition module needs input_codes (set it first)")
        self.add_module("_cond", module)

    def _logits(self, features, conv, *, in_act=None, pre_ln=None, **dense_kw):
        """The model's last 1x1 convolution: deferred when `defer_head` is set and no RowDecode is open, else as always."""
        from pytorch_generative_amd import ops

        if self.defer_head and ops.RowDecode.current is None:
            return ops.DeferredLogits(features, conv, in_act=in_act, pre_ln=pre_ln)
        if pre_ln is not None:
            if ops.gpt_out_head_supported(features, pre_ln, conv):
                return conv(features, pre_ln=pre_ln, **dense_kw)
            return conv(pre_ln(features))
        return conv(features, in_act=in_act)

    def _draw_into(self, canvas, row, col, logits):
        """One pixel of every image: what was given (>= 0) is kept, the rest drawn by `_sample_fn` from the (N, C) logits."""
        n, c = canvas.shape[:2]
        drawn = self._sample_fn(logits).view(n, c)
        current = canvas[:, :, row, col]
        canvas[:, :, row, col] = torch.where(current < 0, drawn, current)

    def _capture_row_steps(self, ctx, step, class_rows, warm_step=None):
        """The row graphs of a row-cached sampler: step() is the row step under `ctx` (an open ops.RowDecode) and class_rows
        {class: a row of that class, None = the step is the same for every row and ctx.row stays as it is}. Per class the
        step is captured ONCE into two hipGraphs, evaluate and evaluate-and-commit — the eager row step is ~100 tiny launches,
        launch bound. All warm-up passes (warm_step, default step: evaluate, then commit, per class; they allocate every
        cache) run first on a side stream, then the captures; then the caches are cleared of what those passes pushed.
        Returns {class: (step graph, commit graph, step's static result)}, or None with the caches dropped when `_row_graph`
        is off or the capture was refused (`_row_step_captured` tells which: the fallback is silent)."""
        from pytorch_generative_amd import graph, ops

        def passes(fn):
            for row in class_rows.values():
                for commit in (False, True):
                    if row is not None:
                        ctx.row = row
                    ctx.commit = commit
                    yield fn

        pairs = None
        if self._row_graph:
            pairs = graph.try_capture(passes(step), lambda: [fn() for fn in passes(warm_step or step)])
            if pairs is None:
                ops.RowDecode.drop_caches(self)
        self._row_step_captured = pairs is not None
        if pairs is None:
            return None
        ops.RowDecode.clear_caches(self)
        return {cls: (pairs[2 * i][0], pairs[2 * i + 1][0], pairs[2 * i][1]) for i, cls in enumerate(class_rows)}

    @dense_head
    @torch.no_grad()
    def sample(self, n_samples=None, conditioned_on=None, *, incremental=True, return_logits=False):
        """Generates samples; entries of `conditioned_on` that are >= 0 are kept as given
        (reference models/base.py:97-120: raster order, `_sample_fn` once per pixel).

        incremental (extension): the reference runs a full forward per pixel; row-causal models here
        run the forward on the CURRENT ROW only, every convolution reading the few rows above it from
        a private cache and attention its cached keys / values (same logits, ~H x less arithmetic).
        return_logits (extension): also returns the (N, C, H, W) logits the draws were made from."""
        canvas = self._start_canvas(n_samples, conditioned_on)
        n, c, h, w = canvas.shape
        logits_map = torch.zeros_like(canvas) if return_logits else None
        if incremental and self._row_decode and (n >= self._row_decode_min_batch or return_logits):
            from pytorch_generative_amd import ops

            ops.RowDecode.drop_caches(self)
            row_in = torch.empty((n, c, 1, w), device=canvas.device, dtype=canvas.dtype)
            with ops.RowDecode(h) as ctx:
                # Row-invariant models (no attention, or attention that takes the row index from ctx.row_dev): the row step
                # touches the same buffers for every row, so one pair of graphs is replayed H*W + H times
                if self._row_graph:
                    row_in.fill_(0.0)
                graphs = self._capture_row_steps(ctx, lambda: self.forward(row_in), {0: None})
                step_graph, commit_graph, step_out = graphs[0] if graphs else (None, None, None)
                for row in range(h):
                    ctx.row, ctx.commit = row, False
                    for col in range(w):
                        row_in.copy_(canvas[:, :, row:row + 1, :])
                        if step_graph is not None:
                            step_graph.replay()
                            logits = step_out[:, :, 0, col]
                        else:
                            logits = self.forward(row_in)[:, :, 0, col]
                        if return_logits:
                            logits_map[:, :, row, col] = logits
                        self._draw_into(canvas, row, col, logits)
                    ctx.commit = True  # the row is final: push it into every layer's cache
                    row_in.copy_(canvas[:, :, row:row + 1, :])
                    if commit_graph is not None:
                        commit_graph.replay()
                    else:
                        self.forward(row_in)
            ops.RowDecode.drop_caches(self)
            return (canvas, logits_map) if return_logits else canvas
        for row in range(h):
            for col in range(w):
                logits = self.forward(canvas)[:, :, row, col]
                if return_logits:
                    logits_map[:, :, row, col] = logits
                self._draw_into(canvas, row, col, logits)
        return (canvas, logits_map) if return_logits else canvas
