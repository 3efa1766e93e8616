"""Generates tests/golden/made/cases.pt from the REAL reference (run in the build container only):

    python tests/golden/make_made_golden.py

MADE (models/autoregressive/made.py): per case the constructor kwargs, the initial state_dict and the inputs; then for
3 consecutive forwards (so that n_masks > 1 rotates): the masks and the ordering the forward drew, the logits, the
BCE-with-logits loss (summed per image, averaged over the batch: the recipe's loss_fn), every (unmasked) weight
gradient, the weights after the in-place masking and the parameters after a torch.optim.Adam step; and one sample()
with the deterministic sample_fn (logits > 0) on a partly filled `conditioned_on`. All in float32 on the CPU. The file
lives in a subdirectory: `_util.golden_names()` feeds every top-level `tests/golden/*.pt` to the model tests.
"""

import os
import sys
import zlib

import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import _ref  # noqa: E402

# name: (ctor kwargs, batch, image (h, w) or None, binary inputs)
CASES = {
    "d12_h20_m1": (dict(input_dim=12, hidden_dims=[20], n_masks=1), 5, None, True),
    "d16_h20_9_13_m3": (dict(input_dim=16, hidden_dims=[20, 9, 13], n_masks=3), 4, (4, 4), True),
    "d12_none_m1": (dict(input_dim=12, hidden_dims=None, n_masks=1), 3, None, False),
    "d16_h20_m3_real": (dict(input_dim=16, hidden_dims=[20], n_masks=3), 6, (4, 4), False),
}
STEPS = 3


def loss_fn(x, preds):
    n = x.shape[0]
    return F.binary_cross_entropy_with_logits(preds.view(n, -1), x.view(n, -1), reduction="none").sum(dim=1).mean()


def clone_params(model):
    return {k: v.detach().clone() for k, v in model.named_parameters()}


def make_case(ref, name, kwargs, n, hw, binary):
    """The first seed salt whose sampled logits all keep 1e-3 away from the threshold."""
    for salt in range(100):
        try:
            return _make_case(ref, name, kwargs, n, hw, binary, salt)
        except _NearThreshold:
            continue
    raise RuntimeError(name)


class _NearThreshold(Exception):
    pass


def _make_case(ref, name, kwargs, n, hw, binary, salt):
    torch.manual_seed(zlib.crc32(name.encode()) + salt)
    model = ref.models.MADE(sample_fn=lambda l: (l > 0).float(), **kwargs)
    d = kwargs["input_dim"]
    shape = (n, 1) + hw if hw else (n, d)
    x = torch.bernoulli(torch.full(shape, 0.4)) if binary else torch.randn(shape)
    state0 = _ref.clone_state(model)
    opt = torch.optim.Adam(model.parameters())
    steps = []
    for _ in range(STEPS):
        seed_before = model._mask_seed
        opt.zero_grad()
        logits = model(x)
        loss = loss_fn(x, logits)
        loss.backward()
        # the masks / ordering this forward used: redraw them from the seed it saw
        saved = model._mask_seed
        model._mask_seed = seed_before
        masks, ordering = model._sample_masks()
        model._mask_seed = saved
        layers = [m for m in model._net if isinstance(m, ref.models.autoregressive.made.MaskedLinear)]
        for layer, m in zip(layers, masks):
            assert torch.equal(layer.mask, m.float())
        rec = {
            "masks": [m.clone() for m in masks], "ordering": torch.from_numpy(ordering.copy()),
            "logits": logits.detach().clone(), "loss": loss.detach().clone(),
            "grads": {k: p.grad.detach().clone() for k, p in model.named_parameters()},
            "masked_weights": {k: p.detach().clone() for k, p in model.named_parameters() if k.endswith("weight")},
        }
        opt.step()
        rec["params_after_adam"] = clone_params(model)
        steps.append(rec)

    # sample(): partly filled conditioned_on (entries >= 0 kept), one mask draw, deterministic sample_fn
    seed_before = model._mask_seed
    cond = torch.full(shape, -1.0)
    flat = cond.view(shape[0], -1)
    g = torch.Generator().manual_seed(7)
    keep = torch.rand(flat.shape, generator=g) < 0.3
    flat[keep] = torch.bernoulli(torch.full(flat.shape, 0.5), generator=g)[keep]
    with torch.no_grad():
        state_sample = _ref.clone_state(model)
        # the logits the sampler thresholds must not sit on the threshold
        masks, ordering = model._sample_masks()
        model._mask_seed = seed_before
        canvas = cond.clone().view(shape[0], -1)
        for dim in ordering.argsort():
            out = model._forward(canvas, masks)[:, dim]
            if float(out.abs().min()) <= 1e-3:
                raise _NearThreshold
            canvas[:, dim] = torch.where(canvas[:, dim] < 0, (out > 0).float(), canvas[:, dim])
        model._mask_seed = seed_before
        model.load_state_dict(state_sample)
        sample = model.sample(None, conditioned_on=cond)
    assert torch.equal(sample.view(shape[0], -1), canvas)
    return {"kwargs": kwargs, "state": state0, "x": x, "steps": steps, "sample_state": state_sample,
            "sample_mask_seed": seed_before, "conditioned_on": cond, "sample": sample.clone()}


def main():
    ref = _ref.load()
    out = {"cases": {name: make_case(ref, name, *spec) for name, spec in CASES.items()}}
    # the recipe's size: masks / ordering only (for the bit-equality of the degree generation), seeds 0..2
    big = {}
    for n_masks in (1, 3):
        model = ref.models.MADE(784, [8000], n_masks=n_masks)
        for step in range(3):
            masks, ordering = model._sample_masks()
            big[(n_masks, step)] = {"ordering": torch.from_numpy(ordering.copy()),
                                    "mask_sums": [int(m.sum()) for m in masks],
                                    "mask_row_sums": [m.sum(1, dtype=torch.int32) for m in masks]}
    out["recipe_masks"] = big
    path = os.path.join(HERE, "made", "cases.pt")
    os.makedirs(os.path.dirname(path), exist_ok=True)
    torch.save(out, path)
    print(f"wrote {path} ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    main()
