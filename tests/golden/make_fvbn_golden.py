"""Generates tests/golden/fvbn/cases.pt from the REAL reference (run in the build container only):

    python tests/golden/make_fvbn_golden.py

FullyVisibleBeliefNetwork (models/autoregressive/fvbn.py): per case the constructor kwargs, the initial state_dict and the
input x; the logits forward returns, the recipe's loss (binary_cross_entropy_with_logits summed over everything and divided by
the batch), every `_net.i.*` gradient and the parameters after one torch.optim.Adam step; then one sample(conditioned_on=...)
on a partly filled IMAGE canvas (the reference's sample() takes images only). The model is built with
`sample_fn = lambda l: (l > 0).float()`, which makes the pass deterministic; the seed of a case is the first one for which no
logit consulted in that pass lies within MARGIN = 4e-3 of 0 (asserted, and stored as `sample_margin`). All in float32 on the
CPU. The file lives in a subdirectory: `_util.golden_names()` feeds every top-level `tests/golden/*.pt` to the model tests.
"""

import os
import sys
import zlib

import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import _ref  # noqa: E402

# name: (n_dims, batch, shape of x behind the batch, shape of the sampling canvas behind the batch, binary inputs)
CASES = {
    "d12_n5": (12, 5, (12,), (1, 3, 4), True),
    "d16_n4_img": (16, 4, (1, 4, 4), (1, 4, 4), True),
    "d1_n3": (1, 3, (1,), (1, 1, 1), True),
    "d5_n4_real": (5, 4, (5,), (1, 1, 5), False),
}
MARGIN = 4e-3


def loss_fn(x, preds):
    return F.binary_cross_entropy_with_logits(preds, x, reduction="none").sum() / x.shape[0]


class _NearThreshold(Exception):
    pass


def _make_case(ref, name, d, n, x_shape, canvas_shape, binary, salt):
    torch.manual_seed(zlib.crc32(name.encode()) + salt)
    seen = []

    def threshold(logits):
        seen.append(logits.detach().clone().reshape(-1))
        return (logits > 0).float()

    model = ref.models.FullyVisibleBeliefNetwork(n_dims=d, sample_fn=threshold)
    shape = (n,) + x_shape
    x = torch.bernoulli(torch.full(shape, 0.4)) if binary else torch.rand(shape)
    opt = torch.optim.Adam(model.parameters())
    opt.zero_grad()
    logits = model(x)  # an image batch registers _c / _h / _w: they are part of the state from here on
    state0 = _ref.clone_state(model)
    loss = loss_fn(x, logits)
    loss.backward()
    rec = {"kwargs": dict(n_dims=d), "state": state0, "x": x, "logits": logits.detach().clone(), "loss": loss.detach().clone(),
           "grads": {k: p.grad.detach().clone() for k, p in model.named_parameters()}}
    opt.step()
    rec["params_after_adam"] = {k: v.detach().clone() for k, v in model.named_parameters()}

    cond = torch.full((n,) + canvas_shape, -1.0)
    flat = cond.view(n, -1)
    g = torch.Generator().manual_seed(7)
    keep = torch.rand(flat.shape, generator=g) < 0.3
    flat[keep] = torch.bernoulli(torch.full(flat.shape, 0.5), generator=g)[keep]
    before = cond.clone()
    sample = model.sample(None, conditioned_on=cond)
    consulted = torch.cat(seen)
    assert consulted.numel() == n * d
    margin = float(consulted.abs().min())
    if margin <= MARGIN:
        raise _NearThreshold
    assert torch.equal(cond, before), "the reference modified conditioned_on"
    assert sample.shape == cond.shape and bool(((sample == 0) | (sample == 1)).all())
    assert torch.equal(sample[before >= 0], before[before >= 0])
    rec.update({"sample_state": _ref.clone_state(model), "conditioned_on": before, "sample": sample.clone(), "sample_margin": margin})
    return rec


def make_case(ref, name, spec):
    for salt in range(100):
        try:
            return _make_case(ref, name, *spec, salt)
        except _NearThreshold:
            continue
    raise RuntimeError(name)


def main():
    ref = _ref.load()
    out = {"cases": {name: make_case(ref, name, spec) for name, spec in CASES.items()}, "margin": MARGIN}
    path = os.path.join(HERE, "fvbn", "cases.pt")
    os.makedirs(os.path.dirname(path), exist_ok=True)
    torch.save(out, path)
    print(f"wrote {path} ({os.path.getsize(path)} bytes)")
    for name, case in out["cases"].items():
        print(f"  {name}: sample margin {case['sample_margin']:.3e}, keys {list(case['state'])[:4]} ...")


if __name__ == "__main__":
    main()
