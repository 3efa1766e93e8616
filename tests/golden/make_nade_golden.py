"""Generates tests/golden/nade/cases.pt from the REAL reference (run in the build container only):

    python tests/golden/make_nade_golden.py

NADE (models/autoregressive/nade.py): per case the constructor kwargs, the initial state_dict and the input x; the
probabilities forward returns, the recipe's loss (binary_cross_entropy_with_logits applied to those probabilities, summed per
sample and averaged over the batch), all four gradients and the parameters after one torch.optim.Adam step; then one sample()
on a partly filled `conditioned_on`, made deterministic by replacing the reference's Bernoulli draw with `p > 0.5`. The seed
of a case is the first one for which no probability of that sampling pass lies within 1e-3 of 0.5 (asserted). The inputs are
non-negative: the reference's forward redraws negative entries. All in float32 on the CPU. The file lives in a subdirectory:
`_util.golden_names()` feeds every top-level `tests/golden/*.pt` to the model tests.
"""

import os
import sys
import zlib

import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import _ref  # noqa: E402

# name: (input_dim, hidden_dim, batch, image (h, w) or None, binary inputs)
CASES = {
    "d12_h20_n5": (12, 20, 5, None, True),
    "d16_h9_n4_img": (16, 9, 4, (4, 4), True),
    "d7_h1_n3": (7, 1, 3, None, True),
    "d10_h6_n4_real": (10, 6, 4, None, False),
}
MARGIN = 1e-3


def loss_fn(x, preds):
    n = x.shape[0]
    return F.binary_cross_entropy_with_logits(preds.view(n, -1), x.view(n, -1), reduction="none").sum(dim=1).mean()


class _NearThreshold(Exception):
    pass


class _Threshold:
    """Stands in for torch.distributions inside the reference's nade module: Bernoulli(probs=p).sample() -> p > 0.5."""

    seen = []

    class Bernoulli:
        def __init__(self, probs):
            self.probs = probs

        def sample(self):
            _Threshold.seen.append(self.probs.detach().clone())
            return (self.probs > 0.5).float()


def _make_case(ref, name, d, h, n, hw, binary, salt):
    torch.manual_seed(zlib.crc32(name.encode()) + salt)
    model = ref.models.NADE(input_dim=d, hidden_dim=h)
    with torch.no_grad():  # biases off zero, so that their role is visible
        model._in_b.normal_(0, 0.3)
        model._h_b.normal_(0, 0.3)
    shape = (n, 1) + hw if hw else (n, d)
    x = torch.bernoulli(torch.full(shape, 0.4)) if binary else torch.rand(shape)
    state0 = _ref.clone_state(model)
    opt = torch.optim.Adam(model.parameters())
    opt.zero_grad()
    probs = model(x)
    loss = loss_fn(x, probs)
    loss.backward()
    rec = {"kwargs": dict(input_dim=d, hidden_dim=h), "state": state0, "x": x, "probs": probs.detach().clone(),
           "loss": loss.detach().clone(), "grads": {k: p.grad.detach().clone() for k, p in model.named_parameters()}}
    opt.step()
    rec["params_after_adam"] = {k: v.detach().clone() for k, v in model.named_parameters()}

    cond = torch.full(shape, -1.0)
    flat = cond.view(n, -1)
    g = torch.Generator().manual_seed(7)
    keep = torch.rand(flat.shape, generator=g) < 0.3
    flat[keep] = torch.bernoulli(torch.full(flat.shape, 0.5), generator=g)[keep]
    before = cond.clone()
    mod = ref.models.autoregressive.nade
    saved, mod.distributions = mod.distributions, _Threshold
    _Threshold.seen = []
    try:
        sample = model.sample(None, conditioned_on=cond)
    finally:
        mod.distributions = saved
    p_all = torch.cat(_Threshold.seen, dim=1)
    if float((p_all - 0.5).abs().min()) <= MARGIN:
        raise _NearThreshold
    assert torch.equal(cond, before), "the reference modified conditioned_on"
    assert sample.shape == cond.shape and bool(((sample == 0) | (sample == 1)).all())
    assert torch.equal(sample[before >= 0], before[before >= 0])
    rec.update({"sample_state": {k: v.detach().clone() for k, v in model.state_dict().items() if k.startswith(("_in", "_h_"))},
                "conditioned_on": before, "sample": sample.clone(), "sample_margin": float((p_all - 0.5).abs().min())})
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
    out = {"cases": {name: make_case(ref, name, spec) for name, spec in CASES.items()}}
    path = os.path.join(HERE, "nade", "cases.pt")
    os.makedirs(os.path.dirname(path), exist_ok=True)
    torch.save(out, path)
    print(f"wrote {path} ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    main()
