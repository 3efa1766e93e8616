"""Generates tests/golden/nice/cases.pt from the REAL reference (run in the build container only):

    python tests/golden/make_nice_golden.py

NICE (models/flow/nice.py): per case the constructor kwargs, the initial state_dict and the input x; what forward returns
(z, log_det_J), the recipe's loss dict (the logistic prior of nice.py:205-213, restated here from its formula), all parameter gradients and the parameters after
one torch.optim.Adam(lr=1e-3) step; then `_inverse` of a recorded z0 under the initial state. `log_scale` and the biases are
perturbed off zero, so that their role is visible. The seed of a case is the first for which no hidden pre-activation of the
float64 restatement (tests/_nice_ref.py) lies within 1e-5 x its layer's largest of zero (asserted). All in float32 on the CPU.
The file lives in a subdirectory: `_util.golden_names()` feeds every top-level `tests/golden/*.pt` to the model tests.
"""

import os
import sys
import zlib

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import _nice_ref as nref  # noqa: E402
import _ref  # noqa: E402

# name: (n_features, n_coupling_blocks, n_hidden_layers, n_hidden_features, batch, image (h, w) or None)
CASES = {
    "f6_b3_l1_h5_n3": (6, 3, 1, 5, 3, None),
    "f16_b4_l2_h9_n4_img": (16, 4, 2, 9, 4, (4, 4)),
    "f70_b2_l3_h33_n5": (70, 2, 3, 33, 5, None),
}
MARGIN = 1e-5


def loss_fn(z, log_det_j):
    """The recipe's three figures from the formulas of tests/_nice_ref.py, in float32 autograd: the standard logistic
    log-density -(|z| + 2 log1p(exp(-|z|))) summed per sample, its batch mean, and minus (that mean + log det J)."""
    a = z.reshape(z.shape[0], -1).abs()
    prior = (-(a + 2 * torch.log1p(torch.exp(-a))).sum(dim=1)).mean()
    return {"loss": -(prior + log_det_j), "prior_log_likelihood": prior, "log_det_J": log_det_j}


def _make_case(ref, name, f, blocks, layers, hidden, n, hw, salt):
    torch.manual_seed(zlib.crc32(name.encode()) + salt)
    kwargs = dict(n_features=f, n_coupling_blocks=blocks, n_hidden_layers=layers, n_hidden_features=hidden)
    model = ref.models.NICE(**kwargs)
    with torch.no_grad():
        model.scaling.log_scale.normal_(0, 0.3)
        for k, p in model.named_parameters():
            if k.endswith(".bias"):
                p.add_(torch.randn_like(p) * 0.3)
    x = torch.rand((n, 1) + hw) if hw else torch.rand(n, f)
    z0 = torch.randn(x.shape)
    state0 = _ref.clone_state(model)
    if nref.relu_margin(x, state0) < MARGIN:
        return None
    with torch.no_grad():
        x_inv = model._inverse(z0).clone()
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    opt.zero_grad()
    z, log_det_j = model(x)
    losses = loss_fn(z, log_det_j)
    losses["loss"].backward()
    rec = {"kwargs": kwargs, "state": state0, "x": x, "z": z.detach().clone(), "log_det_J": log_det_j.detach().clone(),
           "losses": {k: v.detach().clone() for k, v in losses.items()},
           "grads": {k: p.grad.detach().clone() for k, p in model.named_parameters()}, "z0": z0, "inverse": x_inv, "seed_salt": salt}
    opt.step()
    rec["params_after_adam"] = {k: v.detach().clone() for k, v in model.named_parameters()}
    return rec


def make_case(ref, name, spec):
    for salt in range(100):
        rec = _make_case(ref, name, *spec, salt)
        if rec is not None:
            return rec
    raise RuntimeError(name)


def main():
    ref = _ref.load()
    out = {"cases": {name: make_case(ref, name, spec) for name, spec in CASES.items()}}
    path = os.path.join(HERE, "nice", "cases.pt")
    os.makedirs(os.path.dirname(path), exist_ok=True)
    torch.save(out, path)
    print(f"wrote {path} ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    main()
