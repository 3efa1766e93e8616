"""Generates tests/golden/linear_attention/cases.pt from the REAL reference (run in the build container only):

    python tests/golden/make_linear_attention_golden.py

`LinearCausalAttention` (nn/attention.py:168-275): per case the module's state_dict, the input x, an upstream gradient g,
the output y = module(x) and the gradients of sum(y * g) with respect to x and every parameter, all from the reference's
own forward and hand-written backward (`_UnnormalizedLinearCausalAttention`) in float32. The file lives in a
subdirectory: `_util.golden_names()` feeds every top-level `tests/golden/*.pt` to the model tests.
"""

import os
import sys

import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import _ref  # noqa: E402

FEATURES = {"default": None, "softplus": F.softplus}

# name: (N, C, H, W, ctor kwargs, feature)
CASES = {
    "h1_c8_7x9": (2, 8, 7, 9, dict(n_heads=1), "default"),
    "h2_e8_o12_7x9": (2, 16, 7, 9, dict(n_heads=2, embed_channels=8, out_channels=12), "default"),
    "h4_c16_32x32": (2, 16, 32, 32, dict(n_heads=4), "default"),
    "h4_dk1_dv3_7x9": (2, 8, 7, 9, dict(n_heads=4, embed_channels=4, out_channels=12), "default"),
    "h2_dk3_dv1_7x9": (3, 8, 7, 9, dict(n_heads=2, embed_channels=6, out_channels=2), "default"),
    "h1_dk64_dv64_10x13": (2, 16, 10, 13, dict(n_heads=1, embed_channels=64, out_channels=64), "default"),
    "h2_dk64_dv3_32x32": (1, 8, 32, 32, dict(n_heads=2, embed_channels=128, out_channels=6), "default"),
    "h2_L1": (3, 8, 1, 1, dict(n_heads=2), "default"),
    "h1_L1_dk1": (2, 4, 1, 1, dict(n_heads=1, embed_channels=1, out_channels=1), "default"),
    "h2_softplus_9x7": (2, 8, 9, 7, dict(n_heads=2), "softplus"),
}


def main():
    ref = _ref.load()
    out = {"torch_version": torch.__version__, "cases": {}}
    for i, (name, (n, c, h, w, kwargs, feature)) in enumerate(CASES.items()):
        torch.manual_seed(100 + i)
        extra = {} if FEATURES[feature] is None else {"feature_fn": FEATURES[feature]}
        mod = ref.nn.LinearCausalAttention(c, **kwargs, **extra)
        x = torch.randn(n, c, h, w, requires_grad=True)
        y = mod(x)
        g = torch.randn_like(y)
        (y * g).sum().backward()
        out["cases"][name] = {
            "kwargs": dict(in_channels=c, **kwargs),
            "feature": feature,
            "state": _ref.clone_state(mod),
            "x": x.detach().clone(),
            "g": g,
            "y": y.detach().clone(),
            "grads": {"x": x.grad.clone(), **{k: p.grad.clone() for k, p in mod.named_parameters()}},
        }
    os.makedirs(os.path.join(HERE, "linear_attention"), exist_ok=True)
    path = os.path.join(HERE, "linear_attention", "cases.pt")
    torch.save(out, path)
    print(f"wrote {path}: {len(CASES)} cases, torch {out['torch_version']}")


if __name__ == "__main__":
    main()
