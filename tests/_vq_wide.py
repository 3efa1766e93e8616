"""Shared by the VectorQuantizer tests: the fixtures of tests/golden/vq_wide/ (make_vq_wide_golden.py) and the float64
distances / tie margin they were generated under."""

import os

import torch

import _util

DIR = os.path.join(_util.GOLDEN_DIR, "vq_wide")
TIE_MARGIN = 1e-4  # relative to |x|^2 + max |e|^2: about 100 times the fp32 round-off of a 200-term distance


def _load(name):
    return torch.load(os.path.join(DIR, name + ".pt"), map_location="cpu", weights_only=False)


def case_names():
    index = _load("cases")
    assert index["tie_margin"] == TIE_MARGIN
    return list(index["cases"])


def load_case(name):
    """The case's record with the EMA mode's buffers under "ema" ({"before": ..., "after": ...})."""
    case = _load(name)
    case["ema"] = _load(name + "_ema")
    return case


def load_model():
    return _load("vq_vae_wide")


def distances64(x, emb):
    """Float64 distances (P, K) of the NCHW input's positions to the codes, in the reference's expanded form, and the
    scale |x|^2 + max |e|^2 (P,) the tie margin is relative to."""
    f, e = x.permute(0, 2, 3, 1).reshape(-1, x.shape[1]).double(), emb.double()
    x2, e2 = (f * f).sum(1), (e * e).sum(1)
    return x2[:, None] + e2 - 2 * f @ e.t(), x2 + e2.max()


def tie_gap(x, emb, skip=1):
    """min over positions of ((skip + 1)-th smallest distance - smallest) / scale; +inf with too few codes."""
    dist, scale = distances64(x, emb)
    if dist.shape[1] <= skip:
        return float("inf")
    srt = dist.sort(dim=1).values
    return float(((srt[:, skip] - srt[:, 0]) / scale).min())


def ragged_problem():
    """P = 1100 positions, D = 130, K = 300: a kaiming-uniform codebook (the module's initialisation) and normal inputs.
    With 300 codes and 1100 positions some pairs of distances are closer than any margin: the op-parity test accepts
    near-ties by their float64 distance instead."""
    g = torch.Generator().manual_seed(2024)
    bound = (3.0 / 130) ** 0.5  # init.kaiming_uniform_(nonlinearity="linear") on (K, 130)
    emb = (torch.rand(300, 130, generator=g) * 2 - 1) * bound
    x = torch.randn(11, 130, 10, 10, generator=g)
    return x, emb
