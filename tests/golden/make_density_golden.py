"""Generates tests/golden/density/cases.pt from the REAL reference (run in the build container only):

    python tests/golden/make_density_golden.py

Mixture models (models/mixture_models.py): per case the constructor kwargs, the initial state_dict and the input x; then
for 3 torch.optim.Adam steps (default settings) on loss = -forward(x).mean(): the output, the loss, every parameter
gradient and the parameters after the step. The mixture steps run the reference IN FLOAT64 (`model.double()` on the
float32 initial state and inputs, which are what is stored): at its own initialisation every component is nearly the
same, the mixture_logits gradient is a difference of nearly equal sums, and the reference's float32 gradients miss the
project's gradient gate against its own float64 run (Gaussian, K = 7, (6, 3, 8, 8) inputs: element-wise ratio 1.87 for
`mean`, 1.41 for `mixture_logits`, 1.08 for `log_std`; K = 3: 1.44 for `mean`), so they cannot serve as the expected
values of that gate. KDE (models/kde.py): per case the train and test points and, per bandwidth,
the outputs of the Gaussian and the Parzen window kernel; the last test row lies far from every training point (no
Parzen window contains it: -inf). The points are re-drawn (seed salt) until no |test - train| / h lies within 1e-6 of
the window edge 0.5, so the Parzen counts do not depend on the last bit of a division. The KDE outputs are the reference's float32 ones, on the CPU. The
file lives in a subdirectory: `_util.golden_names()` feeds every top-level `tests/golden/*.pt` to the model tests.
"""

import os
import sys
import zlib

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import _ref  # noqa: E402

# name: (class, ctor kwargs, input shape, input kind)
MIXTURES = {}
for _k in (1, 3, 7):
    MIXTURES[f"gaussian_k{_k}_vec"] = ("GaussianMixtureModel", dict(n_components=_k, n_features=12), (9, 12), "randn")
    MIXTURES[f"gaussian_k{_k}_img"] = ("GaussianMixtureModel", dict(n_components=_k, n_features=192), (6, 3, 8, 8),
                                       "randn")
    MIXTURES[f"bernoulli_k{_k}_vec"] = ("BernoulliMixtureModel", dict(n_components=_k, n_features=12), (9, 12),
                                        "binary")
    MIXTURES[f"bernoulli_k{_k}_img"] = ("BernoulliMixtureModel", dict(n_components=_k, n_features=192), (6, 3, 8, 8),
                                        "binary")
MIXTURES["bernoulli_k3_real"] = ("BernoulliMixtureModel", dict(n_components=3, n_features=12), (9, 12), "uniform")
STEPS = 3

KDE_DIMS = (2, 3, 64)
BANDWIDTHS = (0.1, 0.5, 1.0)
N_TRAIN, N_TEST = 40, 11
EDGE_MARGIN = 1e-6


def make_mixture(ref, name, cls, kwargs, shape, kind):
    torch.manual_seed(zlib.crc32(name.encode()))
    model = getattr(ref.models, cls)(**kwargs)
    if kind == "randn":
        x = torch.randn(shape)
    elif kind == "binary":
        x = torch.bernoulli(torch.full(shape, 0.4))
    else:
        x = torch.rand(shape)
    state0 = _ref.clone_state(model)  # float32, as constructed
    model = model.double()
    x64 = x.double()
    opt = torch.optim.Adam(model.parameters())
    steps = []
    for _ in range(STEPS):
        opt.zero_grad()
        out = model(x64)
        loss = -out.mean()
        loss.backward()
        rec = {"out": out.detach().clone(), "loss": loss.detach().clone(),
               "grads": {k: p.grad.detach().clone() for k, p in model.named_parameters()}}
        opt.step()
        rec["params_after_adam"] = {k: p.detach().clone() for k, p in model.named_parameters()}
        steps.append(rec)
    return {"cls": cls, "kwargs": kwargs, "state": state0, "x": x, "steps": steps}


class _NearEdge(Exception):
    pass


def _make_kde(ref, d, salt):
    g = torch.Generator().manual_seed(1000 * d + salt)
    # training points in a box of a few bandwidths, so that windows of every bandwidth hold some test points
    train = torch.rand(N_TRAIN, d, generator=g) * 0.6
    test = train[torch.randint(0, N_TRAIN, (N_TEST,), generator=g)] + (torch.rand(N_TEST, d, generator=g) - 0.5) * 0.08
    test[-1] = 25.0  # far from everything: no window contains it
    rec = {"train": train, "test": test, "gaussian": {}, "parzen": {}}
    for h in BANDWIDTHS:
        ratio = (test[:, None, :] - train[None, :, :]).abs() / h
        if float((ratio - 0.5).abs().min()) <= EDGE_MARGIN:
            raise _NearEdge
        model = ref.models.KernelDensityEstimator(train, ref.models.GaussianKernel(bandwidth=h))
        rec["gaussian"][h] = model(test).clone()
        model = ref.models.KernelDensityEstimator(train, ref.models.ParzenWindowKernel(bandwidth=h))
        rec["parzen"][h] = model(test).clone()
    return rec


def make_kde(ref, d):
    for salt in range(100):
        try:
            return _make_kde(ref, d, salt)
        except _NearEdge:
            continue
    raise RuntimeError(f"kde d = {d}")


def main():
    ref = _ref.load()
    out = {"mixtures": {name: make_mixture(ref, name, *spec) for name, spec in MIXTURES.items()},
           "kde": {d: make_kde(ref, d) for d in KDE_DIMS}, "bandwidths": BANDWIDTHS}
    path = os.path.join(HERE, "density", "cases.pt")
    os.makedirs(os.path.dirname(path), exist_ok=True)
    torch.save(out, path)
    print(f"wrote {path} ({os.path.getsize(path)} bytes)")
    for d, rec in out["kde"].items():
        for h in BANDWIDTHS:
            print(d, h, "parzen", rec["parzen"][h].tolist()[:4], "...", rec["parzen"][h].tolist()[-1])


if __name__ == "__main__":
    main()
