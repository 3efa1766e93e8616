"""Generates tests/golden/gp/cases.pt from the REAL reference (run in the build container only):

    python tests/golden/make_gp_golden.py

GaussianProcess (models/gaussian_process.py) in float32 on the CPU. The reference ships no covariance or mean function outside
its notebook, so the two callables are this maker's own: k(a, b) = std^2 exp(-(cdist(a, b) / lengthscale)^2 / 2) and a
constant mean. Per case: the hyperparameters, the training data in two pieces, the query points, and (mu, sig) from
`predict` after the first `fit` and again after the second.

Every case keeps cond(K + noise_var I) <= 1e3, and the maker asserts that the reference's own float32 result lies within a
QUARTER of the tests' gate of the float64 closed form (tests/_gp_ref.py; gate: mu 1e-4 max |mu|, sig 1e-4 max |kernel(x, x)|);
a case that misses either is shrunk (n to three quarters) until it holds."""

import importlib
import os
import sys
import zlib

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import _gp_ref as gref  # noqa: E402
import _ref  # noqa: E402

# name: (n, m, d, p, noise_var, lengthscale, std, value, spread of the inputs)
CASES = {
    "n40_m17_d1": (40, 17, 1, 1, 0.1, 1.0, 1.0, 0.0, 4.0),
    "n130_m64_d20": (130, 64, 20, 1, 0.01, 3.0, 1.3, 0.5, 1.0),
    "n50_m9_d2_p3": (50, 9, 2, 3, 0.05, 1.5, 0.8, -0.25, 3.0),
}
GATE = 1e-4
MAX_COND = 1e3


def callables(std, lengthscale, value):
    def kernel(a, b):
        return std ** 2 * torch.exp(-0.5 * (torch.cdist(a, b) / lengthscale) ** 2)

    def mean(x):
        return torch.ones(x.shape[0], 1, dtype=x.dtype) * value

    return kernel, mean


def _try_case(ref, name, n, m, d, p, noise_var, lengthscale, std, value, spread):
    g = torch.Generator().manual_seed(zlib.crc32(name.encode()))
    scale = spread if d > 1 else 1.0
    train_x = (torch.rand(n, d, generator=g) * 2 - 1) * spread if d <= 2 else torch.randn(n, d, generator=g) * scale
    x = (torch.rand(m, d, generator=g) * 2 - 1) * spread if d <= 2 else torch.randn(m, d, generator=g) * scale
    truth = torch.sin(train_x.sum(1, keepdim=True) * torch.arange(1, p + 1)) + value
    train_y = truth + noise_var ** 0.5 * torch.randn(n, p, generator=g)
    n1 = max(1, (2 * n) // 3)
    kernel, mean = callables(std, lengthscale, value)
    gp = importlib.import_module(ref.__name__ + ".models.gaussian_process").GaussianProcess(mean, kernel, noise_var)
    noise = float(gp.noise_var)  # the float32 value the reference adds
    k64 = gref.se(train_x, train_x, std, lengthscale) + noise * torch.eye(n, dtype=torch.float64)
    cond = float(torch.linalg.cond(k64))
    rec = {"n": n, "n1": n1, "m": m, "d": d, "p": p, "noise_var": noise_var, "lengthscale": lengthscale, "std": std, "value": value,
           "train_x": train_x, "train_y": train_y, "x": x, "cond": cond}
    worst = 0.0
    for tag, lo, hi in (("", 0, n1), ("2", n1, n)):
        gp.fit(train_x[lo:hi], train_y[lo:hi])
        mu, sig = gp.predict(x)
        mu64, sig64 = gref.posterior(train_x[:hi], train_y[:hi], x, std, lengthscale, value, noise)
        e_mu = float((mu.double() - mu64).abs().max() / mu64.abs().max())
        e_sig = float((sig.double() - sig64).abs().max() / gref.se(x, x, std, lengthscale).abs().max())
        worst = max(worst, e_mu, e_sig)
        rec["mu" + tag], rec["sig" + tag] = mu.clone(), sig.clone()
        rec["ref_err" + tag] = (e_mu, e_sig)
    return rec, cond, worst


def make_case(ref, name, spec):
    n = spec[0]
    while n >= 4:
        rec, cond, worst = _try_case(ref, name, n, *spec[1:])
        if cond <= MAX_COND and worst <= GATE / 4:
            return rec
        print(f"  {name}: n = {n} has cond {cond:.3g}, reference fp32 error {worst:.2e}: shrinking")
        n = (3 * n) // 4
    raise RuntimeError(name)


def main():
    ref = _ref.load()
    out = {"cases": {name: make_case(ref, name, spec) for name, spec in CASES.items()}, "gate": GATE}
    path = os.path.join(HERE, "gp", "cases.pt")
    os.makedirs(os.path.dirname(path), exist_ok=True)
    torch.save(out, path)
    print(f"wrote {path} ({os.path.getsize(path)} bytes)")
    for name, case in out["cases"].items():
        print(f"  {name}: n = {case['n']}, cond {case['cond']:.4g}, reference fp32 errors {case['ref_err']} / {case['ref_err2']}")


if __name__ == "__main__":
    main()
