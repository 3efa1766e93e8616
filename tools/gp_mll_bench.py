"""The log marginal likelihood of the Gaussian process and its hyperparameter gradients on the MI355X.

usage: python tools/gp_mll_bench.py [--out profiles/gp_mll.json] [--rounds 5] [--max-seconds 480]

* `evidence`: at n = 1024, 4096, 8192 and d = 1, 64 (p = 1), every call after reset_cache() so that the covariance, the
  factorisation, both solves of alpha and the read of info are inside:
    `factor_ms`        the factorisation alone (GaussianProcess._ensure_factor), the baseline everything else sits on;
    `value_ms`         log_marginal_likelihood() under no_grad;
    `value_grads_ms`   log_marginal_likelihood() with all four hyperparameters requiring grad, and backward();
  the three phases of the gradients on the cached factor, `inverse_ms` (ops.tri_inverse_t), `gram_ms` (ops.gram_upper_) and
  `sums_ms` (ops.se_mll_sums), each alone; and FOR COMPARISON ONLY, in eager torch-ROCm fp32 on the same GPU,
  `torch_value_ms` and `torch_value_grads_ms` (torch.cdist, torch.linalg.cholesky, cholesky_solve, autograd). Nothing in the
  library routes around its own kernels, so a figure that loses is written down as it is. `grads_vs_factor` is
  value_grads_ms / factor_ms — the flop ratio is 3 — and `slowest_phase` names the phase that takes the most time.
  `err_vs_float64` (n <= 4096): the relative errors of the value and the gradients of both candidates against float64 autograd
  on the same GPU.
* `optimize`: one optimize_hyperparameters(50, 0.05) call at n = 1024, d = 1, host clock, beside the same Adam loop in eager
  torch fp32.
Protocol: the candidates alternate in one process, `--rounds` rounds of timed calls between HIP events after a warm-up; the
figure is the median over the rounds of the per-call mean. The file is rewritten after every row; once `--max-seconds` of wall
clock have passed no further row is started and the file says which were left out."""

import argparse
import json
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pytorch-generative_amd"))
import torch  # noqa: E402
from torch import nn  # noqa: E402

NOISE = 0.1
SHAPES = ((1024, 1, 5), (1024, 64, 5), (4096, 1, 3), (4096, 64, 3), (8192, 1, 2), (8192, 64, 2))  # (n, d, calls per round)
NAMES = ("std", "lengthscale", "noise_var", "value")


def data(n, d, dev):
    """The training points of tools/gp_bench.py: about 20 points per lengthscale on a line, random directions in higher
    dimensions with the lengthscale at sqrt(d)."""
    g = torch.Generator().manual_seed(n + d)
    if d == 1:
        tx, lengthscale = torch.rand(n, 1, generator=g) * n / 20, 1.0
    else:
        tx, lengthscale = torch.randn(n, d, generator=g), float(d) ** 0.5
    ty = torch.sin(tx.sum(1, keepdim=True)) + NOISE ** 0.5 * torch.randn(n, 1, generator=g)
    return tx.to(dev), ty.to(dev), lengthscale


def time_round(fn, iters):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters


def alternate(fns, iters, rounds):
    """{name: median over the rounds of the mean ms per call}, the candidates taking turns inside every round."""
    for fn in fns.values():
        fn()
    torch.cuda.synchronize()
    ts = {name: [] for name in fns}
    for _ in range(rounds):
        for name, fn in fns.items():
            ts[name].append(time_round(fn, iters))
    return {name: statistics.median(v) for name, v in ts.items()}, {name: [min(v), max(v)] for name, v in ts.items()}


def torch_evidence(tx, ty, std, lengthscale, noise, value):
    """log p(y) in eager torch on the device, in the dtype of tx."""
    n = tx.shape[0]
    k = std ** 2 * torch.exp(-0.5 * (torch.cdist(tx, tx) / lengthscale) ** 2) + noise * torch.eye(n, device=tx.device, dtype=tx.dtype)
    chol = torch.linalg.cholesky(k)
    r = ty - value
    alpha = torch.cholesky_solve(r, chol)
    return -0.5 * (r * alpha).sum() - torch.log(torch.diagonal(chol)).sum() - 0.5 * n * math.log(2.0 * math.pi)


def leaves(values, dev, dtype):
    return [torch.tensor(v, device=dev, dtype=dtype, requires_grad=True) for v in values]


def make_model(lengthscale, dev, std=1.0, noise=NOISE, value=0.0):
    from pytorch_generative_amd.models import gaussian_process as gp

    model = gp.GaussianProcess(gp.Const(nn.Parameter(torch.tensor(value))),
                               gp.SquaredExponential(nn.Parameter(torch.tensor(std)), nn.Parameter(torch.tensor(float(lengthscale)))), noise).to(dev)
    model.noise_var.requires_grad_()
    return model


def model_grads(model):
    tensors = (model.kernel.std, model.kernel.lengthscale, model.noise_var, model.mean.value)
    for t in tensors:
        t.grad = None
    value = model.log_marginal_likelihood()
    value.backward()
    return value.detach(), [t.grad for t in tensors]


def evidence_row(n, d, iters, dev, rounds):
    from pytorch_generative_amd import ops

    tx, ty, lengthscale = data(n, d, dev)
    model = make_model(lengthscale, dev)
    model.fit(tx, ty)
    hyper = (1.0, lengthscale, NOISE, 0.0)

    def factor():
        model.reset_cache()
        model._ensure_factor()

    def value():
        model.reset_cache()
        with torch.no_grad():
            model.log_marginal_likelihood()

    def value_grads():
        model.reset_cache()
        model_grads(model)

    def torch_value():
        with torch.no_grad():
            torch_evidence(tx, ty, *hyper)

    def torch_value_grads():
        torch_evidence(tx, ty, *leaves(hyper, dev, torch.float32)).backward()

    model._ensure_factor()
    lower, alpha_t = model._factor[:n, :n], model._alpha_t[:, :n]
    inverse_t, precision = torch.empty((n, n), device=dev), torch.empty((n, n), device=dev)
    sums, work = torch.empty(3, device=dev), torch.empty(ops.gp_mll_plan(n, d, 1)["workspace_floats"], device=dev)
    ops.gram_upper_(precision, ops.tri_inverse_t(lower, out=inverse_t))
    phases = {"inverse_ms": lambda: ops.tri_inverse_t(lower, out=inverse_t), "gram_ms": lambda: ops.gram_upper_(precision, inverse_t),
              "sums_ms": lambda: ops.se_mll_sums(tx, 1.0, lengthscale, precision, alpha_t, out=sums, workspace=work)}
    fns = {"factor_ms": factor, "value_ms": value, "value_grads_ms": value_grads, **phases, "torch_value_ms": torch_value,
           "torch_value_grads_ms": torch_value_grads}
    med, spread = alternate(fns, iters, rounds)
    row = {"n": n, "d": d, "p": 1, "noise_var": NOISE, "lengthscale": lengthscale, "plan": ops.gp_mll_plan(n, d, 1), **med, "min_max_ms": spread,
           "calls_per_round": iters, "grads_vs_factor": med["value_grads_ms"] / med["factor_ms"],
           "value_vs_factor": med["value_ms"] / med["factor_ms"], "slowest_phase": max(phases, key=lambda k: med[k]),
           "phases_tflops_of_n3_over_3": {k: n ** 3 / 3 / med[k] / 1e9 for k in ("inverse_ms", "gram_ms")},
           "vs_torch_value": med["torch_value_ms"] / med["value_ms"], "vs_torch_value_grads": med["torch_value_grads_ms"] / med["value_grads_ms"]}
    if n <= 4096:
        ref = leaves(hyper, dev, torch.float64)
        want = torch_evidence(tx.double(), ty.double(), *ref)
        want.backward()
        ours_value, ours_grads = model_grads(model)
        eager = leaves(hyper, dev, torch.float32)
        eager_value = torch_evidence(tx, ty, *eager)
        eager_value.backward()
        rel = lambda got, ref_: abs(float(got.detach()) - float(ref_.detach())) / abs(float(ref_.detach()))  # noqa: E731
        row["err_vs_float64"] = {
            "ours": {"value": rel(ours_value, want), **{k: rel(g, r.grad) for k, g, r in zip(NAMES, ours_grads, ref)}},
            "torch_fp32": {"value": rel(eager_value, want), **{k: rel(e.grad, r.grad) for k, e, r in zip(NAMES, eager, ref)}}}
    print(json.dumps({k: v for k, v in row.items() if k != "plan"}), flush=True)
    return row


def optimize_row(dev, rounds, n=1024, steps=50, lr=0.05):
    tx, ty, lengthscale = data(n, 1, dev)

    def ours():
        model = make_model(1.0, dev, noise=1.0)
        model.fit(tx, ty)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        seen = model.optimize_hyperparameters(steps, lr)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, seen[-1]

    def eager():
        logs = leaves((0.0, 0.0, 0.0), dev, torch.float32)
        mean = leaves((0.0,), dev, torch.float32)[0]
        opt = torch.optim.Adam(logs + [mean], lr=lr)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            opt.zero_grad()
            out = torch_evidence(tx, ty, logs[0].exp(), logs[1].exp(), logs[2].exp(), mean)
            (-out).backward()
            opt.step()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, float(out.detach())

    ours(), eager()
    ts, last = {"ours": [], "torch_fp32": []}, {}
    for _ in range(rounds):
        for name, fn in (("ours", ours), ("torch_fp32", eager)):
            ms, last[name] = fn()
            ts[name].append(ms)
    out = {"n": n, "d": 1, "steps": steps, "lr": lr, "ours_ms": statistics.median(ts["ours"]), "torch_fp32_ms": statistics.median(ts["torch_fp32"]),
           "min_max_ms": {k: [min(v), max(v)] for k, v in ts.items()}, "last_value_seen": last}
    out["vs_torch"] = out["torch_fp32_ms"] / out["ours_ms"]
    print(json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gp_mll.json"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--max-seconds", type=float, default=480.0)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "gp_mll_bench needs the MI355X"
    dev = torch.device("cuda:0")
    t0 = time.perf_counter()
    rec = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "rounds": a.rounds, "evidence": [], "left_out": []}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    jobs = [(f"evidence n={n} d={d}", lambda n=n, d=d, it=it: rec["evidence"].append(evidence_row(n, d, it, dev, a.rounds))) for n, d, it in SHAPES]
    jobs.insert(2, ("optimize", lambda: rec.__setitem__("optimize", optimize_row(dev, a.rounds))))
    for name, job in jobs:
        if time.perf_counter() - t0 > a.max_seconds:
            rec["left_out"].append(name)
            continue
        job()
        torch.cuda.empty_cache()
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=1)
    print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
