"""ARD lengthscales and Matern kernels of the Gaussian process on the MI355X: what they cost beside the scalar squared exponential.

usage: python tools/gp_ard_bench.py [--out profiles/gp_ard.json] [--rounds 5] [--max-seconds 480] [--test-log LOG]

One row per n = 1024, 4096, 8192 and d = 1, 8, 64 (p = 1):
* `value_grads_ms`: log_marginal_likelihood() with every hyperparameter requiring grad, and backward(), every call after
  reset_cache() (covariance, factorisation, both solves, the inverse, X X^T and the reduction are inside), for
    `scalar_se`     the "se" route, one shared lengthscale: the parent commit's path, which this work leaves bit for bit — the baseline;
    `ard_se`        SquaredExponential with one lengthscale per column ("stationary" route, ops.ard_mll_sums);
    `ard_matern52`  Matern 5/2 with one lengthscale per column;
    `shared_matern52`  Matern 5/2 with one shared lengthscale (ops.stationary_mll_sums).
* `sums_ms`: the reduction alone on a cached inverse — ops.se_mll_sums (the baseline), ops.stationary_mll_sums (Matern 5/2) and
  ops.ard_mll_sums (SE, Matern 5/2) — and `ard_sums_share`, the ARD reduction's share of its gradient evaluation.
* `covariance_ms`: the symmetric covariance launch (lower triangle, not mirrored) by kind, shared and per-dimension, beside
  ops.se_kernel.
* `err_vs_float64` (n = 1024): the relative error of the value and the worst relative error of a d/d l_c against float64
  autograd on the same GPU.
`--test-log`: the output of `pytest tests/test_gpu_gp_ard.py -s`; its worst errors over the test grid are copied into the file.
Protocol (tools/gp_mll_bench.py's): the candidates alternate in one process, `--rounds` rounds of timed calls between HIP events
after a warm-up, the figure is the median over the rounds of the per-call mean. The file is rewritten after every row; once
`--max-seconds` of wall clock have passed no further row is started and the file says which were left out."""

import argparse
import json
import math
import os
import re
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pytorch-generative_amd"))
import torch  # noqa: E402
from torch import nn  # noqa: E402

NOISE = 0.1
SHAPES = tuple((n, d, it) for n, it in ((1024, 5), (4096, 3), (8192, 2)) for d in (1, 8, 64))  # (n, d, calls per round)


def data(n, d, dev):
    """The training points of tools/gp_mll_bench.py, and per-dimension lengthscales within a factor 1.5 of its shared one."""
    g = torch.Generator().manual_seed(n + d)
    if d == 1:
        tx, lengthscale = torch.rand(n, 1, generator=g) * n / 20, 1.0
    else:
        tx, lengthscale = torch.randn(n, d, generator=g), float(d) ** 0.5
    ty = torch.sin(tx.sum(1, keepdim=True)) + NOISE ** 0.5 * torch.randn(n, 1, generator=g)
    vector = lengthscale * (0.75 + 0.75 * torch.rand(d, generator=g))
    return tx.to(dev), ty.to(dev), lengthscale, vector


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


def make_model(kind, lengthscale, dev):
    from pytorch_generative_amd.models import gaussian_process as gp

    lengthscale = nn.Parameter(lengthscale.clone() if torch.is_tensor(lengthscale) else torch.tensor(float(lengthscale)))
    std = nn.Parameter(torch.tensor(1.0))
    kernel = gp.SquaredExponential(std, lengthscale) if kind == "se" else gp.Matern(2.5, std, lengthscale)
    model = gp.GaussianProcess(gp.Const(nn.Parameter(torch.tensor(0.0))), kernel, NOISE).to(dev)
    model.noise_var.requires_grad_()
    return model


def model_grads(model):
    tensors = (model.kernel.std, model.kernel.lengthscale, model.noise_var, model.mean.value)
    for t in tensors:
        t.grad = None
    value = model.log_marginal_likelihood()
    value.backward()
    return value.detach(), [t.grad for t in tensors]


def float64_evidence(tx, ty, kind, std, lengthscale, noise, value):
    """log p(y) in float64 torch on the device; the root is taken off the diagonal only."""
    n = tx.shape[0]
    xs = tx.double() / lengthscale
    sq = (xs * xs).sum(1)
    eye = torch.eye(n, device=tx.device, dtype=torch.float64)
    r2 = (sq[:, None] + sq[None, :] - 2.0 * xs @ xs.t()).clamp_min(0.0) * (1.0 - eye)
    if kind == "se":
        phi = torch.exp(-0.5 * r2)
    else:
        s = math.sqrt(5.0) * torch.sqrt(r2 + eye) * (1.0 - eye)
        phi = (1.0 + s + s * s / 3.0) * torch.exp(-s)
    chol = torch.linalg.cholesky(std ** 2 * phi + noise * eye)
    r = ty.double() - value
    alpha = torch.cholesky_solve(r, chol)
    return -0.5 * (r * alpha).sum() - torch.log(torch.diagonal(chol)).sum() - 0.5 * n * math.log(2.0 * math.pi)


def row(n, d, iters, dev, rounds):
    from pytorch_generative_amd import ops

    tx, ty, shared, vector = data(n, d, dev)
    models = {"scalar_se": make_model("se", shared, dev), "ard_se": make_model("se", vector, dev),
              "ard_matern52": make_model("matern52", vector, dev), "shared_matern52": make_model("matern52", shared, dev)}
    for model in models.values():
        model.fit(tx, ty)

    def value_grads(model):
        def run():
            model.reset_cache()
            model_grads(model)
        return run

    fns = {f"value_grads_ms/{name}": value_grads(model) for name, model in models.items()}
    # the reduction alone, on one cached inverse (its cost does not depend on what the operands hold)
    base = models["scalar_se"]
    base._ensure_factor()
    lower, alpha_t = base._factor[:n, :n], base._alpha_t[:, :n]
    precision = torch.empty((n, n), device=dev)
    ops.gram_upper_(precision, ops.tri_inverse_t(lower))
    inv = vector.to(dev).reciprocal()
    out = torch.empty(d + 2, device=dev)
    work = torch.empty(max(ops.gp_mll_plan(n, d, 1)["workspace_floats"], ops.gp_ard_plan(n, d, 1)["workspace_floats"]), device=dev)
    fns["sums_ms/se_mll_sums"] = lambda: ops.se_mll_sums(tx, 1.0, shared, precision, alpha_t, out=out[:3], workspace=work)
    fns["sums_ms/stationary_matern52"] = lambda: ops.stationary_mll_sums(tx, 1.0, shared, precision, alpha_t, kind="matern52", out=out[:3],
                                                                       workspace=work)
    for kind in ("se", "matern52"):
        fns[f"sums_ms/ard_{kind}"] = lambda kind=kind: ops.ard_mll_sums(tx, 1.0, None, precision, alpha_t, kind=kind, out=out, workspace=work,
                                                                       inv_lengthscale=inv)
    cov = torch.empty((n, n), device=dev)
    fns["covariance_ms/se_kernel"] = lambda: ops.se_kernel(tx, tx, 1.0, shared, NOISE, out=cov, mirror=False)
    for kind in ("se", "matern32", "matern52"):
        fns[f"covariance_ms/shared_{kind}"] = lambda kind=kind: ops.stationary_kernel(tx, tx, 1.0, shared, NOISE, kind=kind, out=cov, mirror=False)
        fns[f"covariance_ms/ard_{kind}"] = lambda kind=kind: ops.stationary_kernel(tx, tx, 1.0, None, NOISE, kind=kind, out=cov, mirror=False,
                                                                               inv_lengthscale=inv)
    med, spread = alternate(fns, iters, rounds)
    rec = {"n": n, "d": d, "p": 1, "noise_var": NOISE, "shared_lengthscale": shared, "calls_per_round": iters, "ard_plan": ops.gp_ard_plan(n, d, 1),
           "covariance_route": ops.gp_plan(n, n, d, 1)["se_route"]}
    for name, ms in med.items():
        group, key = name.split("/")
        rec.setdefault(group, {})[key] = ms
    rec["min_max_ms"] = spread
    vg, sums = rec["value_grads_ms"], rec["sums_ms"]
    rec["vs_scalar_se"] = {k: vg[k] / vg["scalar_se"] for k in vg if k != "scalar_se"}
    rec["ard_sums_vs_se_sums"] = {k: sums[k] / sums["se_mll_sums"] for k in sums if k != "se_mll_sums"}
    rec["ard_sums_share"] = {k: sums[k] / vg[k] for k in ("ard_se", "ard_matern52")}
    rec["se_sums_share"] = sums["se_mll_sums"] / vg["scalar_se"]
    if n <= 1024:
        errs = {}
        for name, kind, ls in (("ard_se", "se", vector), ("ard_matern52", "matern52", vector)):
            leaves = [torch.tensor(1.0, device=dev, dtype=torch.float64, requires_grad=True), ls.to(dev).double().requires_grad_(),
                      torch.tensor(NOISE, device=dev, dtype=torch.float64, requires_grad=True),
                      torch.tensor(0.0, device=dev, dtype=torch.float64, requires_grad=True)]
            want = float64_evidence(tx, ty, kind, *leaves)
            want.backward()
            value, grads = model_grads(models[name])
            rel = lambda got, ref: float(((got.double() - ref).abs() / ref.abs()).max())  # noqa: E731
            errs[name] = {"value": rel(value, want.detach()), "std": rel(grads[0], leaves[0].grad), "lengthscale_worst": rel(grads[1], leaves[1].grad),
                          "noise_var": rel(grads[2], leaves[2].grad), "value_mean": rel(grads[3], leaves[3].grad)}
        rec["err_vs_float64"] = errs
    print(json.dumps({k: v for k, v in rec.items() if k not in ("ard_plan", "min_max_ms")}), flush=True)
    return rec


def test_grid_errors(path):
    """The worst figures the GPU tests printed (pytest -s): the covariance of the maximum, the sums of sum |terms|, the model's
    d/d l_c of sum |terms_c| / (2 l_c) and relative."""
    worst = {"covariance": [0.0, ""], "ard_sums": [0.0, ""], "shared_sums": [0.0, ""], "model_lengthscale_of_terms": [0.0, ""],
             "model_lengthscale_relative": [0.0, ""], "model_other_relative": [0.0, ""]}

    def note(key, value, what):
        if value > worst[key][0]:
            worst[key] = [value, what]

    for line in open(path):
        m = re.search(r"\[gp ard\] (.*(?:symmetric|cross|rows).*): ([0-9.e+-]+)$", line)
        if m:
            note("covariance", float(m.group(2)), m.group(1))
        m = re.search(r"\[gp ard\] (.*) ard sums: ([0-9.e+-]+) of", line)
        if m:
            note("ard_sums", float(m.group(2)), m.group(1))
        m = re.search(r"\[gp ard\] (.*) shared sums: \[(.*)\]", line)
        if m:
            note("shared_sums", max(float(v.strip("' ")) for v in m.group(2).split(",")), m.group(1))
        m = re.search(r"\[gp ard\] (model .*) d/d lengthscale: worst ([0-9.e+-]+) of .* worst relative ([0-9.e+-]+)", line)
        if m:
            note("model_lengthscale_of_terms", float(m.group(2)), m.group(1))
            note("model_lengthscale_relative", float(m.group(3)), m.group(1))
        m = re.search(r"\[gp ard\] (model .*(?:value|std|noise_var)): ([0-9.e+-]+) \(want", line)
        if m:
            note("model_other_relative", float(m.group(2)), m.group(1))
    return worst


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gp_ard.json"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--max-seconds", type=float, default=480.0)
    ap.add_argument("--test-log", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "gp_ard_bench needs the MI355X"
    dev = torch.device("cuda:0")
    t0 = time.perf_counter()
    rec = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "rounds": a.rounds, "rows": [], "left_out": []}
    if a.test_log:
        rec["test_grid_worst_errors"] = test_grid_errors(a.test_log)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    for n, d, iters in SHAPES:
        if time.perf_counter() - t0 > a.max_seconds:
            rec["left_out"].append(f"n={n} d={d}")
            continue
        rec["rows"].append(row(n, d, iters, dev, a.rounds))
        torch.cuda.empty_cache()
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=1)
    print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
