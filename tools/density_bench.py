"""Density estimators on the MI355X: the mixture models' training step and Gaussian / Parzen KDE scoring.

usage: python tools/density_bench.py [--out profiles/density.json] [--iters 30] [--warmup 5] [--quick]

* `mixture_step`: one training step (zero_grad, forward, loss = -mean log p, backward, FlatAdam) of a Gaussian and a
  Bernoulli mixture at F = 784 for several (N, K), captured and replayed from a hipGraph (graph.GraphedTrainStep);
  HIP-event median after warm-up. `eager_torch_reference_ms`: FOR COMPARISON ONLY, the reference's algorithm (its
  (N, K, F) broadcasts, log_softmax, logsumexp, autograd, torch.optim.Adam) in eager torch-ROCm on the same GPU.
* `kde`: log p of M test rows under N training rows at sizes where the reference's (M, N, d) difference tensor still
  fits in memory, ours next to the reference's formula in eager torch; both outputs are compared.
* `kde_mnist`: Gaussian KDE at MNIST's size (10 000 test x 60 000 train x 784), where the reference's algorithm would
  need 1.9 PB. Achieved FLOP/s are the GEMM's 2 M N d operations over the call's time (prepare kernels and split-K
  merge included: an end-to-end rate, not a kernel's), next to the 157.3 TFLOP/s fp32 matrix peak of the MI355X.
Ratios are recorded as measured, including any below 1.
"""

import argparse
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pytorch-generative_amd"))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

FEATURES = 784
FP32_MATRIX_PEAK_TFLOPS = 157.3


def timed(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        torch.cuda.synchronize()
        ts.append(s.elapsed_time(e))
    return statistics.median(ts)


def batch(kind, n, dev):
    g = torch.Generator().manual_seed(n)
    if kind == "gaussian":
        return torch.randn((n, 1, 28, 28), generator=g).to(dev)
    return torch.bernoulli(torch.full((n, 1, 28, 28), 0.13), generator=g).to(dev)


def graphed_step(kind, n, k, dev):
    from pytorch_generative_amd import graph, models, optim

    torch.manual_seed(0)
    cls = models.GaussianMixtureModel if kind == "gaussian" else models.BernoulliMixtureModel
    model = cls(k, FEATURES).to(dev)
    opt = optim.FlatAdam(model.parameters(), lr=1e-3)
    step = graph.GraphedTrainStep(model, opt, lambda xx, preds: -preds.mean(), batch(kind, n, dev))
    return lambda: step()


def eager_reference_step(kind, n, k, dev):
    """The reference's mixture_models.py step in eager torch."""
    torch.manual_seed(0)
    mix = torch.ones(k, device=dev, requires_grad=True)
    if kind == "gaussian":
        params = [(torch.randn(k, FEATURES, device=dev) * 0.01).requires_grad_(True),
                  torch.zeros(k, FEATURES, device=dev, requires_grad=True)]
    else:
        params = [torch.rand(k, FEATURES, device=dev).requires_grad_(True)]
    opt = torch.optim.Adam([mix] + params)
    x = batch(kind, n, dev).view(n, 1, FEATURES)

    def f():
        opt.zero_grad()
        if kind == "gaussian":
            mean, log_std = params
            z = -log_std - 0.5 * math.log(2 * math.pi)
            comp = (z - 0.5 * ((x.unsqueeze(dim=1) - mean) / log_std.exp()) ** 2).sum(-1)
        else:
            logits, xb = torch.broadcast_tensors(params[0], x)
            comp = -F.binary_cross_entropy_with_logits(logits, xb, reduction="none").sum(-1)
        out = torch.logsumexp(torch.log_softmax(mix, dim=-1) + comp, dim=-1)
        (-out.mean()).backward()
        opt.step()

    return f


def reference_gaussian_kde(test, train, h):
    n, d = train.shape
    z = 0.5 * d * math.log(2 * math.pi) + d * math.log(h) + math.log(n)
    diffs = (test.view(test.shape[0], 1, d) - train.view(1, n, d)) / h
    return torch.logsumexp(-0.5 * torch.norm(diffs, p=2, dim=-1) ** 2 - z, dim=-1)


def reference_parzen_kde(test, train, h):
    n, d = train.shape
    abs_diffs = torch.abs(test.view(test.shape[0], 1, d) - train.view(1, n, d))
    inside = torch.sum(abs_diffs / h <= 0.5, dim=2) == d
    return torch.log(((1 / h ** d) * inside).mean(dim=1))


def kde_inputs(m, n, d, dev):
    g = torch.Generator(device=dev).manual_seed(m + n + d)
    sparse = lambda r: torch.rand(r, d, device=dev, generator=g) * (torch.rand(r, d, device=dev, generator=g) < 0.2)  # noqa: E731
    return sparse(m), sparse(n)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "density.json"))
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--quick", action="store_true", help="small sizes only (a rehearsal of the tool itself)")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "density_bench needs the MI355X"
    from pytorch_generative_amd import ops

    dev = torch.device("cuda:0")
    rec = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "iters": a.iters, "warmup": a.warmup,
           "features": FEATURES, "fp32_matrix_peak_tflops": FP32_MATRIX_PEAK_TFLOPS, "mixture_step": [], "kde": []}

    shapes = [(64, 10), (1024, 10)] if a.quick else [(64, 10), (1024, 10), (1024, 64), (4096, 32)]
    for kind in ("gaussian", "bernoulli"):
        for n, k in shapes:
            row = {"kind": kind, "N": n, "K": k, "F": FEATURES,
                   "graphed_step_ms": timed(graphed_step(kind, n, k, dev), a.iters, a.warmup)}
            torch.cuda.empty_cache()
            row["eager_torch_reference_ms"] = timed(eager_reference_step(kind, n, k, dev), a.iters, a.warmup)
            row["speedup_vs_eager_torch"] = row["eager_torch_reference_ms"] / row["graphed_step_ms"]
            row["reference_intermediate_bytes"] = 4 * n * k * FEATURES
            torch.cuda.empty_cache()
            print(json.dumps(row), flush=True)
            rec["mixture_step"].append(row)

    kde_shapes = [(256, 2000, 64)] if a.quick else [(2000, 2000, 64), (500, 5000, 784)]
    for m, n, d in kde_shapes:
        test, train = kde_inputs(m, n, d, dev)
        h = 0.2 if d == 784 else 0.5
        row = {"M_test": m, "N_train": n, "d": d, "bandwidth": h,
               "reference_difference_tensor_bytes": 4 * m * n * d, "flop": 2 * m * n * d}
        ours, ref = ops.kde_gaussian(test, train, h), reference_gaussian_kde(test, train, h)
        row["gaussian_max_abs_diff_vs_reference"] = float((ours - ref).abs().max())
        row["gaussian_max_abs_reference"] = float(ref.abs().max())
        del ours, ref
        row["gaussian_ms"] = timed(lambda: ops.kde_gaussian(test, train, h), a.iters, a.warmup)
        row["gaussian_tflops"] = row["flop"] / row["gaussian_ms"] / 1e9
        row["gaussian_eager_torch_reference_ms"] = timed(lambda: reference_gaussian_kde(test, train, h), a.iters, a.warmup)
        row["gaussian_speedup_vs_eager_torch"] = row["gaussian_eager_torch_reference_ms"] / row["gaussian_ms"]
        torch.cuda.empty_cache()
        hp = 1.0  # wide windows: at d = 784 narrow ones overflow 1 / h**d
        row["parzen_bandwidth"] = hp
        ours, ref = ops.kde_parzen(test, train, hp), reference_parzen_kde(test, train, hp)
        pin = lambda t: torch.nan_to_num(t, nan=3e38, posinf=2e38, neginf=-2e38)  # noqa: E731
        row["parzen_equal_to_reference"] = bool(torch.allclose(pin(ours), pin(ref), rtol=1e-6, atol=0))
        del ours, ref
        row["parzen_ms"] = timed(lambda: ops.kde_parzen(test, train, hp), a.iters, a.warmup)
        row["parzen_eager_torch_reference_ms"] = timed(lambda: reference_parzen_kde(test, train, hp), a.iters, a.warmup)
        row["parzen_speedup_vs_eager_torch"] = row["parzen_eager_torch_reference_ms"] / row["parzen_ms"]
        torch.cuda.empty_cache()
        print(json.dumps(row), flush=True)
        rec["kde"].append(row)

    if not a.quick:
        m, n, d = 10000, 60000, 784
        test, train = kde_inputs(m, n, d, dev)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        ms = timed(lambda: ops.kde_gaussian(test, train, 0.2), max(5, a.iters // 3), 2)
        row = {"M_test": m, "N_train": n, "d": d, "bandwidth": 0.2, "gaussian_ms": ms, "flop": 2 * m * n * d,
               "gaussian_tflops_end_to_end": 2 * m * n * d / ms / 1e9,
               "share_of_fp32_matrix_peak": 2 * m * n * d / ms / 1e9 / FP32_MATRIX_PEAK_TFLOPS,
               "peak_extra_memory_bytes": torch.cuda.max_memory_allocated() - base,
               "reference_difference_tensor_bytes": 4 * m * n * d}
        print(json.dumps(row), flush=True)
        rec["kde_mnist"] = row

    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
    print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
