"""FVBN training step on the MI355X: the recipe's model (FullyVisibleBeliefNetwork(784)) at batch 64 and 512, and D = 3072 at
batch 512.

usage: python tools/fvbn_bench.py [--out profiles/fvbn.json] [--iters 20] [--rounds 5]

* `graphed_step_ms`: one captured training step (zero_grad, forward, the recipe's BCE loss, backward, FlatAdam) of the packed
  route replayed from a hipGraph (graph.GraphedTrainStep, as trainer.Trainer runs it).
* FOR COMPARISON ONLY: `dense_masked_step_ms`, the route the library already had — a dense (D, D) weight through
  ops.masked_linear with strict degrees and FlatAdam, graphed the same way — and, at D = 784, `eager_loop_ms`, the reference's
  algorithm restated in eager torch-ROCm on the same GPU: a list of 784 nn.Linear(max(1, i), 1) and torch.optim.Adam.
* `forward_ms` / `wgrad_ms`: the forward launch and the weight-gradient launches of ops.fvbn alone, with the rate they reach on
  the flops of the triangle, 2 N D (D - 1) / 2 each; `dense_forward_ms` / `dense_backward_ms`: the same of the dense route
  (its backward also builds no data gradient: x does not require one).
Protocol: the candidates alternate, `--rounds` rounds of `--iters` timed calls each between HIP events after a warm-up; the
figure is the median over the rounds of the per-call mean; every call takes the next of four resident input batches.
* `sampling`: whole sample() calls of FullyVisibleBeliefNetwork(784) at n = 1 / 16 / 64 on both routes, same protocol.
* `parity`: ops.fvbn against float64 on the same GPU over the shapes of tests/test_gpu_fvbn.py: the worst max-normalised error
  of the logits and of the two gradients.
"""

import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pytorch-generative_amd"))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

SETS = 4
SHAPES = ((784, 64), (784, 512), (3072, 512))  # (D, N)
PARITY_D = (1, 2, 3, 4, 5, 15, 16, 17, 63, 64, 65, 130, 200, 193)
PARITY_N = (1, 3, 64, 65, 257)


def batches(d, n, dev):
    g = torch.Generator().manual_seed(n)
    return [torch.bernoulli(torch.full((n, d), 0.13), generator=g).to(dev) for _ in range(SETS)]


def bce(xx, preds):
    from pytorch_generative_amd import ops

    return ops.bce_with_logits_sum_mean(preds, xx)


def graphed_step(d, xs, dev):
    from pytorch_generative_amd import graph, optim
    from pytorch_generative_amd.models.autoregressive import fvbn

    torch.manual_seed(0)
    model = fvbn.FullyVisibleBeliefNetwork(d).to(dev)
    opt = optim.FlatAdam(model.parameters(), lr=1e-3)
    step = graph.GraphedTrainStep(model, opt, bce, xs[0])
    return lambda k: step(xs[k % SETS])


class DenseMasked(torch.nn.Module):
    """The route the library had before the packed kernels: a dense (D, D) weight, masked to the strict lower triangle."""

    def __init__(self, d):
        super().__init__()
        self.weight = torch.nn.Parameter((torch.rand(d, d) * 2 - 1) / d ** 0.5)
        self.bias = torch.nn.Parameter(torch.zeros(d))
        self.register_buffer("deg", torch.arange(d, dtype=torch.int32))

    def forward(self, x):
        from pytorch_generative_amd import ops

        return ops.masked_linear(x, self.weight, self.bias, self.deg, self.deg, strict=True)


def dense_masked_step(d, xs, dev):
    from pytorch_generative_amd import graph, optim

    torch.manual_seed(0)
    model = DenseMasked(d).to(dev)
    opt = optim.FlatAdam(model.parameters(), lr=1e-3)
    step = graph.GraphedTrainStep(model, opt, bce, xs[0])
    return lambda k: step(xs[k % SETS])


def eager_loop_step(d, xs, dev):
    """The reference's fvbn.py:34-45 and its recipe, eager."""
    torch.manual_seed(0)
    net = torch.nn.ModuleList(torch.nn.Linear(max(1, i), 1) for i in range(d)).to(dev)
    opt = torch.optim.Adam(net.parameters())

    def f(k):
        x = xs[k % SETS]
        opt.zero_grad()
        out = [net[0](torch.zeros(x.shape[0], 1, device=dev))]
        for i in range(1, d):
            out.append(net[i](x[:, :i]))
        preds = torch.stack(out, dim=1).view(x.shape)
        (F.binary_cross_entropy_with_logits(preds, x, reduction="none").sum() / x.shape[0]).backward()
        opt.step()

    return f


def ops_alone(d, xs, dev):
    from pytorch_generative_amd import ops
    from pytorch_generative_amd.models.autoregressive import fvbn

    torch.manual_seed(0)
    model = fvbn.FullyVisibleBeliefNetwork(d).to(dev)
    dense = DenseMasked(d).to(dev)
    g = torch.randn_like(xs[0])
    y = ops.fvbn(xs[0], model._weight, model._bias)
    yd = dense(xs[0])

    def fwd(k):
        with torch.no_grad():
            ops.fvbn(xs[k % SETS], model._weight, model._bias)

    def wgrad(k):
        torch.autograd.grad(y, [model._weight, model._bias], g, retain_graph=True)

    def dense_fwd(k):
        with torch.no_grad():
            dense(xs[k % SETS])

    def dense_bwd(k):
        torch.autograd.grad(yd, [dense.weight, dense.bias], g, retain_graph=True)

    return fwd, wgrad, dense_fwd, dense_bwd


def time_round(fn, iters, k0):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for k in range(iters):
        fn(k0 + k)
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters


def alternate(fns, rounds):
    """{name: median over the rounds of the mean ms per call}, the candidates taking turns inside every round."""
    for name, (fn, it) in fns.items():
        for k in range(max(2, it // 4)):
            fn(k)
    torch.cuda.synchronize()
    ts = {name: [] for name in fns}
    for r in range(rounds):
        for name, (fn, it) in fns.items():
            ts[name].append(time_round(fn, it, r * it))
    return {name: statistics.median(v) for name, v in ts.items()}, {name: [min(v), max(v)] for name, v in ts.items()}


def sampling(dev, iters, rounds):
    from pytorch_generative_amd.models.autoregressive import fvbn

    torch.manual_seed(0)
    model = fvbn.FullyVisibleBeliefNetwork(784).to(dev)
    rows = []
    for n in (1, 16, 64):
        fns = {"chain_ms": (lambda k, n=n: model.sample(n), iters), "full_ms": (lambda k, n=n: model.sample(n, incremental=False),
                                                                               max(2, iters // 10))}
        med, spread = alternate(fns, rounds)
        rows.append({"n": n, "D": 784, **med, "min_max_ms": spread, "speedup": med["full_ms"] / med["chain_ms"]})
        print(json.dumps(rows[-1]), flush=True)
    return rows


def parity(dev):
    from pytorch_generative_amd import ops

    err = lambda got, want: float((got.double() - want).abs().max() / want.abs().max().clamp_min(1e-30))  # noqa: E731
    rows = []
    for d in PARITY_D:
        for n in PARITY_N:
            g = torch.Generator().manual_seed(d * 1000 + n)
            x, dy = torch.randn(n, d, generator=g).to(dev), torch.randn(n, d, generator=g).to(dev)
            w, b = (torch.randn(d, d, generator=g) / d ** 0.5).to(dev), (torch.randn(d, generator=g) * 0.3).to(dev)
            wp = ops.fvbn_pack(w).requires_grad_(True)
            bb = b.clone().requires_grad_(True)
            y = ops.fvbn(x, wp, bb)
            y.backward(dy)
            want = x.double() @ torch.tril(w.double(), -1).t() + b.double()
            want_dw = torch.tril(dy.double().t() @ x.double(), -1)
            row = {"D": d, "N": n, "logits": err(y.detach(), want), "db": err(bb.grad, dy.double().sum(0))}
            if d > 1:
                row["dW"] = err(torch.tril(ops.fvbn_unpack(wp.grad, d), -1), want_dw)
            rows.append(row)
    return {"reference": "x tril(W, -1)^T + b and its gradients in float64, same GPU", "gate": 1e-4, "shapes": len(rows),
            "worst_output_err": max(r["logits"] for r in rows),
            "worst_gradient_err": max(max(r.get("dW", 0.0), r["db"]) for r in rows)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fvbn.json"))
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "fvbn_bench needs the MI355X"
    dev = torch.device("cuda:0")
    from pytorch_generative_amd import ops

    rows = []
    for d, n in SHAPES:
        xs = batches(d, n, dev)
        fwd, wgrad, dense_fwd, dense_bwd = ops_alone(d, xs, dev)
        fns = {"graphed_step_ms": (graphed_step(d, xs, dev), a.iters * 10), "dense_masked_step_ms": (dense_masked_step(d, xs, dev), a.iters * 10),
               "forward_ms": (fwd, a.iters * 10), "wgrad_ms": (wgrad, a.iters * 10),
               "dense_forward_ms": (dense_fwd, a.iters * 10), "dense_backward_ms": (dense_bwd, a.iters * 10)}
        if d == 784:
            fns["eager_loop_ms"] = (eager_loop_step(d, xs, dev), max(2, a.iters // 10))
        med, spread = alternate(fns, a.rounds)
        flops = n * d * (d - 1)  # of the triangle, forward and weight gradient each
        row = {"N": n, "D": d, "plan": ops.fvbn_plan(d, n), **med, "min_max_ms": spread,
               "calls_per_round": {k: it for k, (_, it) in fns.items()},
               "triangle_gflop": flops / 1e9, "forward_tflops": flops / med["forward_ms"] / 1e9, "wgrad_tflops": flops / med["wgrad_ms"] / 1e9,
               "step_vs_dense_masked": med["dense_masked_step_ms"] / med["graphed_step_ms"],
               "forward_vs_dense": med["dense_forward_ms"] / med["forward_ms"], "wgrad_vs_dense": med["dense_backward_ms"] / med["wgrad_ms"]}
        if d == 784:
            row["speedup_vs_eager_loop"] = med["eager_loop_ms"] / med["graphed_step_ms"]
        print(json.dumps({k: v for k, v in row.items() if k != "plan"}), flush=True)
        rows.append(row)
        del fns, fwd, wgrad, dense_fwd, dense_bwd
        torch.cuda.empty_cache()
    rec = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "iters": a.iters, "rounds": a.rounds,
           "input_sets": SETS, "rows": rows, "sampling": sampling(dev, a.iters, a.rounds), "parity": parity(dev)}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
    print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
