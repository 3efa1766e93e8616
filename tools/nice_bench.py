"""NICE training step on the MI355X: the recipe's model (NICE(784), 4 coupling blocks, 5 hidden layers of 1000) at batch 1024
and 64.

usage: python tools/nice_bench.py [--out profiles/nice.json] [--iters 10] [--rounds 5]

* `graphed_step_ms`: one captured training step (zero_grad, forward, the recipe's logistic-prior loss, backward, FlatAdam)
  replayed from a hipGraph (graph.GraphedTrainStep, as trainer.Trainer runs it), on the dense GEMMs of csrc/dense_linear.hip.
* FOR COMPARISON ONLY, two baselines on the same GPU:
  (a) `eager_step_ms`: the reference's algorithm restated in nn.Linear + torch.cat, softplus loss, torch.optim.Adam, eager;
  (b) `masked_mlp_step_ms`: the same model with every coupling network routed through the unmasked ops.masked_mlp (the 64 x 32
      tile kernels of csrc/masked_linear.hip — what the library could do before the dense family) and torch.cat, otherwise the
      same scaling layer, loss, FlatAdam and hipGraph.
* `forward_ms` / `backward_ms` of the three, outside a graph (forward under no_grad; backward of a retained graph).
* `gemm`: the three launches alone at (N, in, out) = (1024, 1000, 1000), (1024, 392, 1000), (1024, 1000, 392) and, for the
  128 x 128 tile variant, (4096, 1000, 1000): ms and achieved TFLOP/s (2 N in out flop) against the 157.3 TFLOP/s fp32 matrix
  peak, the k-split's reduce launch included.
* `sample_ms`: wall time of sample(64) and sample(1024), synchronised.
Protocol: the candidates alternate, `--rounds` rounds of `--iters` timed calls each between HIP events after a warm-up; the figure
is the median over the rounds of the per-call mean. Every call takes the next of the resident input sets: the model's parameters
and Adam state (about 390 MB) already exceed the 256 MB Infinity Cache; the GEMM launches rotate over 24 operand sets (> 256 MB).
"""

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pytorch-generative_amd"))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402
from torch import nn  # noqa: E402

FEATURES, BLOCKS, LAYERS, HIDDEN = 784, 4, 5, 1000
SETS = 4
GEMM_SETS = 24
PEAK_TFLOPS = 157.3


def batches(n, dev):
    g = torch.Generator().manual_seed(n)
    return [torch.rand(n, 1, 28, 28, generator=g).to(dev) for _ in range(SETS)]


class EagerNICE(nn.Module):
    """The reference's algorithm (flow/nice.py) in nn.Linear + torch.cat."""

    def __init__(self):
        super().__init__()
        half = FEATURES // 2
        self.nets = nn.ModuleList()
        for _ in range(BLOCKS):
            net = [nn.Linear(half, HIDDEN), nn.ReLU()]
            for _ in range(LAYERS - 1):
                net += [nn.Linear(HIDDEN, HIDDEN), nn.ReLU()]
            net.append(nn.Linear(HIDDEN, half))
            self.nets.append(nn.Sequential(*net))
        self.log_scale = nn.Parameter(torch.zeros(1, FEATURES))

    def forward(self, x):
        shape = x.shape
        x = x.view(shape[0], -1)
        c = x.shape[1]
        for b, net in enumerate(self.nets):
            h1, h2 = x[:, : c // 2], x[:, c // 2:]
            if b % 2:
                h1 = h1 + net(h2)
            else:
                h2 = h2 + net(h1)
            x = torch.cat((h1, h2), dim=1)
        return (x * torch.exp(self.log_scale)).view(shape), self.log_scale.sum()


def eager_loss(preds):
    z, ldj = preds
    log_prob = -(F.softplus(z) + F.softplus(-z)).sum(dim=(1, 2, 3))
    return -(log_prob + ldj).mean()


def new_model(dev, masked_mlp=False):
    from pytorch_generative_amd import ops
    from pytorch_generative_amd.models.flows import nice

    torch.manual_seed(0)
    model = nice.NICE(FEATURES, BLOCKS, LAYERS, HIDDEN).to(dev)
    if masked_mlp:
        def couple(self, x, sign):
            c = x.shape[1]
            layers = [(m.weight, m.bias, None, None, False) for m in self.net if isinstance(m, nn.Linear)]
            h1, h2 = x[:, : c // 2], x[:, c // 2:]
            if self.reverse:
                h1 = h1 + sign * ops.masked_mlp(h2.contiguous(), layers)
            else:
                h2 = h2 + sign * ops.masked_mlp(h1.contiguous(), layers)
            return torch.cat((h1, h2), dim=1)

        for block in model.net:
            block._couple = couple.__get__(block)
    return model


def graphed_step(xs, dev, masked_mlp):
    from pytorch_generative_amd import graph, optim, recipes

    model = new_model(dev, masked_mlp)
    opt = optim.FlatAdam(model.parameters(), lr=1e-3)
    step = graph.GraphedTrainStep(model, opt, lambda xx, preds: recipes.nice_loss(xx, None, preds), xs[0])
    return (lambda k: step(xs[k % SETS])), model


def eager_step(xs, dev):
    torch.manual_seed(0)
    model = EagerNICE().to(dev)
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)

    def f(k):
        opt.zero_grad()
        eager_loss(model(xs[k % SETS])).backward()
        opt.step()

    return f, model


def fwd_bwd_alone(model, xs, loss):
    out = loss(model(xs[0]))

    def fwd(k):
        with torch.no_grad():
            model(xs[k % SETS])

    def bwd(k):
        out.backward(retain_graph=True)  # gradients accumulate into the sinks / param.grad: timing only

    return fwd, bwd


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


def gemm_launches(n, i, o, dev):
    """{name: fn(k)} of the three launches on rotating operand sets, and the plans."""
    from pytorch_generative_amd import _lib, ops

    lib = _lib.load()
    g = torch.Generator().manual_seed(i + o)
    sets = []
    for _ in range(GEMM_SETS):
        sets.append([torch.randn(n, i, generator=g).to(dev), (torch.randn(o, i, generator=g) / i ** 0.5).to(dev),
                     torch.randn(o, generator=g).to(dev), torch.randn(n, o, generator=g).to(dev),
                     torch.empty(n, o, device=dev), torch.empty(n, i, device=dev), torch.zeros(o, i, device=dev),
                     torch.zeros(o, device=dev)])
    plans = {k: ops.dense_linear_plan(n, i, o, k) for k in ("fwd", "dgrad", "wgrad")}
    ws = {k: torch.empty(max(1, p["workspace_floats"]), device=dev) for k, p in plans.items()}
    st = torch.cuda.current_stream().cuda_stream

    def fwd(k):
        x, w, b, dy, y, dx, dw, db = sets[k % GEMM_SETS]
        _lib.check(lib.pg_dense_linear_fwd(x.data_ptr(), i, w.data_ptr(), b.data_ptr(), 0, 0, 1, y.data_ptr(), o, n, i, o, 1,
                                           ws["fwd"].data_ptr(), plans["fwd"]["workspace_floats"], st), "fwd")

    def dgrad(k):
        x, w, b, dy, y, dx, dw, db = sets[k % GEMM_SETS]
        _lib.check(lib.pg_dense_linear_dgrad(dy.data_ptr(), o, w.data_ptr(), x.data_ptr(), i, 0, 0, 1, dx.data_ptr(), i, n, i, o,
                                             ws["dgrad"].data_ptr(), plans["dgrad"]["workspace_floats"], st), "dgrad")

    def wgrad(k):
        x, w, b, dy, y, dx, dw, db = sets[k % GEMM_SETS]
        _lib.check(lib.pg_dense_linear_wgrad(x.data_ptr(), i, dy.data_ptr(), o, 1, dw.data_ptr(), db.data_ptr(), n, i, o,
                                             ws["wgrad"].data_ptr(), plans["wgrad"]["workspace_floats"], st), "wgrad")

    return {"fwd": fwd, "dgrad": dgrad, "wgrad": wgrad}, plans


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nice.json"))
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "nice_bench needs the MI355X"
    dev = torch.device("cuda:0")
    from pytorch_generative_amd import recipes

    nice_loss = lambda preds: recipes.nice_loss(None, None, preds)["loss"]  # noqa: E731
    rows = []
    for n in (1024, 64):
        xs = batches(n, dev)
        new, model_new = graphed_step(xs, dev, False)
        old, model_old = graphed_step(xs, dev, True)
        eager, model_eager = eager_step(xs, dev)
        fns = {"graphed_step_ms": (new, a.iters), "masked_mlp_step_ms": (old, a.iters), "eager_step_ms": (eager, a.iters)}
        # forward / backward alone run on models of their own: an optimiser step between two backward passes of a retained
        # graph would invalidate it
        torch.manual_seed(0)
        alone = (("", new_model(dev, False), nice_loss), ("masked_mlp_", new_model(dev, True), nice_loss),
                 ("eager_", EagerNICE().to(dev), eager_loss))
        for tag, model, loss in alone:
            fwd, bwd = fwd_bwd_alone(model, xs, loss)
            fns[tag + "forward_ms"], fns[tag + "backward_ms"] = (fwd, a.iters), (bwd, a.iters)
        med, spread = alternate(fns, a.rounds)
        row = {"N": n, **med, "min_max_ms": spread, "calls_per_round": a.iters,
               "step_ratio_masked_mlp_over_dense": med["masked_mlp_step_ms"] / med["graphed_step_ms"],
               "step_ratio_eager_over_dense": med["eager_step_ms"] / med["graphed_step_ms"]}
        print(json.dumps({k: v for k, v in row.items() if k != "min_max_ms"}), flush=True)
        rows.append(row)
        if n == 1024:
            sample_ms = {}
            model_new(xs[0])
            for m in (64, 1024):
                model_new.sample(m)
                torch.cuda.synchronize()
                ts = []
                for _ in range(a.rounds):
                    t0 = time.perf_counter()
                    model_new.sample(m)
                    torch.cuda.synchronize()
                    ts.append((time.perf_counter() - t0) * 1e3)
                sample_ms[str(m)] = statistics.median(ts)
            print(json.dumps({"sample_ms": sample_ms}), flush=True)
        del fns, new, old, eager, model_new, model_old, model_eager, alone, fwd, bwd
        torch.cuda.empty_cache()
    gemm = []
    # the last shape is the smallest multiple of the recipe's batch at which the plan takes the 128 x 128 tile (forward and data
    # gradient: 32 x 8 = 256 large tiles; the weight gradient stays on the small one)
    for n, i, o in ((1024, 1000, 1000), (1024, 392, 1000), (1024, 1000, 392), (4096, 1000, 1000)):
        launches, plans = gemm_launches(n, i, o, dev)
        med, spread = alternate({k: (fn, a.iters * 4) for k, fn in launches.items()}, a.rounds)
        rec = {"N": n, "in": i, "out": o, "ms": med, "min_max_ms": spread,
               "tflops": {k: 2.0 * n * i * o / (v * 1e-3) / 1e12 for k, v in med.items()},
               "plan": {k: {f: p[f] for f in ("variant", "slices", "workgroups")} for k, p in plans.items()}}
        rec["fraction_of_peak"] = {k: v / PEAK_TFLOPS for k, v in rec["tflops"].items()}
        print(json.dumps({k: v for k, v in rec.items() if k != "min_max_ms"}), flush=True)
        gemm.append(rec)
        del launches
        torch.cuda.empty_cache()
    rec = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "iters": a.iters, "rounds": a.rounds,
           "model": {"n_features": FEATURES, "n_coupling_blocks": BLOCKS, "n_hidden_layers": LAYERS, "n_hidden_features": HIDDEN},
           "input_sets": SETS, "gemm_operand_sets": GEMM_SETS, "fp32_matrix_peak_tflops": PEAK_TFLOPS, "rows": rows,
           "sample_ms": sample_ms, "gemm": gemm}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
    print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
