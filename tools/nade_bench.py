"""NADE training step on the MI355X: the recipe's model (NADE(784, 500)) at batch 64 and 512.

usage: python tools/nade_bench.py [--out profiles/nade.json] [--iters 20] [--rounds 5]

* `graphed_step_ms`: one captured training step (zero_grad, forward, the recipe's BCE loss, backward, FlatAdam) replayed from a
  hipGraph (graph.GraphedTrainStep, as trainer.Trainer runs it).
* FOR COMPARISON ONLY, two baselines in eager torch-ROCm on the same GPU, each a full step with torch.optim.Adam:
  `eager_loop_ms`, the reference's algorithm (a Python loop over the 784 dimensions), and `eager_cumsum_ms`, the vectorised
  formulation a torch user would write (an exclusive cumsum over an (N, D, H) tensor, relu, a multiply and a sum).
* `forward_ms` / `backward_ms`: the two forward launches and the four backward launches of ops.nade alone.
Protocol: the three steps alternate, `--rounds` rounds of `--iters` timed calls each between HIP events after a warm-up; the
figure is the median over the rounds of the per-call mean; every call takes the next of four resident input batches.
* `parity`: ops.nade against the per-dimension loop in float64 on the same GPU at the recipe's D = 784, H = 500 and at three
  edge shapes: the max-normalised error of the logits, the probabilities and the four gradients, and the worst of them.
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

D, HIDDEN = 784, 500
SETS = 4


def batches(n, dev):
    g = torch.Generator().manual_seed(n)
    return [torch.bernoulli(torch.full((n, D), 0.13), generator=g).to(dev) for _ in range(SETS)]


def loop_forward(x, in_w, in_b, h_w, h_b):
    """The reference's nade.py:49-68 with x as given."""
    a = in_b.expand(x.shape[0], -1)
    out = []
    for i in range(x.shape[1]):
        out.append(torch.relu(a) @ h_w[i:i + 1, :].t() + h_b[i:i + 1])
        a = a + x[:, i:i + 1] @ in_w[:, i:i + 1].t()
    return torch.cat(out, dim=1)


def cumsum_forward(x, in_w, in_b, h_w, h_b):
    terms = x[:, :, None] * in_w.t()[None]
    a = in_b + torch.cumsum(terms, 1) - terms
    return h_b + (torch.relu(a) * h_w[None]).sum(-1)


def new_params(dev, dtype=torch.float32):
    torch.manual_seed(0)
    in_w, h_w = torch.empty(HIDDEN, D), torch.empty(D, HIDDEN)
    torch.nn.init.kaiming_normal_(in_w)
    torch.nn.init.kaiming_normal_(h_w)
    ps = [in_w, torch.randn(HIDDEN) * 0.1, h_w, torch.randn(D) * 0.1]
    return [p.to(dev, dtype).requires_grad_(True) for p in ps]


def graphed_step(xs, dev):
    from pytorch_generative_amd import graph, ops, optim
    from pytorch_generative_amd.models.autoregressive import nade

    torch.manual_seed(0)
    model = nade.NADE(D, HIDDEN).to(dev)
    opt = optim.FlatAdam(model.parameters(), lr=1e-3)
    step = graph.GraphedTrainStep(model, opt, lambda xx, preds: ops.bce_with_logits_sum_mean(preds, xx), xs[0])
    return lambda k: step(xs[k % SETS])


def eager_step(forward, xs, dev):
    params = new_params(dev)
    opt = torch.optim.Adam(params)

    def f(k):
        x = xs[k % SETS]
        opt.zero_grad()
        p = torch.sigmoid(forward(x, *params))
        F.binary_cross_entropy_with_logits(p, x, reduction="none").sum(dim=1).mean().backward()
        opt.step()

    return f


def op_alone(xs, dev):
    from pytorch_generative_amd import ops

    params = new_params(dev)
    g = torch.randn_like(xs[0])
    p = ops.nade(xs[0], *params)

    def fwd(k):
        with torch.no_grad():
            ops.nade(xs[k % SETS], *params)

    def bwd(k):
        torch.autograd.grad(p, params, g, retain_graph=True)

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


PARITY_SHAPES = ((784, 500, 70), (67, 65, 261), (33, 1, 261), (31, 500, 2))  # (D, H, N)


def parity_one(d, h, n, dev):
    from pytorch_generative_amd import ops

    g = torch.Generator().manual_seed(d * 1000 + h)
    x = torch.bernoulli(torch.full((n, d), 0.4), generator=g).to(dev)
    dp = torch.randn(n, d, generator=g).to(dev)
    ps = [torch.randn(h, d, generator=g) * (2 / d) ** 0.5, torch.randn(h, generator=g) * 0.1,
          torch.randn(d, h, generator=g) * (2 / h) ** 0.5, torch.randn(d, generator=g) * 0.1]
    params = [q.to(dev).requires_grad_(True) for q in ps]
    p, logits = ops.nade(x, *params, return_logits=True)
    p.backward(dp)
    ref = [q.detach().double().requires_grad_(True) for q in params]
    want_l = loop_forward(x.double(), *ref)
    want_p = torch.sigmoid(want_l)
    want_p.backward(dp.double())
    err = lambda got, want: float((got.double() - want).abs().max() / want.abs().max())  # noqa: E731
    names = ("d_in_W", "d_in_b", "d_h_W", "d_h_b")
    rec = {"N": n, "D": d, "H": h, "logits_max_norm_err": err(logits, want_l.detach()),
           "probabilities_max_norm_err": err(p.detach(), want_p.detach())}
    rec.update({f"{k}_max_norm_err": err(q.grad, r.grad) for k, q, r in zip(names, params, ref)})
    return rec


def parity(dev):
    rows = [parity_one(d, h, n, dev) for d, h, n in PARITY_SHAPES]
    keys = [k for k in rows[0] if k.endswith("_err")]
    return {"reference": "per-dimension loop, float64, autograd, same GPU", "gate": 1e-4, "rows": rows,
            "worst_output_err": max(r[k] for r in rows for k in keys[:2]),
            "worst_gradient_err": max(r[k] for r in rows for k in keys[2:])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nade.json"))
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "nade_bench needs the MI355X"
    dev = torch.device("cuda:0")
    from pytorch_generative_amd import ops

    rows = []
    for n in (64, 512):
        xs = batches(n, dev)
        fwd, bwd = op_alone(xs, dev)
        fns = {"graphed_step_ms": (graphed_step(xs, dev), a.iters * 10), "eager_cumsum_ms": (eager_step(cumsum_forward, xs, dev), a.iters),
               "eager_loop_ms": (eager_step(loop_forward, xs, dev), max(2, a.iters // 10)),
               "forward_ms": (fwd, a.iters * 10), "backward_ms": (bwd, a.iters * 10)}
        med, spread = alternate(fns, a.rounds)
        row = {"N": n, "D": D, "hidden": HIDDEN, "plan": ops.nade_plan(D, HIDDEN, n), **med, "min_max_ms": spread,
               "calls_per_round": {k: it for k, (_, it) in fns.items()},
               "speedup_vs_eager_loop": med["eager_loop_ms"] / med["graphed_step_ms"],
               "speedup_vs_eager_cumsum": med["eager_cumsum_ms"] / med["graphed_step_ms"]}
        print(json.dumps({k: v for k, v in row.items() if k != "plan"}), flush=True)
        rows.append(row)
        del fns, fwd, bwd
        torch.cuda.empty_cache()
    rec = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "iters": a.iters, "rounds": a.rounds,
           "input_sets": SETS, "rows": rows, "parity": parity(dev)}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
    print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
