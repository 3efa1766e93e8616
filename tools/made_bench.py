"""MADE training step on the MI355X: the recipe's model (MADE(784, [8000]), n_masks = 1) at batch 64 and 1024.

usage: python tools/made_bench.py [--out profiles/made.json] [--iters 50] [--warmup 10] [--no-prof]

* `graphed_step_ms`: one captured training step (zero_grad, forward, BCE loss, backward, FlatAdam) replayed from a
  hipGraph (graph.GraphedTrainStep, as trainer.Trainer runs it); HIP-event median after warm-up.
* `eager_torch_reference_ms`: FOR COMPARISON ONLY, the reference's algorithm in eager torch-ROCm on the same GPU:
  `weight.data *= mask` + F.linear per layer, ReLU, BCE with logits, autograd, torch.optim.Adam (default settings).
* `kernels`: per-kernel device time of the graphed step from `rocprofv3 --kernel-trace --stats` (a child process of
  this script replays the step `--iters` times under the profiler; times are per step).
The GEMMs' algorithmic bytes are listed beside the times: both weight matrices read by the forward, re-read by the data
gradient of the second layer (the first layer's input needs none), and both weight gradients written.
"""

import argparse
import csv
import glob
import json
import os
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pytorch-generative_amd"))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

D, HIDDEN = 784, 8000


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


def batch(n, dev):
    g = torch.Generator().manual_seed(n)
    return torch.bernoulli(torch.full((n, 1, 28, 28), 0.13), generator=g).to(dev)


def graphed_step(n, dev):
    from pytorch_generative_amd import graph, models, ops, optim

    torch.manual_seed(0)
    model = models.MADE(D, [HIDDEN], n_masks=1).to(dev)
    opt = optim.FlatAdam(model.parameters(), lr=1e-3)
    x = batch(n, dev)
    step = graph.GraphedTrainStep(model, opt, lambda xx, preds: ops.bce_with_logits_sum_mean(preds, xx), x)
    return lambda: step()


def eager_reference_step(n, dev):
    """The reference's made.py step in eager torch (masks as the reference's float buffers)."""
    torch.manual_seed(0)
    layers = [torch.nn.Linear(D, HIDDEN).to(dev), torch.nn.Linear(HIDDEN, D).to(dev)]
    masks = [(torch.rand(HIDDEN, D, device=dev) < 0.5).float(), (torch.rand(D, HIDDEN, device=dev) < 0.5).float()]
    params = [p for layer in layers for p in layer.parameters()]
    opt = torch.optim.Adam(params)
    x = batch(n, dev)

    def f():
        opt.zero_grad()
        h = x.view(n, -1)
        for i, (layer, m) in enumerate(zip(layers, masks)):
            layer.weight.data *= m
            h = F.linear(h, layer.weight, layer.bias)
            if i == 0:
                h = torch.relu(h)
        loss = F.binary_cross_entropy_with_logits(h, x.view(n, -1), reduction="none").sum(dim=1).mean()
        loss.backward()
        opt.step()

    return f


def gemm_bytes(n):
    w = 4 * D * HIDDEN
    return {"forward": 2 * w + 4 * n * (D + HIDDEN + HIDDEN + D), "data_grad": w + 4 * n * (D + 2 * HIDDEN),
            "weight_grad": 2 * w + 4 * n * (D + HIDDEN + HIDDEN + D)}


def profile(n, iters):
    """Per-kernel times of the graphed step from rocprofv3 (child process)."""
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "made", "--",
               sys.executable, os.path.abspath(__file__), "--child", str(n), "--iters", str(iters)]
        res = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        if res.returncode != 0:
            return {"error": f"rocprofv3 exit {res.returncode}: {res.stderr[-400:]}"}
        files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
        if not files:
            return {"error": "no kernel_stats.csv written"}
        rows = []
        with open(files[0]) as f:
            for r in csv.DictReader(f):
                calls = int(r["Calls"])
                total_ns = float(r["TotalDurationNs"])
                rows.append({"kernel": r["Name"][:120], "calls": calls, "per_step_us": total_ns / 1e3 / (iters + 12),
                             "avg_us": total_ns / 1e3 / max(calls, 1)})
        rows.sort(key=lambda r: -r["per_step_us"])
        return {"steps_profiled": iters + 12, "rows": rows[:16]}


def child(n, iters):
    f = graphed_step(n, torch.device("cuda:0"))
    for _ in range(10 + iters):  # 10 warm-up replays (+ the 2 warm-up steps of the capture)
        f()
    torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "made.json"))
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--no-prof", action="store_true")
    ap.add_argument("--child", type=int, default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "made_bench needs the MI355X"
    if a.child is not None:
        child(a.child, a.iters)
        return
    dev = torch.device("cuda:0")
    rows = []
    for n in (64, 1024):
        row = {"N": n, "D": D, "hidden": [HIDDEN], "parameters": 2 * D * HIDDEN + HIDDEN + D,
               "graphed_step_ms": timed(graphed_step(n, dev), a.iters, a.warmup)}
        torch.cuda.empty_cache()
        row["eager_torch_reference_ms"] = timed(eager_reference_step(n, dev), a.iters, a.warmup)
        row["speedup_vs_eager_torch"] = row["eager_torch_reference_ms"] / row["graphed_step_ms"]
        row["gemm_algorithmic_bytes"] = gemm_bytes(n)
        torch.cuda.empty_cache()
        if not a.no_prof:
            row["kernels"] = profile(n, a.iters)
        print(json.dumps({k: v for k, v in row.items() if k != "kernels"}), flush=True)
        rows.append(row)
    rec = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "iters": a.iters, "warmup": a.warmup,
           "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
    print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
