"""Categorical (K-way softmax) pixel likelihood on the MI355X: the loss kernels and the per-position draw.

usage: python tools/categorical_bench.py [--out profiles/categorical.json] [--rounds 7] [--window-ms 30]
                                         [--no-model | --model-only]

Per shape (N, K, C, H, W) = (64, 256, 1, 28, 28), (1024, 256, 1, 28, 28), (64, 256, 3, 32, 32):
* `graphed_fwd_bwd_ms`: ops.categorical_nll_sum_mean forward + backward (pg_fill of the scalar, pg_categorical_nll_fwd,
  the ATen fill of the upstream gradient, pg_categorical_nll_bwd) captured into one hipGraph, as a training step replays
  it. HIP events around a window of replays sized to `--window-ms`; median over `--rounds` rounds.
* `eager_torch_fwd_bwd_ms`: FOR COMPARISON ONLY, F.cross_entropy(logits.view(N, K, C, H, W), classes, reduction='none')
  .sum((1, 2, 3)).mean() and its backward in eager torch-ROCm on the same GPU. The two are timed alternately, round by
  round, each on ONE set of buffers: at the two batch-64 shapes the logits stay in the 256 MiB Infinity Cache from call
  to call, for both sides alike (in a training step the output head has just written them).
* `fwd` / `bwd`: the two loss launches alone, against the ALGORITHMIC traffic: forward 4 K bytes per sub-pixel for the
  logits plus image and the two lse planes, backward 8 K plus image and the two lse planes. So that the figures are
  memory and not cache rates, a graph holds one launch per buffer set and there are `buffer_sets` sets, enough that 512 MiB
  are streamed between two uses of a set; `ms` is per launch. `fraction_of_hbm_peak` divides by the 8 TB/s of the data
  sheet. Recorded, not gated.
* `sampler`: one ops.categorical_sample call at (64, 256) beside torch.softmax + torch.multinomial, eager, per call.
* `image_gpt_share`: the recipe's ImageGPT with a 256-way head at batch 1024 — the graphed training step, and the share
  of it that the loss forward + backward at that shape takes: what fusing the output head with the loss could save at
  most is the logits' round trip through memory inside that share. --no-model writes NOT YET MEASURED in its place,
  --model-only adds it to an existing file.
Acceptance: `not_slower_than_eager_torch` at every shape."""

import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pytorch-generative_amd"))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

SHAPES = [(64, 256, 1, 28, 28), (1024, 256, 1, 28, 28), (64, 256, 3, 32, 32)]
HBM_PEAK = 8.0e12  # bytes / s (MI355X data sheet)
ROTATE_BYTES = 512 << 20  # streamed between two uses of a buffer set: twice the Infinity Cache


def window_ms(fn, replays):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(replays):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / replays


def alternate(fns, rounds, window, warmup=3):
    """Times the callables round by round, one after the other in every round, each over a window of about `window` ms
    (at least 5 calls); returns the per-call medians (ms), their (min, max) and the calls per window."""
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    replays = {k: max(5, int(window / max(window_ms(fn, 5), 1e-4)) + 1) for k, fn in fns.items()}
    ts = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            ts[k].append(window_ms(fn, replays[k]))
    return ({k: statistics.median(v) for k, v in ts.items()}, {k: [min(v), max(v)] for k, v in ts.items()}, replays)


def graph_of(fn):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fn()
    return g.replay


def inputs(shape, dev):
    n, k, c, h, w = shape
    g = torch.Generator().manual_seed(n + k + c)
    logits = (torch.randn(n, k * c, h, w, generator=g) * 3).to(dev)
    classes = torch.randint(0, k, (n, c, h, w), generator=g)
    return logits, (classes.float() / (k - 1)).to(dev), classes.to(dev)


def loss_row(shape, dev, rounds, window):
    from pytorch_generative_amd import _lib, ops

    lib = _lib.load()
    n, k, c, h, w = shape
    logits, images, classes = inputs(shape, dev)
    z = logits.clone().requires_grad_(True)

    def ours():
        z.grad = None
        ops.categorical_nll_sum_mean(z, images, k).backward()

    zt = logits.clone().requires_grad_(True)

    def eager_torch():
        zt.grad = None
        F.cross_entropy(zt.view(n, k, c, h, w), classes, reduction="none").sum(dim=(1, 2, 3)).mean().backward()

    sub = n * c * h * w
    fwd_bytes, bwd_bytes = 4 * sub * (k + 3), 4 * sub * (2 * k + 3)
    fwd_sets, bwd_sets = -(-ROTATE_BYTES // fwd_bytes), -(-ROTATE_BYTES // bwd_bytes)
    zs = [logits] + [logits.clone() for _ in range(fwd_sets - 1)]
    xs = [images.clone() for _ in range(fwd_sets)]
    lses = [torch.empty((2,) + tuple(images.shape), device=dev) for _ in range(fwd_sets)]
    dzs = [torch.empty_like(logits) for _ in range(bwd_sets)]
    loss = torch.zeros(1, device=dev)
    one = torch.ones(1, device=dev)
    st = lambda: torch.cuda.current_stream().cuda_stream  # noqa: E731

    def fwd():
        for zz, xx, ll in zip(zs, xs, lses):
            _lib.check(lib.pg_categorical_nll_fwd(zz.data_ptr(), xx.data_ptr(), ll.data_ptr(), None, loss.data_ptr(),
                                                  n, c, k, h * w, st()), "pg_categorical_nll_fwd")

    def bwd():  # reads the lse planes fwd() left
        for zz, xx, ll, dd in zip(zs, xs, lses, dzs):
            _lib.check(lib.pg_categorical_nll_bwd(zz.data_ptr(), xx.data_ptr(), ll.data_ptr(), one.data_ptr(),
                                                  dd.data_ptr(), n, c, k, h * w, st()), "pg_categorical_nll_bwd")

    fns = {"graphed_fwd_bwd_ms": graph_of(ours), "eager_torch_fwd_bwd_ms": eager_torch, "fwd": graph_of(fwd),
           "bwd": graph_of(bwd)}
    med, spread, replays = alternate(fns, rounds, window)
    fwd_ms, bwd_ms = med.pop("fwd") / fwd_sets, med.pop("bwd") / bwd_sets
    # same results before the times mean anything
    ours()
    eager_torch()
    torch.cuda.synchronize()
    err = float((z.grad - zt.grad).abs().max() / zt.grad.abs().max())
    import ctypes

    lanes, vec = ctypes.c_int(), ctypes.c_int()
    lib.pg_categorical_plan(n, c, k, h * w, ctypes.byref(lanes), ctypes.byref(vec))
    row = {"shape_N_K_C_H_W": list(shape), "plan": {"lanes_per_pixel": lanes.value, "vec": vec.value}, **med,
           "min_max_ms": {key: spread[key] for key in med}, "calls_per_window": replays,
           "grad_max_norm_diff_vs_torch": err,
           "speedup_vs_eager_torch": med["eager_torch_fwd_bwd_ms"] / med["graphed_fwd_bwd_ms"],
           "not_slower_than_eager_torch": med["graphed_fwd_bwd_ms"] <= med["eager_torch_fwd_bwd_ms"],
           "fwd": {"ms": fwd_ms, "buffer_sets": fwd_sets, "algorithmic_bytes": fwd_bytes,
                   "bytes_per_s": fwd_bytes / (fwd_ms * 1e-3), "fraction_of_hbm_peak": fwd_bytes / (fwd_ms * 1e-3) / HBM_PEAK},
           "bwd": {"ms": bwd_ms, "buffer_sets": bwd_sets, "algorithmic_bytes": bwd_bytes,
                   "bytes_per_s": bwd_bytes / (bwd_ms * 1e-3), "fraction_of_hbm_peak": bwd_bytes / (bwd_ms * 1e-3) / HBM_PEAK}}
    return row


def sampler_row(dev, rounds, window):
    from pytorch_generative_amd import ops

    n, k = 64, 256
    g = torch.Generator().manual_seed(1)
    logits = (torch.randn(n, k, generator=g) * 3).to(dev)
    u = torch.rand(n, 1, generator=g).to(dev)
    fns = {"categorical_sample_us": lambda: ops.categorical_sample(logits, u, k),
           "torch_softmax_multinomial_us": lambda: torch.multinomial(torch.softmax(logits, dim=1), 1).float() / (k - 1)}
    med, spread, _ = alternate(fns, rounds, window)
    return {"N": n, "K": k, **{key: v * 1e3 for key, v in med.items()},
            "min_max_us": {key: [a * 1e3, b * 1e3] for key, (a, b) in spread.items()},
            "note": "eager calls, host launch cost included on both sides"}


def model_row(dev, rounds, loss_ms):
    """The recipe's ImageGPT with a 256-way head at batch 1024: the graphed step and the loss's share of it."""
    from pytorch_generative_amd import graph, models, optim, recipes

    n, k = 1024, 256
    torch.manual_seed(0)
    model = models.ImageGPT(in_channels=1, out_channels=k, in_size=28, n_transformer_blocks=8, n_attention_heads=2,
                            n_embedding_channels=64).to(dev)
    opt = optim.FlatAdam(model.parameters(), lr=5e-3)
    _, images, _ = inputs((n, k, 1, 28, 28), dev)
    loss3 = recipes.categorical_loss(k)
    step = graph.GraphedTrainStep(model, opt, lambda x, preds: loss3(x, None, preds), images)
    med, spread, _ = alternate({"graphed_step_ms": lambda: step()}, rounds, 30.0, warmup=2)
    return {"model": "ImageGPT(out_channels=256, 8 blocks, 2 heads, 64 channels)", "N": n, **med, "min_max_ms": spread,
            "loss_fwd_bwd_ms": loss_ms, "loss_share_of_step": loss_ms / med["graphed_step_ms"],
            "logits_bytes": 4 * n * k * 784}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "categorical.json"))
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--window-ms", type=float, default=30.0)
    ap.add_argument("--no-model", action="store_true")
    ap.add_argument("--model-only", action="store_true")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "categorical_bench needs the MI355X"
    dev = torch.device("cuda:0")
    if a.model_only:
        with open(a.out) as f:
            rec = json.load(f)
        rec["image_gpt_share"] = model_row(dev, a.rounds, rec["rows"][1]["graphed_fwd_bwd_ms"])
        print(json.dumps(rec["image_gpt_share"]), flush=True)
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")
        print(f"wrote {a.out}")
        return
    rows = []
    for shape in SHAPES:
        row = loss_row(shape, dev, a.rounds, a.window_ms)
        print(json.dumps(row), flush=True)
        rows.append(row)
        torch.cuda.empty_cache()
    rec = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "rounds": a.rounds, "window_ms": a.window_ms,
           "hbm_peak_bytes_per_s": HBM_PEAK, "rows": rows, "sampler": sampler_row(dev, a.rounds, a.window_ms)}
    print(json.dumps(rec["sampler"]), flush=True)
    if not a.no_model:
        try:
            rec["image_gpt_share"] = model_row(dev, a.rounds, rows[1]["graphed_fwd_bwd_ms"])
        except Exception as e:  # noqa: BLE001 — the share is a by-product: record why it is missing
            rec["image_gpt_share"] = {"error": f"{type(e).__name__}: {e}"[:400]}
        print(json.dumps(rec["image_gpt_share"]), flush=True)
    else:
        rec["image_gpt_share"] = {"status": "NOT YET MEASURED", "how": "tools/categorical_bench.py --model-only"}
    rec["not_slower_than_eager_torch_at_every_shape"] = all(r["not_slower_than_eager_torch"] for r in rows)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
