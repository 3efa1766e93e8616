"""The output head fused into the categorical likelihood (ops.DeferredLogits, csrc/linear_categorical.hip) next to the dense
route (the 1x1 convolution writes the logits, the categorical kernels read them) on the MI355X.

usage: python tools/linear_categorical_bench.py [--out profiles/linear_categorical.json] [--min-seconds 0.5] [--no-model]

One process. Every figure is a hipGraph of forward + backward, warmed up, replayed at least 20 times and for at least
`--min-seconds`. The two routes alternate, window by window, in the same run.

(a) `head_and_loss`: the head and the loss alone, per shape (N, Cin, K, C, H, W, transform). A graph holds one forward +
    backward per buffer set (features, images and, on the dense route, what autograd allocates), with enough sets that 512 MiB
    of the route's algorithmic traffic pass between two uses of a set: memory rates, not Infinity Cache rates. `ms` is per
    forward + backward. Each record carries the algorithmic FLOP and bytes of both routes, computed from the shape:
      dense  FLOP 3 * 2 P KC Cin (logits, dW, dh);   bytes 4 * (5 P KC + 3 P Cin + 2 KC Cin + 5 S)
      fused  FLOP 4 * 2 P KC Cin (logits recomputed); bytes 4 * (3 P Cin + 5 S + 2 rows * row_len + KC Cin)
    with P = N H W pixels, KC = K C, S = N C H W sub-pixels (image, two lse planes written and read).
(b) `image_gpt_step`: a whole training step (graph.GraphedTrainStep) of the benchmark's ImageGPT with out_channels = 256 at
    batch 1024 and 64, defer_head off and on: images / s and torch.cuda.max_memory_allocated.
No routing threshold is derived from this: defer_head is the user's switch. `fused_is_slower` marks the shapes where it loses."""

import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pytorch-generative_amd"))
import torch  # noqa: E402

SHAPES = [(1024, 16, 256, 1, 28, 28, "ln"), (64, 16, 256, 1, 28, 28, "ln"), (256, 32, 256, 1, 28, 28, "relu"),
          (128, 64, 256, 1, 28, 28, "none"), (64, 64, 256, 3, 32, 32, "ln")]
ROTATE_BYTES = 512 << 20  # streamed between two uses of a buffer set: twice the Infinity Cache
MAX_SETS = 16


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


def window_ms(fn, replays):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(replays):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / replays


def alternate(fns, min_seconds, windows=5):
    """The callables in turn, window after window; per callable at least 20 replays and `min_seconds` in all. Returns the
    medians (ms per call), (min, max) and the replays per callable."""
    for fn in fns.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    per = {k: max(4, int(min_seconds * 1e3 / windows / max(window_ms(fn, 3), 1e-3)) + 1) for k, fn in fns.items()}
    ts = {k: [] for k in fns}
    for _ in range(windows):
        for k, fn in fns.items():
            ts[k].append(window_ms(fn, per[k]))
    return ({k: statistics.median(v) for k, v in ts.items()}, {k: [min(v), max(v)] for k, v in ts.items()},
            {k: per[k] * windows for k in fns})


def counts(n, cin, k, c, h, w):
    from pytorch_generative_amd import _lib

    P, KC, S = n * h * w, k * c, n * c * h * w
    ppt, rows, lds = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    ws = ctypes.c_size_t()
    _lib.check(_lib.load().pg_linear_categorical_plan(n, c, k, cin, h * w, 0, ctypes.byref(ppt), ctypes.byref(rows),
                                                      ctypes.byref(lds), ctypes.byref(ws)), "pg_linear_categorical_plan")
    gemm = 2 * P * KC * cin
    return {"dense": {"flop": 3 * gemm, "bytes": 4 * (5 * P * KC + 3 * P * cin + 2 * KC * cin + 5 * S)},
            "fused": {"flop": 4 * gemm, "bytes": 4 * (3 * P * cin + 5 * S + 2 * ws.value + KC * cin)},
            "plan": {"pixels_per_tile": ppt.value, "rows": rows.value, "lds_bytes": lds.value, "workspace_floats": ws.value},
            "logits_bytes": 4 * P * KC}


def head_row(shape, dev, min_seconds):
    from pytorch_generative_amd import nn as pg_nn
    from pytorch_generative_amd import ops

    n, cin, k, c, h, w, transform = shape
    cnt = counts(n, cin, k, c, h, w)
    torch.manual_seed(n + cin + k)
    conv = pg_nn.Conv2d(in_channels=cin, out_channels=k * c, kernel_size=1).to(dev)
    ln = pg_nn.NCHWLayerNorm(cin).to(dev) if transform == "ln" else None
    in_act = "relu" if transform == "relu" else None
    sets = {r: min(MAX_SETS, max(1, -(-ROTATE_BYTES // cnt[r]["bytes"]))) for r in ("dense", "fused")}
    g = torch.Generator().manual_seed(1)
    hs = [torch.randn(n, cin, h, w, generator=g).to(dev).requires_grad_(True) for _ in range(max(sets.values()))]
    xs = [(torch.randint(0, k, (n, c, h, w), generator=g).float() / (k - 1)).to(dev) for _ in range(max(sets.values()))]

    def route(dense):
        def fn():
            for hh, xx in list(zip(hs, xs))[:sets["dense" if dense else "fused"]]:
                hh.grad = None
                d = ops.DeferredLogits(hh, conv, in_act=in_act, pre_ln=ln)
                ops.categorical_nll_sum_mean(d.dense() if dense else d, xx, k).backward()
        return fn

    assert ops.linear_categorical_supported(hs[0], conv, in_act, ln)
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fns = {}
    peaks = {}
    for name, dense in (("dense", True), ("fused", False)):
        torch.cuda.reset_peak_memory_stats()
        fns[name] = graph_of(route(dense))
        peaks[name] = torch.cuda.max_memory_allocated() - base
    med, spread, replays = alternate(fns, min_seconds)
    row = {"shape_N_Cin_K_C_H_W_transform": list(shape), **{key: cnt[key] for key in ("plan", "logits_bytes")}}
    for name in ("dense", "fused"):
        ms = med[name] / sets[name]
        row[name] = {"ms": ms, "min_max_ms": [v / sets[name] for v in spread[name]], "buffer_sets": sets[name],
                     "graph_replays": replays[name], "algorithmic_flop": cnt[name]["flop"],
                     "algorithmic_bytes": cnt[name]["bytes"], "flop_per_s": cnt[name]["flop"] / (ms * 1e-3),
                     "bytes_per_s": cnt[name]["bytes"] / (ms * 1e-3), "peak_bytes_over_inputs_while_capturing": peaks[name]}
    row["fused_speedup"] = row["dense"]["ms"] / row["fused"]["ms"]
    row["fused_is_slower"] = row["fused"]["ms"] > row["dense"]["ms"]
    return row


def step_rows(dev, batch, min_seconds):
    """The benchmark's ImageGPT with a 256-way head: the graphed training step with defer_head off and on."""
    from pytorch_generative_amd import graph, models, optim, recipes

    k = 256
    g = torch.Generator().manual_seed(batch)
    images = (torch.randint(0, k, (batch, 1, 28, 28), generator=g).float() / (k - 1)).to(dev)
    loss3 = recipes.categorical_loss(k)
    steps, mem = {}, {}
    for defer in (False, True):
        torch.manual_seed(0)
        model = models.ImageGPT(in_channels=1, out_channels=k, in_size=28, n_transformer_blocks=8, n_attention_heads=4,
                                n_embedding_channels=16).to(dev)
        model.defer_head = defer
        opt = optim.FlatAdam(model.parameters(), lr=5e-3)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        step = graph.GraphedTrainStep(model, opt, lambda x, preds: loss3(x, None, preds), images)
        step()
        torch.cuda.synchronize()
        name = "defer_head_on" if defer else "defer_head_off"
        mem[name] = torch.cuda.max_memory_allocated()
        steps[name] = step
    med, spread, replays = alternate({key: (lambda s=s: s()) for key, s in steps.items()}, min_seconds)
    row = {"model": "ImageGPT(out_channels=256, 8 blocks, 4 heads, 16 channels)", "batch": batch}
    for name in steps:
        row[name] = {"step_ms": med[name], "min_max_ms": spread[name], "graph_replays": replays[name],
                     "images_per_s": batch / (med[name] * 1e-3), "max_memory_allocated": mem[name]}
    row["step_speedup"] = med["defer_head_off"] / med["defer_head_on"]
    row["fused_is_slower"] = med["defer_head_on"] > med["defer_head_off"]
    del steps
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "linear_categorical.json"))
    ap.add_argument("--min-seconds", type=float, default=0.5)
    ap.add_argument("--no-model", action="store_true")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "linear_categorical_bench needs the MI355X"
    dev = torch.device("cuda:0")
    t0 = time.time()
    rec = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "min_seconds_per_figure": a.min_seconds,
           "rotate_bytes": ROTATE_BYTES, "head_and_loss": [], "image_gpt_step": []}
    for shape in SHAPES:
        row = head_row(shape, dev, a.min_seconds)
        print(json.dumps(row), flush=True)
        rec["head_and_loss"].append(row)
        torch.cuda.empty_cache()
    if not a.no_model:
        for batch in (1024, 64):
            row = step_rows(dev, batch, a.min_seconds)
            print(json.dumps(row), flush=True)
            rec["image_gpt_step"].append(row)
            torch.cuda.empty_cache()
    else:
        rec["image_gpt_step"] = {"status": "not measured", "how": "tools/linear_categorical_bench.py"}
    rec["seconds"] = time.time() - t0
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
