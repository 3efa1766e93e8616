"""The code-index stem (ops.code_conv2d, csrc/code_conv.hip: `input_codes`) next to the dense route (F.one_hot + the masked
convolution over K input channels) on the MI355X.

usage: python tools/code_prior_bench.py [--out profiles/code_prior.json] [--min-seconds 0.5] [--only stem|step|sample]

One process. Timed figures are hipGraphs, warmed up, replayed at least 20 times and for at least `--min-seconds`; the two
routes alternate, window by window, in the same run (helpers of tools/linear_categorical_bench.py).

(a) `stem`: CausalConv2d(mask A, K -> Cout) forward + backward (weight and bias gradient; the input takes none on either
    route), per shape (N, K, Cout, H, W, kernel). The dense route starts from the int64 indices and includes F.one_hot, the
    layout change and the float conversion: its construction is part of what it costs. It uses only operators that exist
    without this change. A graph holds one forward + backward per buffer set (code image, output gradient), with enough
    sets that 512 MiB of the route's algorithmic traffic pass between two uses of a set. Algorithmic bytes, from the shape,
    with P = N H W, T = kernel taps:  dense 4 (3 P K + 3 P Cout + 3 K Cout T);  code 4 (2 P + 3 P Cout + 4 K Cout T).
    `wgrad_share` is the code route's backward alone over its forward + backward.
(b) `step`: the whole graphed training step (graph.GraphedTrainStep) of reproduce_prior's ImageGPT (K = 512, 8 blocks,
    2 heads, 64 channels) at batch 128 on 8 x 8 and 32 x 32 code images: images / s and the route's own peak memory
    (torch.cuda.max_memory_allocated over what was allocated before its model was built),
    `input_codes` on, and off with the one-hot tensor built inside the step.
(c) `sample`: one sample(64) of a prior over 8 x 8 code images, incremental and incremental=False, wall clock around a
    device synchronise: the recipe's 64-channel model (K/V-cached on the one-launch step kernel, ops.gpt_decode_step;
    tools/gpt_decode_bench.py measures it at more shapes) and a 16-channel, 4-head one (K/V-cached on the block kernels),
    both with pg_sample_embed_codes.
No routing threshold is derived from this: input_codes is the user's switch. `code_is_slower` marks the shapes where it loses."""

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pytorch-generative_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from linear_categorical_bench import MAX_SETS, ROTATE_BYTES, alternate, graph_of  # noqa: E402

STEM_SHAPES = [(128, 512, 64, 8, 8, 3), (64, 512, 64, 32, 32, 3), (128, 512, 256, 8, 8, 7)]
K_PRIOR = 512


def one_hot(idx, k):
    """(N, 1, H, W) int64 -> (N, K, H, W) float32, dense."""
    return F.one_hot(idx[:, 0], k).permute(0, 3, 1, 2).float().contiguous()


def stem_row(shape, dev, min_seconds):
    from pytorch_generative_amd import nn as pg_nn
    from pytorch_generative_amd import ops

    n, k, cout, h, w, ks = shape
    P, T = n * h * w, ks * ks
    nbytes = {"dense": 4 * (3 * P * k + 3 * P * cout + 3 * k * cout * T), "code": 4 * (2 * P + 3 * P * cout + 4 * k * cout * T)}
    sets = {r: min(MAX_SETS, max(1, -(-ROTATE_BYTES // b))) for r, b in nbytes.items()}
    torch.manual_seed(n + k + cout)
    conv = pg_nn.CausalConv2d(True, in_channels=k, out_channels=cout, kernel_size=ks, padding=ks // 2).to(dev)
    g = torch.Generator().manual_seed(1)
    m = max(sets.values())
    idx = [torch.randint(0, k, (n, 1, h, w), generator=g).to(dev) for _ in range(m)]
    lev = [ops.codes_to_levels(i, k) for i in idx]
    dys = [torch.randn(n, cout, h, w, generator=g).to(dev) for _ in range(m)]

    def route(name, backward=True):
        def fn():
            for j in range(sets["dense" if name == "dense" else "code"]):
                conv.weight.grad = conv.bias.grad = None
                y = conv(one_hot(idx[j], k)) if name == "dense" else conv.forward_codes(lev[j], k)
                if backward:
                    y.backward(dys[j])
        return fn

    with torch.no_grad():  # the two routes compute the same numbers: recorded next to the timings
        a, b = conv(one_hot(idx[0], k)), conv.forward_codes(lev[0], k)
        rel = float((a - b).abs().max() / a.abs().max())
    fns, peaks = {}, {}
    base = torch.cuda.memory_allocated()
    for name in ("dense", "code"):
        torch.cuda.reset_peak_memory_stats()
        fns[name] = graph_of(route(name))
        peaks[name] = torch.cuda.max_memory_allocated() - base
    fns["code_forward_only"] = graph_of(route("code", backward=False))
    med, spread, replays = alternate(fns, min_seconds)
    row = {"shape_N_K_Cout_H_W_kernel": list(shape), "code_vs_dense_output_rel_diff": rel,
           "wgrad_plan_max_chunks_items": list(ops.code_conv_wgrad_plan(n, k, h, w))}
    for name in ("dense", "code"):
        ms = med[name] / sets[name]
        row[name] = {"ms": ms, "min_max_ms": [v / sets[name] for v in spread[name]], "buffer_sets": sets[name],
                     "graph_replays": replays[name], "algorithmic_bytes": nbytes[name],
                     "bytes_per_s": nbytes[name] / (ms * 1e-3), "peak_bytes_over_inputs_while_capturing": peaks[name]}
    fwd = med["code_forward_only"] / sets["code"]
    row["code"]["forward_only_ms"] = fwd
    row["code"]["wgrad_share"] = 1.0 - fwd / row["code"]["ms"]
    row["code_speedup"] = row["dense"]["ms"] / row["code"]["ms"]
    row["code_is_slower"] = row["code"]["ms"] > row["dense"]["ms"]
    return row


def _prior(in_size, dev, channels=64, heads=2, codes=True, sample_fn=None):
    from pytorch_generative_amd import models

    torch.manual_seed(0)
    model = models.ImageGPT(in_channels=K_PRIOR, out_channels=K_PRIOR, in_size=in_size, n_transformer_blocks=8,
                            n_attention_heads=heads, n_embedding_channels=channels, sample_fn=sample_fn).to(dev)
    if codes:
        model.input_codes = K_PRIOR
    return model


def step_row(in_size, dev, batch, min_seconds):
    from pytorch_generative_amd import graph, ops, optim

    k = K_PRIOR
    g = torch.Generator().manual_seed(in_size)
    levels = ops.codes_to_levels(torch.randint(0, k, (batch, 1, in_size, in_size), generator=g), k).to(dev)
    steps, mem = {}, {}
    for name in ("dense", "code"):
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()  # the other route's model and graph stay alive for the alternating windows
        model = _prior(in_size, dev, codes=name == "code")
        opt = optim.FlatAdam(model.parameters(), lr=5e-3)
        if name == "code":
            fwd = lambda x, y, model=model: ops.categorical_nll_sum_mean(model(x), x, k)  # noqa: E731
        else:
            fwd = lambda x, y, model=model: ops.categorical_nll_sum_mean(  # noqa: E731
                model(one_hot(torch.round(x * (k - 1)).long(), k)), x, k)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        step = graph.GraphedTrainStep(model, opt, None, levels, forward_fn=fwd)
        step()
        torch.cuda.synchronize()
        mem[name], steps[name] = torch.cuda.max_memory_allocated() - base, step
    med, spread, replays = alternate({key: (lambda s=s: s()) for key, s in steps.items()}, min_seconds)
    row = {"model": f"ImageGPT(K={k}, in_size={in_size}, 8 blocks, 2 heads, 64 channels)", "batch": batch}
    for name in steps:
        row[name] = {"step_ms": med[name], "min_max_ms": spread[name], "graph_replays": replays[name],
                     "images_per_s": batch / (med[name] * 1e-3), "peak_bytes_of_the_route": mem[name]}
    row["code_speedup"] = med["dense"] / med["code"]
    row["code_is_slower"] = med["code"] > med["dense"]
    return row


def sample_row(dev, channels, heads, n=64, in_size=8):
    from pytorch_generative_amd import nn as pg_nn
    from pytorch_generative_amd import ops

    model = _prior(in_size, dev, channels=channels, heads=heads,
                   sample_fn=pg_nn.CategoricalSampler(K_PRIOR, generator=torch.Generator(device=dev).manual_seed(0)))
    with torch.no_grad():
        model(ops.codes_to_levels(torch.zeros(n, 1, in_size, in_size, dtype=torch.int64), K_PRIOR).to(dev))
    row = {"model": f"ImageGPT(K={K_PRIOR}, in_size={in_size}, 8 blocks, {heads} heads, {channels} channels)", "n_samples": n,
           "kv_cached_sampler_taken": bool(model._incremental_ok(n))}
    for name, inc in (("incremental", True), ("full_forward_per_position", False)):
        model.sample(n, incremental=inc)  # warm-up
        torch.cuda.synchronize()
        ts = []
        for _ in range(3):
            t0 = time.perf_counter()
            out = model.sample(n, incremental=inc)
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        assert out.shape == (n, 1, in_size, in_size) and bool((out >= 0).all())
        row[name] = {"seconds_median_of_3": sorted(ts)[1], "seconds_min_max": [min(ts), max(ts)]}
    row["incremental_speedup"] = row["full_forward_per_position"]["seconds_median_of_3"] / row["incremental"]["seconds_median_of_3"]
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "code_prior.json"))
    ap.add_argument("--min-seconds", type=float, default=0.5)
    ap.add_argument("--only", choices=["stem", "step", "sample"], default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "code_prior_bench needs the MI355X"
    dev = torch.device("cuda:0")
    t0 = time.time()
    rec = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "min_seconds_per_figure": a.min_seconds,
           "rotate_bytes": ROTATE_BYTES, "wgrad_algorithm": "store-and-sum over an inverted index",
           "stem": [], "step": [], "sample": []}

    def emit(key, row):
        print(json.dumps(row), flush=True)
        rec[key].append(row)
        torch.cuda.empty_cache()

    if a.only in (None, "stem"):
        for shape in STEM_SHAPES:
            emit("stem", stem_row(shape, dev, a.min_seconds))
    if a.only in (None, "step"):
        for in_size in (8, 32):
            emit("step", step_row(in_size, dev, 128, a.min_seconds))
    if a.only in (None, "sample"):
        for channels, heads in ((64, 2), (16, 4)):
            emit("sample", sample_row(dev, channels, heads))
    for key in ("stem", "step", "sample"):
        if not rec[key]:
            rec[key] = {"status": "not measured", "how": "tools/code_prior_bench.py"}
    rec["seconds"] = time.time() - t0
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
