"""Conditioning an ImageGPT prior on a coarser code image (ops.code_upsample, csrc/code_up.hip: nn.CodeUpsample,
ImageGPT.set_condition) on the MI355X.

usage: python tools/code_cond_bench.py [--out profiles/code_cond.json] [--min-seconds 0.5] [--only stem|step|sample]

One process. Timed figures of (a) and (b) are hipGraphs, warmed up, replayed at least 20 times and for at least
`--min-seconds`; the two sides alternate, window by window, in the same run; median of 5 windows (helpers of
tools/linear_categorical_bench.py).

(a) `stem`: the conditioned stem, base + lookup, forward + backward (weight gradient; `base` takes none on either side), per
    shape (N, K, Cout, h x w -> H x W, f = 2). `fused` is ops.code_upsample. `composed` is the route that exists without
    code_up.hip: ops.code_conv2d with a 1 x 1 kernel over Cout f^2 channels (its weight is the same table, laid out
    (Cout f^2, K, 1, 1)), F.pixel_shuffle, the add — it writes a (N, Cout f^2, h, w) intermediate and reads it back. A
    graph holds one forward + backward per buffer set (code image, base, output gradient), with enough sets that 512 MiB of
    the side's algorithmic traffic pass between two uses of a set. Algorithmic bytes, P = N H W, Wt = K Cout f^2:
    fused 4 (P / f^2 + 3 P Cout + 4 Wt)  (levels, base in, out, dY in; the table packed and read, dW written, weight read);
    composed 4 (2 P / f^2 + 7 P Cout + 4 Wt)  (+ the intermediate written and read in both directions).
    Time and the side's peak memory while capturing are recorded; no ratio is promised and no route is derived.
(b) `step`: the graphed training step (graph.GraphedTrainStep) of reproduce_priors' bottom prior (K = 512, 8 blocks, 2 heads,
    64 channels, CodeUpsample(512, 64, 2)) at batch 128 on 16 x 16 codes next to the same model without `_cond`: images / s
    and peak memory. The difference is the cost of conditioning.
(c) `sample`: whole VectorQuantizedVAE2.sample(n) calls, n = 1 / 16 / 64, for the recipe's VQ-VAE-2 (32 x 32 images: 8 x 8
    top and 16 x 16 bottom codes) with untrained priors of the recipe's size, on the cached route and with
    incremental=False on both priors; wall clock around a device synchronise, median of 3."""

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

STEM_SHAPES = [(128, 512, 64, 8, 8, 2), (64, 512, 64, 16, 16, 2)]  # (N, K, Cout, h, w, f)
K_PRIOR = 512


def stem_row(shape, dev, min_seconds):
    from pytorch_generative_amd import nn as pg_nn
    from pytorch_generative_amd import ops

    n, k, cout, h, w, f = shape
    P, wt = n * h * w * f * f, k * cout * f * f
    nbytes = {"fused": 4 * (P // (f * f) + 3 * P * cout + 4 * wt), "composed": 4 * (2 * P // (f * f) + 7 * P * cout + 4 * wt)}
    sets = {r: min(MAX_SETS, max(1, -(-ROTATE_BYTES // b))) for r, b in nbytes.items()}
    torch.manual_seed(n + k + cout)
    up = pg_nn.CodeUpsample(k, cout, f).to(dev)
    with torch.no_grad():
        up.weight.normal_()
    conv = pg_nn.Conv2d(k, cout * f * f, kernel_size=1, bias=False).to(dev)
    with torch.no_grad():  # the same table: w1x1[co f^2 + a f + b, k] = w[k, co, a, b] (pixel_shuffle's channel order)
        conv.weight.copy_(up.weight.permute(1, 2, 3, 0).reshape(cout * f * f, k, 1, 1))
    g = torch.Generator().manual_seed(1)
    m = max(sets.values())
    lev = [ops.codes_to_levels(torch.randint(0, k, (n, 1, h, w), generator=g), k).to(dev) for _ in range(m)]
    bases = [torch.randn(n, cout, h * f, w * f, generator=g).to(dev) for _ in range(m)]
    dys = [torch.randn(n, cout, h * f, w * f, generator=g).to(dev) for _ in range(m)]

    def run(name, j):
        if name == "fused":
            return up(lev[j], base=bases[j])
        return bases[j] + F.pixel_shuffle(conv.forward_codes(lev[j], k), f)

    def route(name, backward=True):
        def fn():
            for j in range(sets[name]):
                up.weight.grad = conv.weight.grad = None
                y = run(name, j)
                if backward:
                    y.backward(dys[j])
        return fn

    a, b = run("fused", 0), run("composed", 0)  # the two sides compute the same numbers: recorded next to the timings
    rel = float((a - b).abs().max() / a.abs().max())
    a.backward(dys[0])
    b.backward(dys[0])
    grel = float((up.weight.grad.permute(1, 2, 3, 0).reshape(conv.weight.shape) - conv.weight.grad).abs().max()
                 / up.weight.grad.abs().max())
    del a, b
    fns, peaks = {}, {}
    for name in ("fused", "composed"):
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        fns[name] = graph_of(route(name))
        peaks[name] = torch.cuda.max_memory_allocated() - base
    fns["fused_forward_only"] = graph_of(route("fused", backward=False))
    med, spread, replays = alternate(fns, min_seconds)
    row = {"shape_N_K_Cout_h_w_f": list(shape), "fused_vs_composed_output_rel_diff": rel,
           "fused_vs_composed_weight_grad_rel_diff": grel, "wgrad_plan_max_chunks_items": list(ops.code_up_plan(n, k, h, w))}
    for name in ("fused", "composed"):
        ms = med[name] / sets[name]
        row[name] = {"ms": ms, "min_max_ms": [v / sets[name] for v in spread[name]], "buffer_sets": sets[name],
                     "graph_replays": replays[name], "algorithmic_bytes": nbytes[name],
                     "bytes_per_s": nbytes[name] / (ms * 1e-3), "peak_bytes_over_inputs_while_capturing": peaks[name]}
    fwd = med["fused_forward_only"] / sets["fused"]
    row["fused"]["forward_only_ms"] = fwd
    row["fused"]["wgrad_share"] = 1.0 - fwd / row["fused"]["ms"]
    row["fused_speedup"] = row["composed"]["ms"] / row["fused"]["ms"]
    row["fused_is_slower"] = row["fused"]["ms"] > row["composed"]["ms"]
    return row


def _prior(in_size, dev, cond, sample_fn=None):
    from pytorch_generative_amd import models
    from pytorch_generative_amd import nn as pg_nn

    torch.manual_seed(0)
    model = models.ImageGPT(in_channels=K_PRIOR, out_channels=K_PRIOR, in_size=in_size, n_transformer_blocks=8,
                            n_attention_heads=2, n_embedding_channels=64, sample_fn=sample_fn)
    model.input_codes = K_PRIOR
    if cond:
        model.set_condition(pg_nn.CodeUpsample(K_PRIOR, 64, 2))
        with torch.no_grad():
            model._cond.weight.normal_(0, 0.1)
    return model.to(dev)


def step_row(dev, batch, min_seconds, in_size=16):
    from pytorch_generative_amd import graph, ops, optim

    k = K_PRIOR
    g = torch.Generator().manual_seed(in_size)
    levels = ops.codes_to_levels(torch.randint(0, k, (batch, 1, in_size, in_size), generator=g), k).to(dev)
    top = ops.codes_to_levels(torch.randint(0, k, (batch, 1, in_size // 2, in_size // 2), generator=g), k).to(dev)
    steps, mem = {}, {}
    for name in ("unconditional", "conditional"):
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()  # the other side's model and graph stay alive for the alternating windows
        model = _prior(in_size, dev, cond=name == "conditional")
        opt = optim.FlatAdam(model.parameters(), lr=5e-3)
        if name == "conditional":
            fwd = lambda x, y, model=model: ops.categorical_nll_sum_mean(model(x, cond=y), x, k)  # noqa: E731
        else:
            fwd = lambda x, y, model=model: ops.categorical_nll_sum_mean(model(x), x, k)  # noqa: E731
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        step = graph.GraphedTrainStep(model, opt, None, levels, example_y=top, forward_fn=fwd)
        step()
        torch.cuda.synchronize()
        mem[name], steps[name] = torch.cuda.max_memory_allocated() - base, step
    med, spread, replays = alternate({key: (lambda s=s: s()) for key, s in steps.items()}, min_seconds)
    row = {"model": f"ImageGPT(K={k}, in_size={in_size}, 8 blocks, 2 heads, 64 channels), CodeUpsample({k}, 64, 2)",
           "batch": batch}
    for name in steps:
        row[name] = {"step_ms": med[name], "min_max_ms": spread[name], "graph_replays": replays[name],
                     "images_per_s": batch / (med[name] * 1e-3), "peak_bytes_of_the_side": mem[name]}
    row["conditioning_cost_ms"] = med["conditional"] - med["unconditional"]
    row["conditioning_cost_fraction"] = med["conditional"] / med["unconditional"] - 1.0
    row["conditioning_cost_peak_bytes"] = mem["conditional"] - mem["unconditional"]
    return row


def sample_rows(dev, counts=(1, 16, 64)):
    from pytorch_generative_amd import models
    from pytorch_generative_amd import nn as pg_nn

    torch.manual_seed(0)
    vq = models.VectorQuantizedVAE2(in_channels=3, out_channels=3, hidden_channels=128, n_residual_blocks=2,
                                    residual_channels=64, n_embeddings=K_PRIOR, embedding_dim=64).to(dev).eval()
    x = torch.rand(2, 3, 32, 32, device=dev)
    with torch.no_grad():
        vq(x)  # registers the image shape
    top, bottom = vq.encode_codes(x)
    gen = torch.Generator(device=dev).manual_seed(0)
    priors = [_prior(top.shape[2], dev, False, pg_nn.CategoricalSampler(K_PRIOR, generator=gen)),
              _prior(bottom.shape[2], dev, True, pg_nn.CategoricalSampler(K_PRIOR, generator=gen))]
    with torch.no_grad():
        priors[0](top)
        priors[1](bottom, cond=top)
    vq.set_priors(*priors)
    vq._sample_fn = lambda out: out

    def full(n):  # the same call with a full forward per position on both priors
        t = priors[0].sample(n, incremental=False)
        return vq.decode_codes(t, priors[1].sample(cond=t, incremental=False))

    rows = []
    for n in counts:
        row = {"model": "VectorQuantizedVAE2 of the recipe (32 x 32 images, 8 x 8 top and 16 x 16 bottom codes), priors of "
                        "reproduce_priors' size, untrained", "n_samples": n}
        for name, fn in (("cached", lambda n=n: vq.sample(n)), ("full_forward_per_position", lambda n=n: full(n))):
            fn()  # warm-up
            torch.cuda.synchronize()
            ts = []
            for _ in range(3):
                t0 = time.perf_counter()
                out = fn()
                torch.cuda.synchronize()
                ts.append(time.perf_counter() - t0)
            assert out.shape == (n, 3, 32, 32) and bool(torch.isfinite(out).all())
            row[name] = {"seconds_median_of_3": sorted(ts)[1], "seconds_min_max": [min(ts), max(ts)]}
            if name == "cached":
                row["routes_top_bottom"] = [p._sample_route for p in priors]
        row["cached_speedup"] = row["full_forward_per_position"]["seconds_median_of_3"] / row["cached"]["seconds_median_of_3"]
        rows.append(row)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "code_cond.json"))
    ap.add_argument("--min-seconds", type=float, default=0.5)
    ap.add_argument("--only", choices=["stem", "step", "sample"], default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "code_cond_bench needs the MI355X"
    dev = torch.device("cuda:0")
    t0 = time.time()
    rec = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "min_seconds_per_figure": a.min_seconds,
           "rotate_bytes": ROTATE_BYTES, "stem": [], "step": [], "sample": []}

    def emit(key, row):
        print(json.dumps(row), flush=True)
        rec[key].append(row)
        torch.cuda.empty_cache()

    if a.only in (None, "stem"):
        for shape in STEM_SHAPES:
            emit("stem", stem_row(shape, dev, a.min_seconds))
    if a.only in (None, "step"):
        emit("step", step_row(dev, 128, a.min_seconds))
    if a.only in (None, "sample"):
        for row in sample_rows(dev):
            emit("sample", row)
    for key in ("stem", "step", "sample"):
        if not rec[key]:
            rec[key] = {"status": "NOT YET MEASURED", "how": "tools/code_cond_bench.py"}
    rec["seconds"] = time.time() - t0
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
