"""PixelSNAIL sampling on the MI355X: the cached row attention (ops.attention_row, csrc/attention_row.hip) with the row step
captured into hipGraphs, against the row-cached sampler as it stood before (attention over the whole prefix, eager) and
against one full forward per pixel.

usage: python tools/pixelsnail_sample_bench.py [--out profiles/pixelsnail_sampling.json] [--repeats 5]
                                               [--models recipe benchmark] [--batches 1 16 64 256] [--full-pixels 8]

Models: `recipe` = models.autoregressive.pixel_snail.reproduce()'s (1 channel, 28 x 28), `benchmark` = bench.py's
pixel_snail workload (3 channels, 32 x 32); both 64 channels, 8 blocks, key 4 / value 32.

Routes, all through AutoregressiveModel.sample() with the row-cached sampler forced on (`_row_decode_min_batch = 1`):
(a) `prefix_eager`:   CausalAttention.row_attention = "prefix" — the parent's route: the training attention kernel over all rows
                      <= r per step, two prefix copies per attention layer; its capture is refused, so it runs eagerly;
(b) `decode_eager`:   the new kernel, `_row_graph = False`;
(c) `decode_graphed`: the new kernel, the row step captured (the default); model._row_step_captured is recorded;
(d) `full_forward`:   what sample() does below `_row_decode_min_batch`: one full forward per pixel. Not run whole: the loop
                      body of sample(incremental=False) is timed over the first k and the first 2k raster positions
                      (`--full-pixels` k); the per-pixel cost is the DIFFERENCE of the two, (t_2k - t_k) / k, and
                      `full_forward_s` is H W times it.
(a)-(c) are whole sample() calls, wall clock to a device synchronise, graph capture included. The variants of a row run in one
process and alternate within a round; one warm-up round, then `--repeats` (at least 5) timed rounds; medians are reported, all
timings kept. `row_step_replay_us` is one replay of the captured row step at the last row, over full caches."""

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pytorch-generative_amd"))
import torch  # noqa: E402

MODELS = {"recipe": (1, 28, 28), "benchmark": (3, 32, 32)}


def _model(dev, channels):
    from pytorch_generative_amd import models

    torch.manual_seed(0)
    model = models.PixelSNAIL(in_channels=channels, out_channels=channels, n_channels=64, n_pixel_snail_blocks=8,
                              n_residual_blocks=2, attention_key_channels=4, attention_value_channels=32).to(dev)
    model._row_decode_min_batch = 1  # every row route below is the row-cached sampler, whatever the routing constant says
    return model


def compare(variants, repeats):
    """{name: fn} -> {name: [seconds]}: one warm-up round, then `repeats` rounds, the variants alternating within a round."""
    times = {name: [] for name in variants}
    for rnd in range(repeats + 1):
        for name, fn in variants.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if rnd:
                times[name].append(time.perf_counter() - t0)
    return times


def full_forward_pixels(model, empty, k):
    """The loop body of sample(incremental=False) over the first k raster positions."""
    canvas = empty.clone()
    w = canvas.shape[3]
    with torch.no_grad():
        for p in range(k):
            row, col = divmod(p, w)
            model._draw_into(canvas, row, col, model.forward(canvas)[:, :, row, col])
    return canvas


def sample_row(model, what, n, shape, repeats, k):
    from pytorch_generative_amd import nn as pg_nn

    c, h, w = shape
    dev = next(model.parameters()).device
    empty = torch.full((n, c, h, w), -1.0, device=dev)
    captured = {}

    def call(name, route, graph):
        pg_nn.CausalAttention.row_attention = route
        model._row_graph = graph
        try:
            out = model.sample(conditioned_on=empty)
        finally:
            pg_nn.CausalAttention.row_attention = "decode"
            del model._row_graph
        captured[name] = bool(model._row_step_captured)
        assert out.shape == empty.shape and bool((out >= 0).all())

    variants = {
        "prefix_eager": lambda: call("prefix_eager", "prefix", True),  # the capture is tried and refused, as in the parent
        "decode_eager": lambda: call("decode_eager", "decode", False),
        "decode_graphed": lambda: call("decode_graphed", "decode", True),
        "full_forward_k": lambda: full_forward_pixels(model, empty, k),
        "full_forward_2k": lambda: full_forward_pixels(model, empty, 2 * k),
    }
    times = compare(variants, repeats)
    row = {"model": what, "image": [c, h, w], "n_samples": n, "row_step_captured": captured, "full_pixels_timed": [k, 2 * k],
           "timed_s": times}
    for name in ("prefix_eager", "decode_eager", "decode_graphed"):
        row[name + "_s"] = statistics.median(times[name])
    per_pixel = statistics.median([(t2 - t1) / k for t1, t2 in zip(times["full_forward_k"], times["full_forward_2k"])])
    row["full_forward_per_pixel_s"] = per_pixel
    row["full_forward_s"] = per_pixel * h * w
    row["graphed_speedup_over_prefix_eager"] = row["prefix_eager_s"] / row["decode_graphed_s"]
    row["graphed_speedup_over_full_forward"] = row["full_forward_s"] / row["decode_graphed_s"]
    row["graphed_is_fastest"] = row["decode_graphed_s"] < min(row["prefix_eager_s"], row["full_forward_s"])
    return row


def row_step_replay(model, n, shape, replays=100):
    """The captured row step (evaluate, no commit) at the last row over full caches: microseconds per replay."""
    from pytorch_generative_amd import graph as pg_graph
    from pytorch_generative_amd import ops

    c, h, w = shape
    dev = next(model.parameters()).device
    ops.RowDecode.drop_caches(model)
    row_in = torch.bernoulli(torch.full((n, c, 1, w), 0.5, device=dev))
    with torch.no_grad(), ops.RowDecode(h) as ctx:
        def warm():
            ctx.commit = True  # allocates every band and cache
            model.forward(row_in)
            ctx.commit = False
            model.forward(row_in)

        pg_graph.warm_up(warm)
        for m in model.modules():  # full caches: what the last row of an image sees
            for name in ("_row_k", "_row_v"):
                if getattr(m, name, None) is not None:
                    getattr(m, name).normal_()
        ctx.row = h - 1
        graph, _ = pg_graph.capture(lambda: model.forward(row_in))
        for _ in range(10):
            graph.replay()
        torch.cuda.synchronize()
        per = []
        for _ in range(5):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(replays):
                graph.replay()
            b.record()
            torch.cuda.synchronize()
            per.append(a.elapsed_time(b) * 1e3 / replays)
    ops.RowDecode.drop_caches(model)
    return {"us_median_of_5": statistics.median(per), "us_min_max": [min(per), max(per)], "replays_per_timing": replays,
            "row": h - 1}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pixelsnail_sampling.json"))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--models", nargs="+", choices=sorted(MODELS), default=["recipe", "benchmark"])
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 16, 64, 256])
    ap.add_argument("--full-pixels", type=int, default=8, help="k: the full-forward sampler is timed on k and 2k pixels")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "pixelsnail_sample_bench needs the MI355X"
    assert a.repeats >= 5, "medians are taken over at least 5 calls"
    dev = torch.device("cuda:0")
    from pytorch_generative_amd import ops

    t0 = time.time()
    rec = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "repeats": a.repeats,
           "note": "prefix_eager / decode_eager / decode_graphed: whole sample() calls, wall clock to a device synchronise, graph "
                   "capture included; full_forward_s is H W times a per-pixel cost taken from the difference of two runs of "
                   "sample(incremental=False)'s loop body over k and 2k pixels (full_pixels_timed) of the same round; one warm-up "
                   "round, the variants of a row alternating within a round; *_s are medians of timed_s",
           "attention_plan": {}, "rows": []}

    def write():
        rec["seconds"] = time.time() - t0
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")

    for key in a.models:
        c, h, w = MODELS[key]
        what = f"PixelSNAIL({c} -> {c}, {h} x {w}, 64 channels, 8 blocks, key 4 / value 32)"
        rec["attention_plan"][key] = ops.attention_row_plan(1, 4, 32, h, w)
        model = _model(dev, c)
        model(torch.zeros(1, c, h, w, device=dev))  # registers the image shape
        for n in a.batches:
            row = sample_row(model, what, n, (c, h, w), a.repeats, a.full_pixels)
            row["row_step_replay_us"] = row_step_replay(model, n, (c, h, w))
            slim = {k: v for k, v in row.items() if k != "timed_s"}
            print(json.dumps(slim), flush=True)
            rec["rows"].append(row)
            write()  # after every row: a run that is cut short keeps what it measured
            torch.cuda.empty_cache()
    write()
    print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
