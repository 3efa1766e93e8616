"""ImageGPT sampling on the MI355X: the one-launch decode step (ops.gpt_decode_step, csrc/gpt_decode.hip) against the
full-forward sampler, and against the block-kernel K/V-cached route at the width both cover.

usage: python tools/gpt_decode_bench.py [--out profiles/gpt_decode.json] [--repeats 5] [--only recipe|prior|baseline|step]

Every figure of (a)-(c) is the wall clock around a whole `sample()` call that ends in a device synchronise (graph capture
and the parameter pack included: they are part of every call). The routes of a comparison run in the same process and
alternate within a round; one warm-up round, then `--repeats` (at least 5) timed rounds; medians are reported, all timings kept.

(a) `recipe`: models.autoregressive.image_gpt.reproduce()'s model (64 channels, 2 heads, 8 blocks, 28 x 28, one binary
    channel) at n = 1, 16, 64: the step kernel against `incremental=False` (a full forward per pixel; whole calls), and
    the step kernel alone at n = 1024 (one workgroup per sample, not tuned for that many).
(b) `prior`: models.vae.vq_vae.reproduce_prior()'s model (K = 512 codes, 64 channels, 2 heads, 8 blocks) over 8 x 8 and
    32 x 32 code images at n = 64, against `incremental=False`.
(c) `baseline`: the 16-channel, 4-head, 8-block benchmark shape on 28 x 28 at n = 64: the block-kernel cached route (what
    sample() takes there) against the step kernel forced with sample(route="step"). This number tells whether to reroute.
(d) `step`: the step alone — one hipGraph holding one pg_gpt_decode_step at p = L - 1, replayed: microseconds per position;
    and the library calls per position of each route, counted over one eager sample() call (ATen launches of the final
    transpose and of the draw are the same on both routes and not counted)."""

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pytorch-generative_amd"))
import torch  # noqa: E402

K_PRIOR = 512


def _gpt(dev, size, channels, heads, cin=1, sample_fn=None):
    from pytorch_generative_amd import models

    torch.manual_seed(0)
    model = models.ImageGPT(in_channels=cin, out_channels=cin, in_size=size, n_transformer_blocks=8,
                            n_attention_heads=heads, n_embedding_channels=channels, sample_fn=sample_fn).to(dev)
    with torch.no_grad():
        model._pos.normal_(0, 0.1)
    return model


def _prior(dev, size):
    from pytorch_generative_amd import nn as pg_nn

    model = _gpt(dev, size, 64, 2, cin=K_PRIOR,
                 sample_fn=pg_nn.CategoricalSampler(K_PRIOR, generator=torch.Generator(device=dev).manual_seed(0)))
    model.input_codes = K_PRIOR
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


def sample_row(model, n, size, repeats, variants, what):
    """variants: {name: sample() keywords}. The route each call took is recorded from model._sample_route."""
    dev = model._pos.device
    c = 1 if model.input_codes is not None else model._pos.shape[1]
    empty = torch.full((n, c, size, size), -1.0, device=dev)
    routes = {}

    def call(name, kw):
        out = model.sample(conditioned_on=empty, **kw)
        routes[name] = model._sample_route
        assert out.shape == empty.shape and bool((out >= 0).all())

    times = compare({name: (lambda name=name, kw=kw: call(name, kw)) for name, kw in variants.items()}, repeats)
    row = {"model": what, "n_samples": n, "positions": size * size, "kv_cached_sampler_taken": bool(model._incremental_ok(n)),
           "route_taken": routes, "timed_s": times}
    for name in variants:
        row[name + "_s"] = statistics.median(times[name])
    return row


def step_alone(dev, channels, heads, size, n, replays=200):
    """One hipGraph = one pg_gpt_decode_step of all 8 blocks at p = L - 1 over full caches; microseconds per replay."""
    from pytorch_generative_amd import ops

    model = _gpt(dev, size, channels, heads)
    L, ld = size * size, (n + 15) // 16 * 16
    pack = ops.gpt_decode_pack(model._transformer)
    g = torch.Generator().manual_seed(1)
    x0 = torch.randn(channels, ld, generator=g).to(dev)
    x = x0.clone()
    kc = torch.randn(8, n, channels, L, generator=g).to(dev)
    vc = torch.randn(8, n, channels, L, generator=g).to(dev)
    pos = torch.full((1,), L - 1, dtype=torch.int32, device=dev)

    def step():
        x.copy_(x0)  # in place: keep the input the same for every replay (the copy is part of the graph, 1 extra launch)
        ops.gpt_decode_step(x, pack, kc, vc, pos, heads=heads)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    for _ in range(20):
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
    plan = ops.gpt_decode_plan(channels, heads, 8, L)
    return {"shape": f"{channels} channels, {heads} heads, 8 blocks, L = {L}, n = {n}, p = L - 1",
            "us_per_position_median_of_5": statistics.median(per), "us_min_max": [min(per), max(per)],
            "replays_per_timing": replays, "launches_in_graph": 2, "step_kernel_launches_per_position": 1,
            "lds_bytes_per_workgroup": plan["lds_bytes"], "pack_floats": plan["pack_floats"]}


class _CountingLib:
    """Counts the C-ABI calls that launch kernels (everything except queries)."""

    QUERIES = ("pg_last_error", "pg_abi_version", "pg_gpt_decode_plan")

    def __init__(self, lib):
        self._lib, self.calls = lib, {}

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith("pg_") or name in self.QUERIES or name.endswith(("_supported", "_floats", "_ok", "_plan")):
            return fn

        def call(*args):
            self.calls[name] = self.calls.get(name, 0) + 1
            return fn(*args)

        return call


def library_calls_per_position(dev, channels, heads, route, size=8, n=16):
    """One eager sample() (graph capture refused): its library calls over the L + 1 positions it evaluates (one warm-up)."""
    from pytorch_generative_amd import _lib

    model = _gpt(dev, size, channels, heads)
    empty = torch.full((n, 1, size, size), -1.0, device=dev)
    real, real_graph = _lib.load(), torch.cuda.CUDAGraph

    class Refused:
        def __init__(self, *a, **k):
            raise RuntimeError("capture refused: count eager launches")

    counter = _CountingLib(real)
    _lib._lib, torch.cuda.CUDAGraph = counter, Refused
    try:
        model.sample(conditioned_on=empty, route=route)
    finally:
        _lib._lib, torch.cuda.CUDAGraph = real, real_graph
    assert model._sample_route == route
    positions = size * size + 1
    per = {k: v / positions for k, v in sorted(counter.calls.items())}
    return {"shape": f"{channels} channels, {heads} heads, 8 blocks", "route": route, "per_call": per,
            "library_calls_per_position": sum(counter.calls.values()) / positions}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gpt_decode.json"))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--only", choices=["recipe", "prior", "baseline", "step"], default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "gpt_decode_bench needs the MI355X"
    assert a.repeats >= 5, "medians are taken over at least 5 calls"
    dev = torch.device("cuda:0")
    t0 = time.time()
    rec = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "repeats": a.repeats,
           "note": "whole sample() calls, wall clock to a device synchronise, one warm-up round, the variants of a row "
                   "alternating within a round; *_s are medians of timed_s",
           "recipe": [], "prior": [], "baseline": [], "step": []}

    def emit(key, row):
        print(json.dumps(row), flush=True)
        rec[key].append(row)
        torch.cuda.empty_cache()

    both = {"step_kernel": {}, "full_forward_per_position": {"incremental": False}}
    if a.only in (None, "recipe"):
        model = _gpt(dev, 28, 64, 2)
        what = "ImageGPT(1 -> 1, in_size=28, 8 blocks, 2 heads, 64 channels)"
        for n in (1, 16, 64):
            row = sample_row(model, n, 28, a.repeats, both, what)
            row["speedup"] = row["full_forward_per_position_s"] / row["step_kernel_s"]
            emit("recipe", row)
        row = sample_row(model, 1024, 28, a.repeats, {"step_kernel": {}}, what)
        row["note"] = "one workgroup per sample; several samples per workgroup for very large n are not built: not tuned"
        emit("recipe", row)
    if a.only in (None, "prior"):
        for size in (8, 32):
            row = sample_row(_prior(dev, size), 64, size, a.repeats, both,
                             f"ImageGPT(K={K_PRIOR} codes, in_size={size}, 8 blocks, 2 heads, 64 channels)")
            row["speedup"] = row["full_forward_per_position_s"] / row["step_kernel_s"]
            emit("prior", row)
    if a.only in (None, "baseline"):
        row = sample_row(_gpt(dev, 28, 16, 4), 64, 28, a.repeats,
                         {"block_kernels": {}, "step_kernel": {"route": "step"}},
                         "ImageGPT(1 -> 1, in_size=28, 8 blocks, 4 heads, 16 channels)")
        row["step_kernel_speedup_over_block_kernels"] = row["block_kernels_s"] / row["step_kernel_s"]
        emit("baseline", row)
    if a.only in (None, "step"):
        emit("step", step_alone(dev, 64, 2, 28, 64))
        emit("step", step_alone(dev, 16, 4, 28, 64))
        emit("step", library_calls_per_position(dev, 64, 2, "step"))
        emit("step", library_calls_per_position(dev, 16, 4, "step"))
        emit("step", library_calls_per_position(dev, 16, 4, "blocks"))
    for key in ("recipe", "prior", "baseline", "step"):
        if not rec[key]:
            rec[key] = {"status": "NOT YET MEASURED", "how": "tools/gpt_decode_bench.py"}
    rec["seconds"] = time.time() - t0
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
