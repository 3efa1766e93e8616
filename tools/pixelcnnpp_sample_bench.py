"""PixelCNN++ sampling on the MI355X: the row-cached incremental sampler against the full-forward sampler.

usage: python tools/pixelcnnpp_sample_bench.py [--out profiles/pixelcnnpp_sampling.json] [--batches 1 16 64]
                                               [--repeats 3] [--full-pixels 32] [--whole-parent-batches 1]

Model: the paper configuration (160 filters, 5 resnets per stage, 10 mixture components), random weights, 32 x 32 x 3.
Per batch size n, seconds per `sample(n_samples=n)` call (host clock around a call that ends in a device synchronise) in four
variants, each timed `--repeats` times after one warm-up round, the variants alternating within a round; medians are reported:

* `incremental_graphed_s`: sample(), the default path — row steps replayed from their hipGraphs, captures included (they are
  part of every call). A whole all-unknown call.
* `incremental_eager_s`: the same with capture switched off (`_row_graph = False`): every row step launched eagerly.
* `full_forward_s`: sample(incremental=False), one full forward and sample_from_mixture per pixel.
* `parent_s`: the sampler as it stood before the incremental path existed, restated here (`parent_sample`): the yardstick.

The last two are not run whole: each is timed on two canvases whose last k and 2k pixels (`--full-pixels` k) are unknown and
all others known. A call on such a canvas also scans its known pixels, with a host sync each, which a whole all-unknown call
does not; so the per-pixel cost is taken from the DIFFERENCE of the two calls, (t_2k - t_k) / k, where that fixed part
cancels, and multiplied by H W. `*_fixed_part_of_timed_call_s` records what cancelled. At `--whole-parent-batches` one whole
all-unknown call of the parent's sampler is timed as well (`parent_whole_call_s`), as a check of the scaling.
`launches_per_pixel` counts, for one all-levels row step (y % 4 == 0) and one odd-row step, the C-ABI calls of the library and
the ATen copies next to them (the band copies of nn.Conv2d), each of which is one kernel launch.

The routing rule (`PixelCNNpp._incremental_min_batch`) follows from `rows`: the smallest measured batch size from which the
graphed incremental path is faster than the parent's sampler at every larger measured size.
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

H = W = 32
CONFIG = dict(in_channels=3, n_filters=160, n_resnet=5, n_mix=10)


@torch.no_grad()
def parent_sample(model, conditioned_on):
    """The sampler before the incremental path: one full forward, two dozen ATen launches and one host sync per pixel."""
    canvas = conditioned_on.clone()
    n, _, h, w = canvas.shape
    unknown = canvas < -1.0
    canvas = torch.where(unknown, torch.zeros_like(canvas), canvas)
    for row in range(h):
        for col in range(w):
            if not bool(unknown[:, :, row, col].any()):
                continue
            params = model._net(canvas)[:, :, row, col]
            drawn = model.sample_from_mixture(params, model._n_mix)
            canvas[:, :, row, col] = torch.where(unknown[:, :, row, col], drawn, canvas[:, :, row, col])
    return canvas


class _CountingLib:
    """Counts the C-ABI calls that launch kernels (everything except queries)."""

    def __init__(self, lib):
        self._lib, self.calls = lib, 0

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith("pg_") or name in ("pg_last_error", "pg_abi_version"):
            return fn

        def call(*args):
            self.calls += 1
            return fn(*args)

        return call


def launches_per_pixel(model, n, dev):
    """One eager row step of each extreme class (all three levels / level 0 only) plus the draw."""
    from pytorch_generative_amd import _lib, ops

    out = {}
    real = _lib.load()
    k = model._n_mix
    row_in = torch.zeros((n, 3, 1, W), device=dev)
    canvas = torch.zeros((n, 3, H, W), device=dev)
    unknown = torch.ones((n, 3, H, W), device=dev, dtype=torch.bool)
    uniforms = torch.rand((H * W, n, k + 3), device=dev)
    ops.RowDecode.drop_caches(model)
    with torch.no_grad(), ops.RowDecode(H) as ctx:
        for name, row in (("row_with_all_levels", 0), ("odd_row", 1)):
            ctx.row, ctx.commit = row, False

            def step():
                ops.dmol_sample(model._row_net(ctx, row_in), uniforms, canvas, unknown, k, row, 0, row_buf=row_in)

            step()  # bands and constants exist afterwards
            counter, aten = _CountingLib(real), [0]
            real_copy, real_clone = torch.Tensor.copy_, torch.Tensor.clone
            torch.Tensor.copy_ = lambda t, *x, **kw: (aten.__setitem__(0, aten[0] + 1), real_copy(t, *x, **kw))[1]
            torch.Tensor.clone = lambda t, *x, **kw: (aten.__setitem__(0, aten[0] + 1), real_clone(t, *x, **kw))[1]
            _lib._lib = counter
            try:
                step()
            finally:
                _lib._lib = real
                torch.Tensor.copy_, torch.Tensor.clone = real_copy, real_clone
            rec = {"library_calls": counter.calls, "aten_copies": aten[0], "launches": counter.calls + aten[0]}
            out[name] = rec
    ops.RowDecode.drop_caches(model)
    out["graphed_host_launches_per_pixel"] = 2  # one position fill + one graph replay
    out["full_forward_note"] = ("the full-forward sampler launches the whole network (about 90 convolutions and their "
                                "element-wise kernels) plus about two dozen ATen kernels of sample_from_mixture per pixel")
    return out


def known_but_last(n, pixels, dev):
    """An (n, 3, H, W) canvas in [-1, 1] whose last `pixels` raster positions are unknown."""
    g = torch.Generator().manual_seed(n)
    cond = (torch.rand(n, 3, H, W, generator=g) * 2.0 - 1.0).to(dev)
    cond.view(n, 3, H * W)[:, :, H * W - pixels:] = -2.0
    return cond


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pixelcnnpp_sampling.json"))
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 16, 64])
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--full-pixels", type=int, default=32, help="k: the full-forward samplers are timed on k and 2k unknown pixels")
    ap.add_argument("--whole-parent-batches", type=int, nargs="*", default=[1],
                    help="batch sizes at which one WHOLE call of the parent's sampler is timed too, as a check of the scaling")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "pixelcnnpp_sample_bench needs the MI355X"
    k = a.full_pixels
    assert a.repeats >= 1 and 1 <= 2 * k <= H * W
    dev = torch.device("cuda:0")
    import pytorch_generative_amd as pg

    torch.manual_seed(0)
    model = pg.models.PixelCNNpp(**CONFIG).to(dev)

    def incremental(n, graph):
        model._row_graph = graph
        try:
            return model.sample(n_samples=n, image_size=(H, W))
        finally:
            model._row_graph = True

    rows = []
    for n in a.batches:
        cond_k, cond_2k = known_but_last(n, k, dev), known_but_last(n, 2 * k, dev)
        variants = {
            "incremental_graphed": lambda: incremental(n, True),
            "incremental_eager": lambda: incremental(n, False),
            "full_forward_k": lambda: model.sample(conditioned_on=cond_k, incremental=False),
            "full_forward_2k": lambda: model.sample(conditioned_on=cond_2k, incremental=False),
            "parent_k": lambda: parent_sample(model, cond_k),
            "parent_2k": lambda: parent_sample(model, cond_2k),
        }
        times = {name: [] for name in variants}
        for rnd in range(a.repeats + 1):  # round 0 warms every variant up; the variants alternate within a round
            for name, fn in variants.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                if rnd:
                    times[name].append(time.perf_counter() - t0)
        row = {"n": n, "image": [3, H, W], "full_pixels_timed": [k, 2 * k], "timed_s": times}
        for name in ("incremental_graphed", "incremental_eager"):
            row[name + "_s"] = statistics.median(times[name])
        for name in ("full_forward", "parent"):
            # the per-pixel cost from the DIFFERENCE of the two calls of a round: what a call costs apart from its unknown
            # pixels (the scan of the known ones with its host sync each, the set-up) cancels
            per_pixel = statistics.median([(t2 - t1) / k for t1, t2 in zip(times[name + "_k"], times[name + "_2k"])])
            row[name + "_per_pixel_s"] = per_pixel
            row[name + "_s"] = per_pixel * H * W
            row[name + "_fixed_part_of_timed_call_s"] = statistics.median(times[name + "_k"]) - k * per_pixel
        if n in a.whole_parent_batches:
            cond_all = torch.full((n, 3, H, W), -2.0, device=dev)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            parent_sample(model, cond_all)
            torch.cuda.synchronize()
            row["parent_whole_call_s"] = time.perf_counter() - t0
        row["speedup_graphed_vs_parent"] = row["parent_s"] / row["incremental_graphed_s"]
        row["speedup_eager_vs_parent"] = row["parent_s"] / row["incremental_eager_s"]
        print(json.dumps(row), flush=True)
        rows.append(row)
    faster = [r["n"] for r in rows if r["incremental_graphed_s"] < r["parent_s"]]
    min_batch = None
    for r in sorted(rows, key=lambda r: -r["n"]):  # the smallest n from which every larger measured n is faster
        if r["n"] in faster:
            min_batch = r["n"]
        else:
            break
    note = ("full_forward_s and parent_s are H W times a per-pixel cost taken from the difference of two calls of the same round, "
            "with k and 2k unknown pixels at the end of an otherwise known canvas (full_pixels_timed), so that the fixed part of "
            "such a call (scanning the known pixels, one host sync each) cancels; parent_whole_call_s, where present, is ONE whole "
            "all-unknown call of the same sampler, timed as a check of that scaling; parent_s is the sampler as it stood before "
            "the incremental path, restated in tools/pixelcnnpp_sample_bench.py (parent_sample); the incremental variants are "
            "whole all-unknown calls, graph captures included; every variant is timed `repeats` times after one warm-up round, "
            "the variants alternating within a round")
    rec = {"measured": True, "note": note, "device": torch.cuda.get_device_name(0), "torch": torch.__version__, "config": CONFIG,
           "repeats": a.repeats, "rows": rows, "launches_per_pixel": launches_per_pixel(model, a.batches[-1], dev),
           "routing": {"incremental_min_batch_in_model": pg.models.PixelCNNpp._incremental_min_batch,
                       "smallest_measured_batch_from_which_incremental_is_faster": min_batch,
                       "rule": "sample(incremental=True) takes the row-cached path for n >= _incremental_min_batch (or with "
                               "return_params) and the full-forward procedure below it"}}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
    print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
