"""MADE sampling on the MI355X: the one-launch sampler on cached hidden sums (ops.made_sample_chain, csrc/made_sample.hip;
MADE.sample's route "chain") against the reference's procedure, one full masked forward per dimension (route "full").

usage: python tools/made_sample_bench.py [--out profiles/made_sampling.json] [--repeats 5] [--ns 1 16 64 1024]
                                         [--parity-report FILE]

(a) `sample`: models.autoregressive.made.reproduce()'s model, MADE(784, [8000]), at n = 1, 16, 64, 1024. Every figure is the
    wall clock around a whole `sample()` call that ends in a device synchronise (the in-place masking, the uniforms and the
    weight pack included: they are part of every call). The two routes run in the same process and alternate within a round;
    one warm-up round, then `--repeats` (at least 5) timed rounds; medians are reported, all timings kept.
(b) `launch`: the two kernels of the chain route alone, device events around single launches on an empty canvas: the pack
    (pg_made_sample_pack) and the chain (pg_made_sample), median of 9 after one warm-up, at the same n.
(c) `parity`: the worst logit error of tests/test_gpu_made_sampling.py against the float64 chain, read from the file that
    `PG_PARITY_REPORT=FILE pytest -m gpu tests/test_gpu_made_sampling.py` appends to (--parity-report FILE)."""

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pytorch-generative_amd"))
import torch  # noqa: E402

D, H = 784, 8000


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


def sample_row(model, n, repeats):
    empty = torch.full((n, D), -1.0, device=model.device)
    routes = {}

    def call(name, kw):
        out = model.sample(conditioned_on=empty, **kw)
        routes[name] = model._sample_route
        assert out.shape == empty.shape and bool(((out == 0) | (out == 1)).all())

    variants = {"chain": {}, "full": {"incremental": False}}
    times = compare({name: (lambda name=name, kw=kw: call(name, kw)) for name, kw in variants.items()}, repeats)
    assert routes == {"chain": "chain", "full": "full"}, routes
    row = {"model": f"MADE({D}, [{H}])", "n_samples": n, "dimensions": D, "route_taken": routes, "timed_s": times}
    for name in variants:
        row[name + "_s"] = statistics.median(times[name])
    row["speedup"] = row["full_s"] / row["chain_s"]
    return row


def launch_row(model, n, timings=9):
    """Device events around single launches of the chain route's two kernels on the model's (already masked) weights."""
    from pytorch_generative_amd import _lib, ops

    lib, dev = _lib.load(), model.device
    hidden, out = model._masked_layers()
    plan = ops.made_sample_plan(D, H, n)
    pack = torch.empty(plan["pack_floats"], device=dev)
    canvas = torch.empty((n, D), device=dev)
    uniforms = torch.rand((n, D), device=dev, generator=torch.Generator(device=dev).manual_seed(0))
    order = model._order(0, dev)
    stream = torch.cuda.current_stream().cuda_stream

    def run_pack():
        _lib.check(lib.pg_made_sample_pack(hidden.weight.data_ptr(), out.weight.data_ptr(), pack.data_ptr(), D, H, stream),
                   "pg_made_sample_pack")

    def run_chain():
        _lib.check(lib.pg_made_sample(pack.data_ptr(), hidden.bias.data_ptr(), out.bias.data_ptr(), order.data_ptr(),
                                      canvas.data_ptr(), uniforms.data_ptr(), None, n, D, H, stream), "pg_made_sample")

    def timed(fn):
        per = []
        for i in range(timings + 1):
            canvas.fill_(-1.0)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            if i:
                per.append(a.elapsed_time(b) * 1e3)
        return {"us_median": statistics.median(per), "us_min_max": [min(per), max(per)], "launches_timed": timings}

    row = {"n_samples": n, "plan": plan, "pack": timed(run_pack), "chain": timed(run_chain)}
    row["chain_us_per_dimension"] = row["chain"]["us_median"] / D
    return row


def parity(path):
    rows = [json.loads(line) for line in open(path) if line.strip()]
    rows = [r for r in rows if str(r.get("case", "")).startswith("made_sample ")]
    assert rows, f"{path}: no made_sample parity record"
    worst = max(rows, key=lambda r: r["worst_logit_rel_err"])
    return {"cases": len(rows), "worst_logit_rel_err": worst["worst_logit_rel_err"], "worst_case": worst["case"],
            "tol": worst["tol"], "reference": "float64 chain, tests/made_sample_ref.py"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "made_sampling.json"))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--ns", type=int, nargs="+", default=[1, 16, 64, 1024])
    ap.add_argument("--parity-report", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "made_sample_bench needs the MI355X"
    assert a.repeats >= 5, "medians are taken over at least 5 calls"
    from pytorch_generative_amd import models

    dev = torch.device("cuda:0")
    t0 = time.time()
    rec = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "repeats": a.repeats,
           "note": "sample: whole sample() calls, wall clock to a device synchronise, one warm-up round, the two routes "
                   "alternating within a round; *_s are medians of timed_s. launch: device events around single launches",
           "sample": [], "launch": []}
    torch.manual_seed(0)
    model = models.MADE(input_dim=D, hidden_dims=[H], n_masks=1).to(dev)
    for n in a.ns:
        row = sample_row(model, n, a.repeats)
        print(json.dumps(row), flush=True)
        rec["sample"].append(row)
    for n in a.ns:
        row = launch_row(model, n)
        print(json.dumps(row), flush=True)
        rec["launch"].append(row)
    rec["parity"] = parity(a.parity_report) if a.parity_report else {"status": "NOT YET MEASURED",
                                                                     "how": "--parity-report, see the docstring"}
    rec["seconds"] = time.time() - t0
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
