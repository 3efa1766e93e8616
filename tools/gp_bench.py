"""The Gaussian process on the MI355X: whole `predict` calls, the Bayesian-optimisation loop, the factorisation alone and the two
covariance routes.

usage: python tools/gp_bench.py [--out profiles/gp.json] [--rounds 5]

* `predict`: GaussianProcess.predict at (n, m, d) = (512, 1024, 1), (4096, 1024, 1), (4096, 4096, 8), (8192, 2048, 64):
  `predict_cached_ms` with the factor kept from the call before (what a second `predict` costs), `predict_fresh_ms` after
  reset_cache() (covariance, factorisation, both solves of alpha and the read of info included). FOR COMPARISON ONLY, in eager
  torch-ROCm on the same GPU: `reference_lu_ms`, the reference's algorithm (torch.cdist, torch.linalg.solve, eye on the device),
  and `torch_cholesky_ms` (torch.linalg.cholesky + cholesky_solve). Nothing in the library routes around its own kernels, so a
  figure that loses is written down as it is. `err_vs_float64`: every candidate's
  max |mu - mu64| / max |mu64| and max |sig - sig64| (the prior variance is 1) against the float64 posterior on the same GPU.
* `bo_loop`: 256 rounds of fit-one-point, predict, sample(1) on a grid of 1024 points, `incremental` True ("append") against
  False ("full"); host clock around the whole loop (every round reads info back).
* `factor`: ops.cholesky_ alone at n = 1024, 4096, 8192 (a device copy of the matrix included) in TFLOP/s of n^3 / 3 against the
  157.3 TFLOP/s fp32 matrix peak, and torch.linalg.cholesky beside it.
* `se_routes`: the cross covariance (4096, 4096) at d = 4, 8, 16, 32, 64 on the exact-difference and on the MFMA route.
* `parity`: the worst errors against float64 over the grid of tests/test_gpu_gp.py.
Protocol: the candidates alternate in one process, `--rounds` rounds of timed calls between HIP events after a warm-up; the
figure is the median over the rounds of the per-call mean; every call takes the next of four resident query sets."""

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pytorch-generative_amd"))
import torch  # noqa: E402

SETS = 4
PEAK_TFLOPS = 157.3
PREDICT_SHAPES = ((512, 1024, 1, 20), (4096, 1024, 1, 10), (4096, 4096, 8, 5), (8192, 2048, 64, 3))  # (n, m, d, calls per round)
NOISE = 0.1


def data(n, m, d, dev):
    """Training and query points of a moderately conditioned problem: about 20 points per lengthscale on a line, random
    directions in higher dimensions with the lengthscale at sqrt(d)."""
    g = torch.Generator().manual_seed(n + d)
    if d == 1:
        tx, lengthscale = torch.rand(n, 1, generator=g) * n / 20, 1.0
        xs = [torch.rand(m, 1, generator=g) * n / 20 for _ in range(SETS)]
    else:
        tx, lengthscale = torch.randn(n, d, generator=g), float(d) ** 0.5
        xs = [torch.randn(m, d, generator=g) for _ in range(SETS)]
    ty = torch.sin(tx.sum(1, keepdim=True)) + NOISE ** 0.5 * torch.randn(n, 1, generator=g)
    return tx.to(dev), ty.to(dev), [x.to(dev) for x in xs], lengthscale


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
    for fn, it in fns.values():
        for k in range(2):
            fn(k)
    torch.cuda.synchronize()
    ts = {name: [] for name in fns}
    for r in range(rounds):
        for name, (fn, it) in fns.items():
            ts[name].append(time_round(fn, it, r * it))
    return {name: statistics.median(v) for name, v in ts.items()}, {name: [min(v), max(v)] for name, v in ts.items()}


def float64_errors(tx, ty, x, lengthscale, results):
    """{candidate: {mu, sig}} against the posterior in float64 on the same GPU (squared distances as |a|^2 + |b|^2 - 2 a.b in
    float64, clamped at 0: 1e-11 absolute at these inputs; Cholesky solve)."""
    tx, ty, x = tx.double(), ty.double(), x.double()

    def kernel(a, b):
        sq = (a * a).sum(1)[:, None] + (b * b).sum(1)[None, :] - 2.0 * (a @ b.t())
        return torch.exp(-0.5 * sq.clamp_min_(0.0) / lengthscale ** 2)

    chol = torch.linalg.cholesky(kernel(tx, tx) + NOISE * torch.eye(tx.shape[0], device=tx.device, dtype=torch.float64))
    cross = kernel(tx, x)
    w = torch.cholesky_solve(cross, chol).t()
    mu, sig = w @ ty, kernel(x, x) - w @ cross
    return {name: {"mu": float((m.double() - mu).abs().max() / mu.abs().max()), "sig": float((s.double() - sig).abs().max())}
            for name, (m, s) in results.items()}


def predict_rows(dev, rounds):
    from pytorch_generative_amd import ops
    from pytorch_generative_amd.models import gaussian_process as gp

    rows = []
    for n, m, d, iters in PREDICT_SHAPES:
        tx, ty, xs, lengthscale = data(n, m, d, dev)
        model = gp.GaussianProcess(gp.Const(0.0), gp.SquaredExponential(1.0, lengthscale), NOISE).to(dev)
        model.fit(tx, ty)
        eye = torch.eye(n, device=dev)

        def kernel(a, b):
            return torch.exp(-0.5 * (torch.cdist(a, b) / lengthscale) ** 2)

        def cached(k):
            model.predict(xs[k % SETS])

        def fresh(k):
            model.reset_cache()
            model.predict(xs[k % SETS])

        def reference_lu(k):
            x = xs[k % SETS]
            k_cross = kernel(tx, x)
            w = torch.linalg.solve(kernel(tx, tx) + NOISE * eye, k_cross).T
            return w @ ty, kernel(x, x) - w @ k_cross

        def torch_cholesky(k):
            x = xs[k % SETS]
            chol = torch.linalg.cholesky(kernel(tx, tx) + NOISE * eye)
            cross = kernel(tx, x)
            solved = torch.cholesky_solve(cross, chol).T
            return solved @ ty, kernel(x, x) - solved @ cross

        errors = float64_errors(tx, ty, xs[0], lengthscale, {"predict": model.predict(xs[0]), "reference_lu": reference_lu(0),
                                                             "torch_cholesky": torch_cholesky(0)})
        fns = {"predict_cached_ms": (cached, iters), "predict_fresh_ms": (fresh, iters), "reference_lu_ms": (reference_lu, iters),
               "torch_cholesky_ms": (torch_cholesky, iters)}
        med, spread = alternate(fns, rounds)
        row = {"n": n, "m": m, "d": d, "noise_var": NOISE, "lengthscale": lengthscale, "plan": ops.gp_plan(n, m, d, 1), **med,
               "min_max_ms": spread, "calls_per_round": iters, "err_vs_float64": errors,
               "fresh_vs_reference_lu": med["reference_lu_ms"] / med["predict_fresh_ms"],
               "fresh_vs_torch_cholesky": med["torch_cholesky_ms"] / med["predict_fresh_ms"],
               "cached_vs_reference_lu": med["reference_lu_ms"] / med["predict_cached_ms"]}
        print(json.dumps({k: v for k, v in row.items() if k != "plan"}), flush=True)
        rows.append(row)
        del model, eye
        torch.cuda.empty_cache()
    return rows


def bo_loop(dev, rounds, steps=256, grid=1024):
    from pytorch_generative_amd.models import gaussian_process as gp

    grid_x = torch.linspace(0, 10, grid, device=dev).reshape(-1, 1)
    f = lambda x: torch.sin(x) + torch.sin(10 / 3 * x)  # noqa: E731

    def run(incremental):
        model = gp.GaussianProcess(gp.Const(0.0), gp.SquaredExponential(1.0, 1.0), 0.01).to(dev)
        model.incremental = incremental
        gen = torch.Generator(device=dev).manual_seed(0)
        jitters = {}
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            sample = model.sample(grid_x, 1, generator=gen)
            jitters[model._sample_jitter] = jitters.get(model._sample_jitter, 0) + 1
            idx = int(torch.argmax(sample))
            x = grid_x[idx:idx + 1]
            model.fit(x, f(x))
            model.predict(grid_x)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, model._factor_route, jitters

    run(True), run(False)
    ts = {"append": [], "full": []}
    info = {}
    for _ in range(rounds):
        for name, inc in (("append", True), ("full", False)):
            ms, route, jitters = run(inc)
            ts[name].append(ms)
            info[name] = {"last_factor_route": route, "ladder_steps_taken": {f"{k:g}": v for k, v in sorted(jitters.items())}}
    out = {"rounds_of_the_loop": steps, "grid": grid, "noise_var": 0.01,
           "append_ms": statistics.median(ts["append"]), "full_ms": statistics.median(ts["full"]),
           "min_max_ms": {k: [min(v), max(v)] for k, v in ts.items()}, **info}
    out["append_vs_full"] = out["full_ms"] / out["append_ms"]
    print(json.dumps(out), flush=True)
    return out


def factor_rows(dev, rounds):
    from pytorch_generative_amd import ops

    rows = []
    for n, iters in ((1024, 10), (4096, 5), (8192, 3)):
        g = torch.Generator(device=dev).manual_seed(n)
        b = torch.randn(n, n, device=dev, generator=g)
        a = b @ b.t() / n + torch.eye(n, device=dev)
        work = torch.empty_like(a)
        info = torch.zeros(1, dtype=torch.int32, device=dev)

        def ours(k):
            work.copy_(a)
            ops.cholesky_(work, info=info)

        def torch_chol(k):
            torch.linalg.cholesky(a)

        ours(0)
        err = float((torch.tril(work) - torch.linalg.cholesky(a.double())).abs().max())
        assert int(info) == 0
        med, spread = alternate({"cholesky_ms": (ours, iters), "torch_cholesky_ms": (torch_chol, iters)}, rounds)
        flops = n ** 3 / 3
        row = {"n": n, **med, "min_max_ms": spread, "tflops": flops / med["cholesky_ms"] / 1e9,
               "share_of_fp32_matrix_peak": flops / med["cholesky_ms"] / 1e9 / PEAK_TFLOPS,
               "torch_tflops": flops / med["torch_cholesky_ms"] / 1e9, "vs_torch": med["torch_cholesky_ms"] / med["cholesky_ms"],
               "max_abs_err_vs_float64": err, "launches": ops.gp_plan(n, 1, 1, 1)["potrf_launches"]}
        print(json.dumps(row), flush=True)
        rows.append(row)
        del a, b, work
        torch.cuda.empty_cache()
    return rows


def se_routes(dev, rounds, n=4096):
    from pytorch_generative_amd import ops

    rows = []
    for d in (4, 8, 16, 32, 64):
        g = torch.Generator(device=dev).manual_seed(d)
        a = [torch.randn(n, d, device=dev, generator=g) for _ in range(SETS)]
        b = torch.randn(n, d, device=dev, generator=g)
        out = torch.empty(n, n, device=dev)
        fns = {r + "_ms": (lambda k, r=r: ops.se_kernel(a[k % SETS], b, 1.0, d ** 0.5, out=out, route=r), 20) for r in ("direct", "mfma")}
        med, spread = alternate(fns, rounds)
        direct = ops.se_kernel(a[0], b, 1.0, d ** 0.5, route="direct")
        mfma = ops.se_kernel(a[0], b, 1.0, d ** 0.5, route="mfma")
        row = {"n": n, "m": n, "d": d, **med, "min_max_ms": spread, "direct_vs_mfma": med["mfma_ms"] / med["direct_ms"],
               "plan_route": ("direct", "mfma")[ops.gp_plan(n, n, d, 1)["se_route"]], "max_abs_difference": float((direct - mfma).abs().max()),
               "output_gb_per_s": n * n * 4 / min(med.values()) / 1e6}
        print(json.dumps(row), flush=True)
        rows.append(row)
    return rows


def parity(dev):
    from pytorch_generative_amd import ops

    err = lambda got, want: float((got.double() - want).abs().max() / want.abs().max().clamp_min(1e-30))  # noqa: E731
    worst = {"factor": 0.0, "solve": 0.0, "solve_transposed": 0.0, "se_direct": 0.0, "se_mfma": 0.0}
    for n in (1, 2, 63, 64, 65, 130, 321):
        g = torch.Generator().manual_seed(100 + n)
        b = torch.randn(n, n, generator=g, dtype=torch.float64)
        a = (b @ b.t() / n + torch.eye(n, dtype=torch.float64)).float().to(dev)
        want = torch.linalg.cholesky(a.double())
        got = a.clone()
        ops.cholesky_(got)
        worst["factor"] = max(worst["factor"], err(torch.tril(got), want))
        low = want.float().contiguous()
        for rows in (1, 3, 64, 65):
            rhs = torch.randn(rows, n, device=dev)
            x = ops.trsm_right_(low, rhs.clone())
            worst["solve"] = max(worst["solve"], err(x, torch.linalg.solve_triangular(low.double(), rhs.double().t(), upper=False).t()))
            x = ops.trsm_right_(low, rhs.clone(), transposed=True)
            want_t = torch.linalg.solve_triangular(low.double().t(), rhs.double().t(), upper=True).t()
            worst["solve_transposed"] = max(worst["solve_transposed"], err(x, want_t))
    for d in (1, 3, 16, 17, 40):
        g = torch.Generator().manual_seed(d)
        a, b = torch.randn(130, d, generator=g).to(dev), torch.randn(70, d, generator=g).to(dev)
        lengthscale = 0.9 * d ** 0.5
        want = 1.69 * torch.exp(-torch.cdist(a.double(), b.double()) ** 2 / (2 * lengthscale ** 2))
        for route in ("direct", "mfma"):
            worst["se_" + route] = max(worst["se_" + route], err(ops.se_kernel(a, b, 1.3, lengthscale, route=route), want))
    out = {"reference": "float64 on the same GPU", "gate": 1e-4, "worst_max_normalised_err": worst}
    print(json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gp.json"))
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "gp_bench needs the MI355X"
    dev = torch.device("cuda:0")
    rec = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "rounds": a.rounds, "input_sets": SETS,
           "fp32_matrix_peak_tflops": PEAK_TFLOPS}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    sections = (("parity", lambda: parity(dev)), ("factor", lambda: factor_rows(dev, a.rounds)), ("se_routes", lambda: se_routes(dev, a.rounds)),
                ("predict", lambda: predict_rows(dev, a.rounds)), ("bo_loop", lambda: bo_loop(dev, a.rounds)))
    for name, section in sections:  # the file is rewritten after every finished section; any error but an exhausted ladder ends the tool
        try:
            rec[name] = section()
        except torch.linalg.LinAlgError as e:  # sample's jitter ladder exhausted: no device fault, written down as it is
            rec[name] = {"failed": f"{type(e).__name__}: {e}"}
            print(json.dumps({name: rec[name]}), flush=True)
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=1)
    print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
