"""Do two builds of the library give the same bits on the fp32-MFMA tile kernels (csrc/mfma_tile.h: dense_linear, fvbn, gp) and
on everything the Gaussian process runs?

    PG_HIP_LIB=<library A> timeout -k 10 240 python tools/tile_bits.py --label A --out A.json [--package <tree A>] \\
      && PG_HIP_LIB=<library B> timeout -k 10 240 python tools/tile_bits.py --label B --out B.json \\
      && python tools/tile_bits.py --compare A.json B.json [--verdict verdict.json]   # exit code 1 on any difference

One process per library (_lib loads one only), each under its own time limit, chained so that nothing starts after a failure.
The other library is built from an earlier commit with build.py's flags, outside the tree:
    mkdir -p /tmp/pg_parent && git archive <commit> pytorch-generative_amd include | tar -x -C /tmp/pg_parent \\
      && python /tmp/pg_parent/pytorch-generative_amd/build.py
    # -> /tmp/pg_parent/pytorch-generative_amd/pytorch_generative_amd/lib/libpg_hip.so
--package /tmp/pg_parent/pytorch-generative_amd imports pytorch_generative_amd from that directory instead of the working tree,
so that the earlier commit's Python layer (operators, model) runs on its own library; the cases only use names both have.

For a fixed list of cases the inputs come from seeded CPU generators, the entry points run once and the JSON holds the sha256 of
every output's raw bytes. The cases are the shape lists with which the GPU tests reach every branch of the three plans
(tests/test_gpu_nice.py DIRECT_SHAPES and its two extra weight-gradient shapes, tests/test_gpu_fvbn.py SHAPES,
tests/test_gpu_gp.py FACTOR_N, its append pairs, its GEMM update and its covariance at d = 17, 40); the dense list is checked
against pg_dense_linear_plan to reach small-unsplit, small-k-split and large for every kind, and the record says so. The
Gaussian process is covered beyond the tile: every covariance entry point, kind, lengthscale form and route on both sides of
the route threshold (gp_covariance), the triangular inverse and X X^T over one to three panels (gp_inverse), the three
reductions through the C-ABI with the workspace rows they write (gp_sums), the value, and three models end to end (gp_models)."""

import argparse
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pytorch-generative_amd"))

DENSE_SHAPES = [(5, 7, 3), (65, 33, 70), (8, 1500, 32), (130, 129, 258), (1537, 2, 2049), (1537, 33, 2049), (1537, 2049, 17)]
DENSE_WGRAD_EXTRA = [(3, 1665, 1665), (33, 1665, 1665)]
TILE = 64
FVBN_D = (1, 2, 3, 4, 5, 15, 16, 17, 63, 64, 65, 130, 200, 3 * TILE + 1)
FVBN_N = (1, 3, 64, 65, 257)
FVBN_SHAPES = [(d, n) for d in FVBN_D for n in FVBN_N] + [(200, 33 * TILE - 62)]
FACTOR_N = (1, 2, 63, 64, 65, 130, 321)
APPEND = [(1, 2), (63, 65), (64, 65), (65, 130), (130, 321)]
SE_D = (17, 40)
GP_KINDS = ("se", "matern32", "matern52")  # ops.GP_KINDS: 0, 1, 2
COV_D = (1, 16, 17, 64, 70)     # the route threshold (16 | 17) and the largest d of the forced exact-difference route (64 | 70)
INVERSE_N = (1, 63, 64, 65, 130)  # 130: three panels, a fresh row tile, a continued one, two column tiles in the update
SUMS_N = (1, 64, 65, 130)
SUMS_D = (1, 16, 17, 70)
ARD_D = (1, 64, 65, 130)        # one chunk, a full chunk, two chunks, three chunks
VALUE_N = (1, 65, 130)


def digest(t):
    import torch

    torch.cuda.synchronize()
    return hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()


def strided(rows, cols, ld, g, dev, fill=None):
    import torch

    buf = torch.full((rows, ld), 7.0)
    buf[:, :cols] = torch.randn(rows, cols, generator=g) if fill is None else fill
    return buf.to(dev)


def dense(dev, out):
    import torch
    from pytorch_generative_amd import _lib, ops

    lib, cl = _lib.load(), _lib.check
    st = torch.cuda.current_stream().cuda_stream
    reached = {}

    def ws_of(n, i, o, kind):
        plan = ops.dense_linear_plan(n, i, o, kind)
        branch = "large" if plan["variant"] == 1 else ("small-k-split" if plan["slices"] > 1 else "small-unsplit")
        reached.setdefault(kind, set()).add(branch)
        return torch.empty(max(plan["workspace_floats"], 1), device=dev), plan["workspace_floats"]

    for n, i, o in DENSE_SHAPES:
        g = torch.Generator().manual_seed(n * 31 + i * 7 + o)
        w, b = (torch.randn(o, i, generator=g) / i ** 0.5).to(dev), torch.randn(o, generator=g).to(dev)
        x, res = strided(n, i, i + 3, g, dev), strided(n, o, o + 5, g, dev)
        ws, floats = ws_of(n, i, o, "fwd")
        for bias, relu, sign in ((True, 0, 0), (False, 0, 0), (True, 1, 0), (True, 0, 1), (False, 0, -1)):
            y = torch.full((n, o + 2), 7.0, device=dev)
            cl(lib.pg_dense_linear_fwd(x.data_ptr(), i + 3, w.data_ptr(), b.data_ptr() if bias else 0, res.data_ptr() if sign else 0, o + 5,
                                       sign or 1, y.data_ptr(), o + 2, n, i, o, relu, ws.data_ptr(), floats, st), "fwd")
            out[f"dense fwd {n}x{i}x{o} bias={bias} relu={relu} sign={sign}"] = digest(y)
        g = torch.Generator().manual_seed(n * 37 + i * 5 + o)
        w = (torch.randn(o, i, generator=g) / o ** 0.5).to(dev)
        dy = strided(n, o, o + 1, g, dev)
        gate = strided(n, i, i + 2, g, dev, fill=torch.randn(n, i, generator=g).clamp_min(0))
        add = strided(n, i, i + 4, g, dev)
        ws, floats = ws_of(n, i, o, "dgrad")
        for gated, addend, sign in ((False, False, 1), (True, False, 1), (False, True, -1), (True, True, 1), (True, True, -1)):
            dx = torch.full((n, i + 3), 7.0, device=dev)
            cl(lib.pg_dense_linear_dgrad(dy.data_ptr(), o + 1, w.data_ptr(), gate.data_ptr() if gated else 0, i + 2,
                                         add.data_ptr() if addend else 0, i + 4, sign, dx.data_ptr(), i + 3, n, i, o, ws.data_ptr(), floats,
                                         st), "dgrad")
            out[f"dense dgrad {n}x{i}x{o} gate={gated} addend={addend} sign={sign}"] = digest(dx)
    for n, i, o in DENSE_SHAPES + DENSE_WGRAD_EXTRA:
        g = torch.Generator().manual_seed(n * 41 + i * 3 + o)
        x, dy = strided(n, i, i + 3, g, dev), strided(n, o, o + 2, g, dev)
        ws, floats = ws_of(n, i, o, "wgrad")
        for sign, with_db in ((1, True), (-1, True), (1, False)):
            dw, db = torch.randn(o, i, generator=g).to(dev), torch.randn(o, generator=g).to(dev)
            cl(lib.pg_dense_linear_wgrad(x.data_ptr(), i + 3, dy.data_ptr(), o + 2, sign, dw.data_ptr(), db.data_ptr() if with_db else 0, n, i,
                                         o, ws.data_ptr(), floats, st), "wgrad")
            out[f"dense wgrad {n}x{i}x{o} sign={sign} db={with_db} dw"] = digest(dw)
            out[f"dense wgrad {n}x{i}x{o} sign={sign} db={with_db} db"] = digest(db)
    want = {"small-unsplit", "small-k-split", "large"}
    assert all(reached[k] == want for k in ("fwd", "dgrad", "wgrad")), f"the dense shapes miss a plan branch: {reached}"
    return {k: sorted(v) for k, v in reached.items()}


def fvbn(dev, out):
    import torch
    from pytorch_generative_amd import ops

    reached = set()
    for d, n in FVBN_SHAPES:
        plan = ops.fvbn_plan(d, n)
        reached.add("fwd-split" if plan["forward_split"] else "fwd-walked")
        reached.add("wgrad-split" if plan["wgrad_slices"] > 1 else "wgrad-unsplit")
        g = torch.Generator().manual_seed(d * 1000 + n)
        weight = ops.fvbn_pack((torch.randn(d, d, generator=g) / max(d, 1) ** 0.5).to(dev)).requires_grad_()
        bias = torch.randn(d, generator=g).to(dev).requires_grad_()
        x = (torch.rand(n, d, generator=g) < 0.5).float().to(dev)
        logits = ops.fvbn(x, weight, bias)
        out[f"fvbn fwd D={d} N={n}"] = digest(logits)
        logits.backward(torch.randn(n, d, generator=g).to(dev))
        out[f"fvbn wgrad D={d} N={n} dw"] = digest(weight.grad)
        out[f"fvbn wgrad D={d} N={n} db"] = digest(bias.grad)
    return sorted(reached)


def spd(n, seed):
    import torch

    b = torch.randn(n, n, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)
    return (b @ b.t() / n + torch.eye(n, dtype=torch.float64)).float()


def gp(dev, out):
    import torch
    from pytorch_generative_amd import ops

    for n in FACTOR_N:
        for pad in (0, 37):
            buf = torch.full((n, n + pad), 7.0)
            buf[:, :n] = spd(n, 100 + n)
            buf = buf.to(dev)
            assert int(ops.cholesky_(buf[:, :n])) == 0
            out[f"gp potrf n={n} pad={pad}"] = digest(buf)
    for done, n in APPEND:
        buf = torch.full((n, 384), 7.0)
        buf[:, :n] = spd(n, 100 + n)
        buf = buf.to(dev)
        assert int(ops.cholesky_(buf[:done, :done])) == 0 and int(ops.cholesky_(buf[:, :n], n_done=done)) == 0
        out[f"gp potrf append {done}->{n}"] = digest(buf)
        low = torch.tril(buf[:, :n]).contiguous()
        b = torch.randn(3, n, generator=torch.Generator().manual_seed(n)).to(dev)
        ops.trsm_right_(low[:done, :done], b[:, :done])
        out[f"gp trsm append {done}->{n}"] = digest(ops.trsm_right_(low, b, col_done=done))
        out[f"gp trsm transposed n={n}"] = digest(ops.trsm_right_(low, torch.randn(3, n, generator=torch.Generator().manual_seed(n + 1)).to(dev),
                                                                  transposed=True))
    g = torch.Generator().manual_seed(11)
    a, b, c = torch.randn(70, 160, generator=g).to(dev), torch.randn(90, 160, generator=g).to(dev), torch.randn(70, 90, generator=g).to(dev)
    out["gp gemm c - a b^T"] = digest(ops.gemm_nt_(c.clone(), a, b))
    pieces = c.clone()
    for lo, hi in ((0, 64), (64, 128), (128, 160)):
        ops.gemm_nt_(pieces, a[:, lo:hi], b[:, lo:hi])
    out["gp gemm in three pieces"] = digest(pieces)
    out["gp gemm c + a b, b transposed"] = digest(ops.gemm_nt_(c.clone(), a, b.t().contiguous(), add=True, b_transposed=True))
    out["gp gemm lower mirrored"] = digest(ops.gemm_nt_(torch.randn(70, 70, generator=g).to(dev), a, a, lower=True, mirror=True))
    for d in SE_D:
        g = torch.Generator().manual_seed(d)
        a, b = torch.randn(130, d, generator=g).to(dev), torch.randn(70, d, generator=g).to(dev)
        std, lengthscale = 1.3, 0.9 * d ** 0.5
        cross = torch.full((130, 79), 7.0, device=dev)
        ops.se_kernel(a, b, std, lengthscale, 0.05, out=cross[:, :70], route="mfma")
        out[f"gp se d={d} cross"] = digest(cross)
        out[f"gp se d={d} symmetric mirrored diag"] = digest(ops.se_kernel(a, a, std, lengthscale, 0.05, route="mfma"))
        rows = torch.full((60, 130), 7.0, device=dev)
        ops.se_kernel(a[70:], a, std, lengthscale, 0.05, out=rows, diag_offset=70, route="mfma")
        out[f"gp se d={d} lower rows diag_offset=70"] = digest(rows)
        half = torch.full((130, 130), 7.0, device=dev)
        ops.se_kernel(a, a, std, lengthscale, 0.05, out=half, mirror=False, route="mfma")
        out[f"gp se d={d} lower no mirror"] = digest(half)


def gp_covariance(dev, out):
    """pg_gp_se_kernel and pg_gp_stat_kernel (every kind, shared / per-dimension lengthscales) through the C-ABI, both routes, in
    the four forms of gp(): cross into a strided out, symmetric mirrored, lower rows at diag_offset = 70, lower without mirror."""
    import torch
    from pytorch_generative_amd import _lib
    from pytorch_generative_amd.ops import gp as og

    lib, st = _lib.load(), torch.cuda.current_stream().cuda_stream
    n, m, std, noise = 130, 70, 1.3, 0.05
    sym = og.GP_LOWER | og.GP_DIAG
    for d in COV_D:
        g = torch.Generator().manual_seed(300 + d)
        a, b = strided(n, d, d + 3, g, dev), strided(m, d, d + 2, g, dev)
        lengthscale = 0.9 * d ** 0.5
        inv = (1.0 / (lengthscale * (0.5 + torch.rand(d, generator=g)))).to(dev)
        entries = [("se_kernel", None, None)] + [(f"stat {k} {'ard' if w is not None else 'shared'}", c, w)
                                                 for c, k in enumerate(GP_KINDS) for w in (None, inv)]
        for route, flag in (("direct", og.GP_SE_DIRECT), ("mfma", og.GP_SE_MFMA)):
            if route == "direct" and d > 64:
                continue
            for label, code, w in entries:
                def run(form, left, rows, right, cols, k, off, flags):
                    head = (left.data_ptr(), d + 3, rows, right.data_ptr(), right.stride(0), cols, d, std, lengthscale)
                    tail = (noise, k.data_ptr(), k.stride(0), off, flags | flag, st)
                    if code is None:
                        _lib.check(lib.pg_gp_se_kernel(*head, *tail), "pg_gp_se_kernel")
                    else:
                        _lib.check(lib.pg_gp_stat_kernel(code, *head, None if w is None else w.data_ptr(), *tail), "pg_gp_stat_kernel")
                    out[f"gp cov {label} d={d} {route} {form}"] = digest(k)

                run("cross", a, n, b, m, torch.full((n, m + 9), 7.0, device=dev), 0, 0)
                run("symmetric mirrored diag", a, n, a, n, torch.full((n, n), 7.0, device=dev), 0, sym | og.GP_MIRROR)
                run("lower rows diag_offset=70", a[70:], n - 70, a, n, torch.full((n - 70, n), 7.0, device=dev), 70, sym)
                run("lower no mirror", a, n, a, n, torch.full((n, n), 7.0, device=dev), 0, sym)


def gp_factor(n, pad, dev):
    """The lower factor of spd(n) in a buffer of row stride n + pad (7.0 beyond the row), by ops.cholesky_."""
    import torch
    from pytorch_generative_amd import ops

    buf = torch.full((n, n + pad), 7.0)
    buf[:, :n] = spd(n, 200 + n)
    buf = buf.to(dev)
    assert int(ops.cholesky_(buf[:, :n])) == 0
    return buf


def gp_inverse(dev, out):
    import torch
    from pytorch_generative_amd import ops

    for n in INVERSE_N:
        low = gp_factor(n, 3, dev)
        x = torch.full((n, n + 5), 7.0, device=dev)
        ops.tri_inverse_t(low[:, :n], out=x[:, :n])
        out[f"gp tri_inverse_t n={n}"] = digest(x)
        for mirror in (False, True):
            h = torch.full((n, n + 2), 7.0, device=dev)
            ops.gram_upper_(h[:, :n], x[:, :n], mirror=mirror)
            out[f"gp gram_upper n={n} mirror={mirror}"] = digest(h)


def gp_sums(dev, out):
    """pg_gp_se_mll_sums, pg_gp_stat_mll_sums and pg_gp_ard_mll_sums through the C-ABI on strided operands; the digests are of
    `out` and of the workspace rows the plan says are written. Then ops.mll_value."""
    import torch
    from pytorch_generative_amd import _lib, ops

    lib, st = _lib.load(), torch.cuda.current_stream().cuda_stream
    std = 1.3
    for ard, ds in ((False, SUMS_D), (True, ARD_D)):
        for n in SUMS_N:
            for d in ds:
                for p in (1, ops.gp_plan(n, 1, d, 1)["k_chunk"] + 1):
                    g = torch.Generator().manual_seed(n * 1000 + d * 10 + p)
                    x, at = strided(n, d, d + 3, g, dev), strided(p, n, n + 5, g, dev)
                    h = torch.randn(n, n, generator=g)
                    h = strided(n, n, n + 2, g, dev, fill=(h + h.t()) / n)
                    lengthscale = 0.9 * d ** 0.5
                    inv = (1.0 / (lengthscale * (0.5 + torch.rand(d, generator=g)))).to(dev)
                    floats = (ops.gp_ard_plan if ard else ops.gp_mll_plan)(n, d, p)["workspace_floats"]
                    entries = [(f"{'ard' if ard else 'stat'} {k}", c) for c, k in enumerate(GP_KINDS)] + ([] if ard else [("se_mll_sums", None)])
                    for label, code in entries:
                        ws, res = torch.full((floats + 4,), 7.0, device=dev), torch.full((d + 2 if ard else 3,), 7.0, device=dev)
                        head = (x.data_ptr(), d + 3, n, d, std)
                        tail = (h.data_ptr(), n + 2, at.data_ptr(), n + 5, p, ws.data_ptr(), floats, res.data_ptr(), st)
                        if ard:
                            _lib.check(lib.pg_gp_ard_mll_sums(code, *head, inv.data_ptr(), *tail), "pg_gp_ard_mll_sums")
                        elif code is None:
                            _lib.check(lib.pg_gp_se_mll_sums(*head, lengthscale, *tail), "pg_gp_se_mll_sums")
                        else:
                            _lib.check(lib.pg_gp_stat_mll_sums(code, *head, lengthscale, *tail), "pg_gp_stat_mll_sums")
                        out[f"gp sums {label} n={n} d={d} p={p} out"] = digest(res)
                        out[f"gp sums {label} n={n} d={d} p={p} workspace"] = digest(ws[:floats])
    for n in VALUE_N:
        low = gp_factor(n, 3, dev)
        for p in (1, ops.gp_plan(n, 1, 1, 1)["k_chunk"] + 1):
            g = torch.Generator().manual_seed(n * 10 + p)
            zt, at = strided(p, n, n + 1, g, dev), strided(p, n, n + 4, g, dev)
            out[f"gp mll_value n={n} p={p}"] = digest(ops.mll_value(low[:, :n], zt[:, :n], at[:, :n]))


def gp_models(dev, out):
    """Scalar SE, Matern 5/2 with a shared lengthscale and SE with per-dimension lengthscales, every hyperparameter a parameter:
    fit 65 rows, predict 70 queries, fit 65 more, predict, then the evidence and its gradients. Returns the routes seen."""
    import torch
    from torch import nn
    from pytorch_generative_amd.models import gaussian_process as gpm

    g = torch.Generator().manual_seed(12)
    x = 4.0 * torch.rand(130, 3, generator=g)
    y = (torch.sin(x.sum(1, keepdim=True)) + 0.3 * torch.randn(130, 1, generator=g)).to(dev)
    x, q = x.to(dev), (4.0 * torch.rand(70, 3, generator=g)).to(dev)
    par = lambda v: nn.Parameter(torch.tensor(v))
    kernels = {"se": lambda: gpm.SquaredExponential(par(1.3), par(0.7)), "matern52": lambda: gpm.Matern(2.5, par(1.3), par(0.7)),
               "se ard": lambda: gpm.SquaredExponential(par(1.3), par([0.7, 0.9, 1.2]))}
    routes = {}
    for name, make in kernels.items():
        model = gpm.GaussianProcess(gpm.Const(par(0.2)), make(), 0.1).to(dev)
        model.noise_var.requires_grad_()
        seen = [model._kernel_route]
        for step, (lo, hi) in enumerate(((0, 65), (65, 130))):
            model.fit(x[lo:hi], y[lo:hi])
            mu, sig = model.predict(q)
            out[f"gp model {name} predict {step} mu"], out[f"gp model {name} predict {step} sig"] = digest(mu), digest(sig)
            seen.append(model._factor_route)
        value = model.log_marginal_likelihood()
        value.backward()
        out[f"gp model {name} log p(y)"] = digest(value)
        for label, t in (("std", model.kernel.std), ("lengthscale", model.kernel.lengthscale), ("noise_var", model.noise_var),
                         ("value", model.mean.value)):
            out[f"gp model {name} d/d {label}"] = digest(t.grad)
        routes[name] = seen
    return routes


def compare(path_a, path_b, verdict_path):
    a, b = json.load(open(path_a)), json.load(open(path_b))
    da, db = a["digests"], b["digests"]
    differing = sorted(k for k in set(da) | set(db) if da.get(k) != db.get(k))
    verdict = {"a": a["library"], "b": b["library"], "cases": len(set(da) | set(db)), "differences": len(differing), "differing": differing}
    print(json.dumps(verdict))
    if verdict_path:
        json.dump(verdict, open(verdict_path, "w"), indent=1)
    return 1 if differing or not da else 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--label", default=None, help="what the record calls the library, e.g. the commit it was built from")
    ap.add_argument("--compare", nargs=2, metavar=("A.json", "B.json"))
    ap.add_argument("--verdict", default=None)
    ap.add_argument("--package", default=None, metavar="DIR", help="import pytorch_generative_amd from DIR, not from the working tree")
    a = ap.parse_args()
    if a.compare:
        sys.exit(compare(a.compare[0], a.compare[1], a.verdict))
    if a.package:
        sys.path[0] = os.path.abspath(a.package)
    import torch
    from pytorch_generative_amd import _lib

    assert torch.cuda.is_available() and a.out, "tile_bits needs the MI355X and --out"
    dev = torch.device("cuda:0")
    digests = {}
    rec = {"library": a.label or os.path.basename(_lib.LIB_PATH), "device": torch.cuda.get_device_name(0), "dense_plan_branches": dense(dev, digests), "fvbn_plan_branches": fvbn(dev, digests)}
    gp(dev, digests)
    gp_covariance(dev, digests)
    gp_inverse(dev, digests)
    gp_sums(dev, digests)
    rec["gp_model_routes"] = gp_models(dev, digests)
    rec["package"] = os.path.dirname(os.path.dirname(os.path.abspath(_lib.__file__)))
    rec["digests"] = digests
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(rec, open(a.out, "w"), indent=1)
    print(f"wrote {a.out}: {len(digests)} digests")


if __name__ == "__main__":
    main()
