"""Do two builds of the library give the same bits on the fp32-MFMA tile kernels (csrc/mfma_tile.h: dense_linear, fvbn, gp)?

    PG_HIP_LIB=<library A> timeout -k 10 240 python tools/tile_bits.py --label A --out A.json \\
      && PG_HIP_LIB=<library B> timeout -k 10 240 python tools/tile_bits.py --label B --out B.json \\
      && python tools/tile_bits.py --compare A.json B.json [--verdict verdict.json]   # exit code 1 on any difference

One process per library (_lib loads one only), each under its own time limit, chained so that nothing starts after a failure.
The other library is built from an earlier commit with build.py's flags, outside the tree:
    mkdir -p /tmp/pg_parent && git archive <commit> pytorch-generative_amd/build.py pytorch-generative_amd/csrc include \\
      | tar -x -C /tmp/pg_parent && python /tmp/pg_parent/pytorch-generative_amd/build.py
    # -> /tmp/pg_parent/pytorch-generative_amd/pytorch_generative_amd/lib/libpg_hip.so

For a fixed list of cases the inputs come from seeded CPU generators, the entry points run once and the JSON holds the sha256 of
every output's raw bytes. The cases are the shape lists with which the GPU tests reach every branch of the three plans
(tests/test_gpu_nice.py DIRECT_SHAPES and its two extra weight-gradient shapes, tests/test_gpu_fvbn.py SHAPES,
tests/test_gpu_gp.py FACTOR_N, its append pairs, its GEMM update and its covariance at d = 17, 40); the dense list is checked
against pg_dense_linear_plan to reach small-unsplit, small-k-split and large for every kind, and the record says so."""

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
    a = ap.parse_args()
    if a.compare:
        sys.exit(compare(a.compare[0], a.compare[1], a.verdict))
    import torch
    from pytorch_generative_amd import _lib

    assert torch.cuda.is_available() and a.out, "tile_bits needs the MI355X and --out"
    dev = torch.device("cuda:0")
    digests = {}
    rec = {"library": a.label or os.path.basename(_lib.LIB_PATH), "device": torch.cuda.get_device_name(0), "dense_plan_branches": dense(dev, digests), "fvbn_plan_branches": fvbn(dev, digests)}
    gp(dev, digests)
    rec["digests"] = digests
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(rec, open(a.out, "w"), indent=1)
    print(f"wrote {a.out}: {len(digests)} digests")


if __name__ == "__main__":
    main()
