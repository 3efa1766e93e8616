"""VectorQuantizer forward + backward on the MI355X, in both codebook modes and at two widths.

usage: python tools/vq_bench.py [--out profiles/vq.json] [--iters 50] [--warmup 10]

* `graphed_ms`: one quantizer forward + backward of `q.sum() * 0.5 + loss` (for the EMA codebook the update inside the
  training forward, for the gradient-trained codebook its gradient) captured once and replayed from a hipGraph;
  HIP-event median after warm-up. Shapes: the VQ-VAE recipe's quantizer input 128 x 64 x 8 x 8 with K = 512 (P = 8192
  positions), and the same with D = 128 (the tiled assignment).
* `eager_torch_reference_ms`: FOR COMPARISON ONLY, the reference's algorithm (nn/utils.py:53-96: the P x K distance matrix,
  argmin, one-hot matmuls, autograd) in eager torch-ROCm on the same GPU.
* `assign_d64`: the two assignment entry points alone at the recipe's shape, each replayed from a hipGraph: pg_vq_assign
  (one position per thread, D <= 64) against pg_vq_assign_tiled (fp32-MFMA tiles, any D), and whether their indices agree.
  This is the measurement behind the routing of widths up to 64 (nn/utils.py TILED_MIN_DIM).
"""

import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pytorch-generative_amd"))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

N, HW, K = 128, 8, 512


def timed(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        torch.cuda.synchronize()
        ts.append(s.elapsed_time(e))
    return statistics.median(ts)


def graphed(fn):
    """Captures fn() after three warm-up calls on a side stream; returns the replay."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fn()
    return g.replay


def inputs(d, dev):
    g = torch.Generator().manual_seed(d)
    return torch.randn(N, d, HW, HW, generator=g).to(dev)


def quantizer_step(d, use_ema, dev):
    import pytorch_generative_amd as pg

    torch.manual_seed(0)
    m = pg.nn.VectorQuantizer(K, d, use_ema=use_ema).to(dev)
    m.train()
    x = inputs(d, dev).requires_grad_(True)

    def f():
        x.grad = None
        if not use_ema:
            m._embedding.grad = None
        q, loss = m(x)
        (q.sum() * 0.5 + loss).backward()

    return f


def eager_reference_step(d, use_ema, dev):
    torch.manual_seed(0)
    emb = torch.zeros(K, d)
    torch.nn.init.kaiming_uniform_(emb, nonlinearity="linear")
    emb = emb.to(dev).requires_grad_(not use_ema)
    cluster, avg = torch.zeros(K, device=dev), emb.detach().clone()
    x = inputs(d, dev).requires_grad_(True)

    def f():
        x.grad = None
        emb.grad = None
        n, c, h, w = x.shape
        flat = x.permute(0, 2, 3, 1).contiguous().view(-1, c)
        dist = torch.sum(flat ** 2, dim=1, keepdim=True) + torch.sum(emb ** 2, dim=1) - 2 * flat @ emb.t()
        idxs = torch.argmin(dist, dim=1, keepdim=True)
        one_hot = torch.zeros(idxs.shape[0], K, device=dev)
        one_hot.scatter_(1, idxs, 1)
        q = (one_hot @ emb).view(n, h, w, c).permute(0, 3, 1, 2).contiguous()
        loss = F.mse_loss(x, q.detach())
        if use_ema:
            cluster.mul_(0.99).add_(one_hot.sum(axis=0), alpha=0.01)
            avg.mul_(0.99).add_((flat.t() @ one_hot).t().detach(), alpha=0.01)
            emb.data.copy_(avg / (cluster + 1e-5).unsqueeze(1))
        else:
            loss = loss + F.mse_loss(q, x.detach())
        q = x + (q - x).detach()
        (q.sum() * 0.5 + loss).backward()

    return f


def assign_pair(dev, iters, warmup):
    from pytorch_generative_amd import _lib, ops

    lib = _lib.load()
    d = 64
    x = inputs(d, dev)
    torch.manual_seed(0)
    emb = torch.zeros(K, d)
    torch.nn.init.kaiming_uniform_(emb, nonlinearity="linear")
    emb = emb.to(dev)
    out = {}
    idxs = {}
    for name in ("pg_vq_assign", "pg_vq_assign_tiled"):
        idx = torch.empty(N * HW * HW, device=dev, dtype=torch.int32)
        q, st = torch.empty_like(x), torch.empty_like(x)
        loss = torch.zeros(1, device=dev)
        fn = getattr(lib, name)

        def f(fn=fn, idx=idx, q=q, st=st, loss=loss, name=name):
            _lib.check(fn(x.data_ptr(), emb.data_ptr(), idx.data_ptr(), q.data_ptr(), st.data_ptr(), loss.data_ptr(),
                          N, d, HW * HW, K, ops._stream()), name)

        out[name + "_ms"] = timed(graphed(f), iters, warmup)
        idxs[name] = idx.clone()
    out["indices_equal"] = bool(torch.equal(idxs["pg_vq_assign"], idxs["pg_vq_assign_tiled"]))
    out["positions_differing"] = int((idxs["pg_vq_assign"] != idxs["pg_vq_assign_tiled"]).sum())
    out["tiled_over_per_thread"] = out["pg_vq_assign_tiled_ms"] / out["pg_vq_assign_ms"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vq.json"))
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "vq_bench needs the MI355X"
    assert a.iters >= 20, "median over at least 20 replays"
    dev = torch.device("cuda:0")
    from pytorch_generative_amd.nn import utils as nn_utils

    rows = []
    for d in (64, 128):
        for use_ema in (True, False):
            row = {"x": [N, d, HW, HW], "K": K, "positions": N * HW * HW, "codebook": "ema" if use_ema else "gradient",
                   "assign_kernel": "pg_vq_assign_tiled" if d >= nn_utils.TILED_MIN_DIM else "pg_vq_assign",
                   "graphed_ms": timed(graphed(quantizer_step(d, use_ema, dev)), a.iters, a.warmup),
                   "eager_ms": timed(quantizer_step(d, use_ema, dev), a.iters, a.warmup),
                   "eager_torch_reference_ms": timed(eager_reference_step(d, use_ema, dev), a.iters, a.warmup)}
            row["speedup_vs_eager_torch"] = row["eager_torch_reference_ms"] / row["graphed_ms"]
            print(json.dumps(row), flush=True)
            rows.append(row)
    pair = assign_pair(dev, a.iters, a.warmup)
    print(json.dumps(pair), flush=True)
    rec = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "iters": a.iters, "warmup": a.warmup,
           "rows": rows, "assign_d64": pair, "tiled_min_dim": nn_utils.TILED_MIN_DIM}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
    print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
