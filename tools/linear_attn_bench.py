"""LinearCausalAttention vs CausalAttention on the MI355X: forward + backward times, bytes and FLOP per C-ABI call of the
linear-attention core, and the core's fraction of the roofline.

usage: python tools/linear_attn_bench.py [--out profiles/linear_attention.json] [--iters 20] [--warmup 5]

Shapes: N = 64, C = 64 (embed = out = 64), heads 1 and 4, 32 x 32 and 64 x 64 images. Times are HIP-event medians on
the current stream after warm-up. `module_*`: the whole nn module (1x1 projections included; CausalAttention also
runs its output projection, LinearCausalAttention has none — as in the reference). `core_*`: one pg_linear_attn_fwd /
pg_linear_attn_bwd call (ops.linear_causal_attention forward / its backward). Bytes and FLOP are the algorithm's
(computed from the shapes below, not counted by the hardware): every tensor read or written once plus the chunk-state
traffic of the two-pass scan (states written, read and rewritten by the prefix, read again), and the FLOP of the
chunked products as executed (intra-chunk score tiles counted in full). Roofline: the larger of bytes / 8 TB/s and
FLOP / 157.3 TF/s (the fp32 MFMA peak) over the measured time.
"""

import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pytorch-generative_amd"))
import torch  # noqa: E402

from pytorch_generative_amd import nn as pg_nn, ops  # noqa: E402

T = 64  # positions per chunk (csrc/linear_attention.hip LA_T)
HBM_PEAK = 8.0e12
F32_PEAK = 157.3e12


def model(n, heads, L, dk, dv):
    """Algorithmic bytes / FLOP of one forward and one backward C-ABI call."""
    nh, nch = n * heads, -(-L // T)
    st = 4 * nh * nch * dk * dv if nch > 1 else 0  # one pass over the chunk states
    scan_flop = nh * nch * (2 * T * T * dk + 2 * T * dk * dv + 2 * T * T * dv + 2 * T * dk * dv)  # Sm, A P, Sm C, state
    fwd_bytes = 4 * nh * L * (2 * dk + dv) + 4 * nh * L * (dv + 1) + 4 * st
    fwd_flop = scan_flop + nh * L * 4 * dk
    # backward: reads q, k, v, out, g, den; writes dq, dk, dv; gs round trip; three scans
    bwd_bytes = 4 * nh * L * (2 * dk + dv + 2 * dv + 1) + 4 * nh * L * (2 * dk + dv) + 8 * nh * L + 12 * st
    bwd_flop = 3 * scan_flop + nh * L * (2 * dv + 8 * dk)
    return fwd_bytes, fwd_flop, bwd_bytes, bwd_flop


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


def roof(bytes_, flop, ms):
    t = ms * 1e-3
    tb, tf = bytes_ / HBM_PEAK, flop / F32_PEAK
    return {"bytes": int(bytes_), "flop": int(flop), "achieved_gbps": bytes_ / t / 1e9, "achieved_tflops": flop / t / 1e12,
            "roofline_fraction": max(tb, tf) / t, "bound": "hbm" if tb >= tf else "fp32_mfma"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "linear_attention.json"))
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "linear_attn_bench needs the MI355X"
    dev = torch.device("cuda:0")
    n, c = 64, 64
    rows = []
    for hw in (32, 64):
        for heads in (1, 4):
            L, d = hw * hw, c // heads
            g = torch.Generator().manual_seed(0)
            x = torch.randn(n, c, hw, hw, generator=g).to(dev).requires_grad_(True)
            dy = torch.randn(n, c, hw, hw, generator=g).to(dev)
            torch.manual_seed(0)
            lin = pg_nn.LinearCausalAttention(c, n_heads=heads).to(dev)
            ca = pg_nn.CausalAttention(c, n_heads=heads).to(dev)

            def step(m):
                def f():
                    x.grad = None
                    m(x).backward(dy)
                return f

            q = torch.randn(n, c, hw, hw, generator=g).to(dev).requires_grad_(True)
            kv = torch.randn(n, 2 * c, hw, hw, generator=g).to(dev).requires_grad_(True)

            def core_fwd():
                with torch.no_grad():
                    ops.linear_causal_attention(q, kv, heads, c, c)

            o = ops.linear_causal_attention(q, kv, heads, c, c)

            def core_bwd():  # one pg_linear_attn_bwd call (the saved forward is reused)
                torch.autograd.grad(o, (q, kv), dy, retain_graph=True)

            row = {"N": n, "C": c, "H": hw, "W": hw, "L": L, "heads": heads, "dk": d, "dv": d,
                   "linear_module_fwd_bwd_ms": timed(step(lin), a.iters, a.warmup),
                   "causal_module_fwd_bwd_ms": timed(step(ca), a.iters, a.warmup),
                   "core_fwd_ms": timed(core_fwd, a.iters, a.warmup),
                   "core_bwd_ms": timed(core_bwd, a.iters, a.warmup)}
            fb, ff, bb, bf = model(n, heads, L, d, d)
            row["core_fwd"] = roof(fb, ff, row["core_fwd_ms"])
            row["core_bwd"] = roof(bb, bf, row["core_bwd_ms"])
            row["linear_over_causal"] = row["linear_module_fwd_bwd_ms"] / row["causal_module_fwd_bwd_ms"]
            print(json.dumps(row), flush=True)
            rows.append(row)
            del lin, ca, x, dy, q, kv, o
            torch.cuda.empty_cache()
    rec = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "iters": a.iters, "warmup": a.warmup,
           "peaks": {"hbm_bytes_per_s": HBM_PEAK, "fp32_flop_per_s": F32_PEAK}, "chunk": T, "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
    print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
