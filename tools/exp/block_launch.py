"""A few launches of the GPT-block kernels (csrc/gpt_block.hip: head / tail forward and backward, the fused tail + next head
forward and the fused next head + tail backward) at the bench's batch, through the C-ABI, for rocprofv3 counter
passes (--pmc alone, never combined with a trace domain) and for a library A/B (PG_HIP_LIB=<other build>):

    python tools/exp/block_launch.py [launches] [batch]

Each kernel is launched `launches` times in a row, once untimed first; prints the HIP-event time per launch as one JSON line (the
backward figures include the small reduce launch that follows the kernel). The launches of one kernel run back to back on the same
buffers, so a working set under 256 MB (head_fwd, tail_fwd at batch 1024) is served from the Infinity Cache: the timings rank builds of
one kernel against each other and are lower than the kernel's cost inside a training step."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "pytorch-generative_amd")]
import torch  # noqa: E402

from pytorch_generative_amd import _lib  # noqa: E402

launches = int(sys.argv[1]) if len(sys.argv) > 1 else 3
n = int(sys.argv[2]) if len(sys.argv) > 2 else 1024
L, eps = 784, 1e-5
lib = _lib.load()
dev = torch.device("cuda:0")
torch.manual_seed(0)
r = lambda *s: torch.randn(*s, device=dev)  # noqa: E731
x, o, d, gx, dqkv = r(n, 16, L), r(n, 16, L), r(n, 16, L), r(n, 16, L), r(n, 48, L)
qkv, xnew, d_o, gxo, dx = (torch.empty(n, c, L, device=dev) for c in (48, 16, 16, 16, 16))
qkv2, xnew2 = torch.empty(n, 48, L, device=dev), torch.empty(n, 16, L, device=dev)  # the fused launch's own outputs
d_o2, gxo2 = torch.empty(n, 16, L, device=dev), torch.empty(n, 16, L, device=dev)
g1, be1, wq, bq, wkv, bkv = r(16), r(16), r(16, 16) * .2, r(16), r(32, 16) * .2, r(32)
wp, bp, g2, be2, w1, b1, w2, b2 = r(16, 16) * .2, r(16), r(16), r(16), r(64, 16) * .2, r(64), r(16, 64) * .1, r(16)
G = {k: torch.zeros_like(v) for k, v in dict(g1=g1, be1=be1, wq=wq, bq=bq, wkv=wkv, bkv=bkv, wp=wp, bp=bp, g2=g2, be2=be2, w1=w1,
                                            b1=b1, w2=w2, b2=b2).items()}
hn, tn = lib.pg_gpt_block_head_bwd_workspace_floats(n, L), lib.pg_gpt_block_tail_bwd_workspace_floats(n, L)
hws, tws = torch.zeros(hn, device=dev), torch.zeros(tn, device=dev)
st = torch.cuda.current_stream().cuda_stream
p = lambda t: t.data_ptr()  # noqa: E731
calls = {
    "head_fwd": lambda: lib.pg_gpt_block_head_fwd(p(x), p(g1), p(be1), p(wq), p(bq), p(wkv), p(bkv), p(qkv), n, 16, L, eps, st),
    "tail_fwd": lambda: lib.pg_gpt_block_tail_fwd(p(o), p(x), p(wp), p(bp), p(g2), p(be2), p(w1), p(b1), p(w2), p(b2), p(xnew),
                                                  n, 16, 64, L, eps, st),
    # tail of a block + head of the next one (the head's parameters stand in for the next block's)
    "tail_head_fwd": lambda: lib.pg_gpt_block_tail_head_fwd(p(o), p(x), p(wp), p(bp), p(g2), p(be2), p(w1), p(b1), p(w2), p(b2),
                                                            p(xnew2), p(g1), p(be1), p(wq), p(bq), p(wkv), p(bkv), p(qkv2),
                                                            n, 16, 64, L, eps, st),
    "tail_bwd": lambda: lib.pg_gpt_block_tail_bwd(p(o), p(x), p(wp), p(bp), p(g2), p(be2), p(w1), p(b1), p(w2), p(d), p(d_o), p(gxo),
                                                  p(G["wp"]), p(G["bp"]), p(G["g2"]), p(G["be2"]), p(G["w1"]), p(G["b1"]), p(G["w2"]),
                                                  p(G["b2"]), n, 16, 64, L, eps, p(tws), tn, st),
    "head_bwd": lambda: lib.pg_gpt_block_head_bwd(p(x), p(g1), p(be1), p(wq), p(wkv), p(dqkv), p(gx), p(dx), p(G["g1"]), p(G["be1"]),
                                                  p(G["wq"]), p(G["bq"]), p(G["wkv"]), p(G["bkv"]), n, 16, L, eps, p(hws), hn, st),
    # the backward boundary without any reduce launch: the two kernels on their own, then both chains in one launch (x and the
    # head's parameters stand in for the next block's; d_o2 / gxo2 are the fused launch's own outputs)
    "tail_bwd_partial": lambda: lib.pg_gpt_block_tail_bwd_partial(p(o), p(x), p(wp), p(bp), p(g2), p(be2), p(w1), p(b1), p(w2), p(d),
                                                                  p(d_o), p(gxo), n, 16, 64, L, eps, p(tws), tn, st),
    "head_bwd_partial": lambda: lib.pg_gpt_block_head_bwd_partial(p(x), p(g1), p(be1), p(wq), p(wkv), p(dqkv), p(gx), p(dx), n, 16, L,
                                                                  eps, p(hws), hn, st),
    "head_tail_bwd_partial": lambda: lib.pg_gpt_block_head_tail_bwd_partial(
        p(x), p(g1), p(be1), p(wq), p(wkv), p(dqkv), p(gx), p(o), p(x), p(wp), p(bp), p(g2), p(be2), p(w1), p(b1), p(w2), p(d_o2),
        p(gxo2), n, 16, 64, L, eps, p(hws), hn, p(tws), tn, st),
}
out = {"launches": launches, "batch": n, "lib": os.path.basename(_lib.LIB_PATH)}
for name, fn in calls.items():
    assert fn() == 0, name
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(launches):
        fn()
    e1.record()
    torch.cuda.synchronize()
    out[name + "_us"] = round(e0.elapsed_time(e1) * 1e3 / launches, 2)
print(json.dumps(out))
