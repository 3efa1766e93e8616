"""float64 restatement of the contract of pg_attn_row (include/pg_hip.h), written from its formula, and the shared cases of
tests/test_attn_row_cpu.py and tests/test_gpu_attn_row.py.

Query column x of row r admits every cache key of rows y < r, the keys x' < x of row r, and x' == x when mask_center is 0;
row r's own keys and values come from kv_row. o = sum_j softmax_j(q . k_j / sqrt(dk)) v_j, 0 when nothing is admitted."""

import math

import torch

PLAN_INTS = 6
TOL = 1e-5  # the project's bound for the sampler kernels (_util.assert_close)

# (N, heads, dk, dv, H, W) of the GPU tier
SHAPES = [
    (2, 1, 4, 32, 3, 5),     # the recipe's head
    (5, 3, 5, 7, 4, 7),      # odd, unaligned
    (1, 1, 4, 16, 1, 1),     # a single pixel: exact zeros with mask_center
    (2, 2, 3, 4, 4, 1),
    (2, 1, 4, 32, 3, 65),    # a row longer than a wave
    (1, 1, 64, 128, 2, 3),   # domain edge
]


def attn_row_ref(q_row, kv_row, k_cache, v_cache, heads, r, mask_center, dtype=torch.float64):
    """(o_row, k_cache', v_cache') in `dtype`: the output of the row and the caches after a write_cache launch. Plain loops
    over sample, head and query; cache rows >= r are never touched by the arithmetic."""
    q_row, kv_row, k_cache, v_cache = (t.detach().cpu().to(dtype) for t in (q_row, kv_row, k_cache, v_cache))
    n, e, _, w = q_row.shape
    o = v_cache.shape[1]
    dk, dv = e // heads, o // heads
    out = torch.zeros(n, o, 1, w, dtype=dtype)
    for i in range(n):
        for h in range(heads):
            q = q_row[i, h * dk:(h + 1) * dk, 0]                       # (dk, W)
            k_new = kv_row[i, h * dk:(h + 1) * dk, 0]                  # (dk, W)
            v_new = kv_row[i, e + h * dv:e + (h + 1) * dv, 0]          # (dv, W)
            k_old = k_cache[i, h * dk:(h + 1) * dk, :r].reshape(dk, -1)  # (dk, r W)
            v_old = v_cache[i, h * dv:(h + 1) * dv, :r].reshape(dv, -1)
            for x in range(w):
                own = x if mask_center else x + 1
                keys = torch.cat((k_old, k_new[:, :own]), dim=1)
                vals = torch.cat((v_old, v_new[:, :own]), dim=1)
                if keys.shape[1] == 0:
                    continue
                s = (q[:, x] @ keys) / math.sqrt(dk)
                p = torch.exp(s - s.max())
                out[i, h * dv:(h + 1) * dv, 0, x] = (vals @ p) / p.sum()
    kc, vc = k_cache.clone(), v_cache.clone()
    kc[:, :, r] = kv_row[:, :e, 0]
    vc[:, :, r] = kv_row[:, e:, 0]
    return out, kc, vc


def case(shape, seed=0, scale=1.0):
    """Seeded float32 operands of a whole image: q (N, E, H, W), kv (N, E + V, H, W). Row r of them is a launch's input, rows
    < r its caches."""
    n, heads, dk, dv, h, w = shape
    g = torch.Generator().manual_seed(1000 + seed)
    q = torch.randn(n, heads * dk, h, w, generator=g) * scale
    kv = torch.randn(n, heads * (dk + dv), h, w, generator=g)
    kv[:, :heads * dk] *= scale
    return q, kv


def row_inputs(q, kv, e, r, fill=0.0):
    """(q_row, kv_row, k_cache, v_cache) of row r: caches hold rows < r of the image and `fill` (e.g. NaN) from row r on."""
    k_cache, v_cache = kv[:, :e].clone(), kv[:, e:].clone()
    k_cache[:, :, r:] = fill
    v_cache[:, :, r:] = fill
    return q[:, :, r:r + 1].contiguous(), kv[:, :, r:r + 1].contiguous(), k_cache, v_cache


def spike_case(shape, where, seed=0):
    """Scores of size about 80: every query lies (up to small noise) along one direction u with norm sqrt(80 sqrt(dk)), and
    so does the ONE key at pixel `where` = (row, col): its score with every query is ~80, the other keys' (unit normal) are
    of order +-sqrt(80)/dk^(1/4). Queries that admit the spiked key put all their weight on it (to ~e^-50); the running
    maximum of a query jumps by ~100 (in the exp2 domain) where the spike enters."""
    n, heads, dk, dv, h, w = shape
    g = torch.Generator().manual_seed(2000 + seed)
    amp = math.sqrt(80.0 * math.sqrt(dk))
    u = torch.randn(dk, generator=g)
    u = u / u.norm()
    base = (amp * u).repeat(heads).view(1, heads * dk, 1, 1)
    q = base + 0.05 * torch.randn(n, heads * dk, h, w, generator=g)
    kv = torch.randn(n, heads * (dk + dv), h, w, generator=g)
    kv[:, :heads * dk, where[0], where[1]] = base[:, :, 0, 0]
    return q, kv
