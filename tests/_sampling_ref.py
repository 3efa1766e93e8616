"""Float64 restatement of the two kernels of incremental sampling (csrc/sampling.hip), from the contract in
include/pg_hip.h ("Incremental autoregressive sampling") — plain torch, no GPU. tests/test_sampling_ref_cpu.py pins
it against oracle.ops and torch's conv2d, tests/test_gpu_sampling_kernels.py compares the kernels with it.

`dtype` exists so that the CPU tier can run the very same statement in float32 and check that the project's
tolerances hold for a correct fp32 evaluation of the chosen inputs; the reference itself is the float64 default.
The input builders at the end are shared by the CPU and the GPU tier, so both look at the same numbers."""

import math

import torch

L_DECODE = 130                    # crosses the 64-lane stride of the decode kernel twice
P_SINGLE = (0, 1, 63, 64, 65, 127, 128, 129)
DECODE_SHAPES = [                 # (heads, dk, dv)
    (4, 4, 4),
    (3, 2, 3),
    (1, 1, 1),
    (2, 5, 4),                    # the 32 template through dk alone
    (2, 4, 5),                    # ... through dv alone
    (1, 16, 16),
    (2, 32, 32),
    (1, 7, 29),
]
SENTINEL = -12345.678             # finite: torch.equal works, and a key / value read from it wrecks the output
GARBAGE = 1.0e30                  # padding columns of qkv


def decode_step(qkv, k_cache, v_cache, N, heads, L, p, dk, dv, ld, strict, o=None, dtype=torch.float64):
    """One pg_attn_decode call. qkv: (2 * heads * dk + heads * dv, ld), rows [q | k | v], column n = sample n.
    Returns (o, k_cache', v_cache'): the caches (N, heads * dk, L) / (N, heads * dv, L) with column p replaced by the
    k / v rows of qkv, and o[(h * dv + c), n] = softmax_{j <= p - strict}(q . k_j / sqrt(dk)) v_j over the NEW caches
    (0 when no key is admitted). Columns n >= N of `o` (zeros if not given) are left as given."""
    E, V = heads * dk, heads * dv
    assert qkv.shape == (2 * E + V, ld) and k_cache.shape == (N, E, L) and v_cache.shape == (N, V, L)
    assert 0 <= p < L and N <= ld and strict in (0, 1)
    cols = qkv[:, :N].to(dtype)
    kc, vc = k_cache.to(dtype).clone(), v_cache.to(dtype).clone()
    kc[:, :, p] = cols[E:2 * E].t()
    vc[:, :, p] = cols[2 * E:].t()
    out = torch.zeros(V, ld, dtype=dtype) if o is None else o.to(dtype).clone()
    last = p - strict                                   # admitted keys: j = 0 .. last
    if last < 0:
        out[:, :N] = 0
        return out, kc, vc
    q = cols[:E].t().reshape(N, heads, dk)
    keys = kc[:, :, :last + 1].reshape(N, heads, dk, last + 1)
    vals = vc[:, :, :last + 1].reshape(N, heads, dv, last + 1)
    s = torch.einsum("nhd,nhdj->nhj", q, keys) / math.sqrt(dk)
    w = torch.softmax(s, dim=-1)
    out[:, :N] = torch.einsum("nhj,nhcj->nhc", w, vals).reshape(N, V).t()
    return out, kc, vc


def embed_pixel(canvas, pos, w, b, r, c, ld, out=None, dtype=torch.float64):
    """One pg_sample_embed call: out[co, n] = b[co] + sum_{ci,u,v} w[co, ci, u, v] * xin[n, ci, r + u - KH // 2,
    c + v - KW // 2], xin = canvas + pos inside the image and 0 outside. pos (Cin, H, W) and b (Cout) may be None.
    Returns (Cout, ld); columns n >= N are those of `out` (zeros if not given)."""
    N, Cin, H, W = canvas.shape
    Cout, _, KH, KW = w.shape
    assert w.shape[1] == Cin and 0 <= r < H and 0 <= c < W and N <= ld
    xin = canvas.to(dtype)
    if pos is not None:
        xin = xin + pos.to(dtype).reshape(1, Cin, H, W)
    w = w.to(dtype)
    res = torch.zeros(Cout, ld, dtype=dtype) if out is None else out.to(dtype).clone()
    acc = torch.zeros(Cout, N, dtype=dtype)
    if b is not None:
        acc += b.to(dtype).reshape(Cout, 1)
    for ci in range(Cin):
        for u in range(KH):
            rr = r + u - KH // 2
            if rr < 0 or rr >= H:
                continue
            for v in range(KW):
                cc = c + v - KW // 2
                if cc < 0 or cc >= W:
                    continue
                acc += w[:, ci, u, v].reshape(Cout, 1) * xin[:, ci, rr, cc].reshape(1, N)
    res[:, :N] = acc
    return res


# ---------------------------------------------------------------------------------------------
# inputs shared by the CPU tier (fp32-restatement check of the tolerances) and the GPU tier
def _gen(*key):
    seed = 0
    for k in key:
        seed = (seed * 1000003 + int(k) + 1) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(seed)


def decode_qkv(heads, dk, dv, N, ld, seed):
    """Seeded-normal qkv (fp32), padding columns n >= N = GARBAGE."""
    rows = 2 * heads * dk + heads * dv
    qkv = torch.full((rows, ld), GARBAGE)
    qkv[:, :N] = torch.randn(rows, N, generator=_gen(heads, dk, dv, N, seed))
    return qkv


def decode_caches(heads, dk, dv, N, L, p, seed):
    """Caches pre-filled for j < p from a seeded normal, SENTINEL in every column j >= p (fp32)."""
    g = _gen(heads, dk, dv, N, L, seed, 7)
    kc = torch.full((N, heads * dk, L), SENTINEL)
    vc = torch.full((N, heads * dv, L), SENTINEL)
    kc[:, :, :p] = torch.randn(N, heads * dk, L, generator=g)[:, :, :p]
    vc[:, :, :p] = torch.randn(N, heads * dv, L, generator=g)[:, :, :p]
    return kc, vc


def decode_sequence_qkv(heads, dk, dv, N, ld, L, seed):
    """(L, rows, ld): a fresh qkv for every step of a whole-sequence run."""
    rows = 2 * heads * dk + heads * dv
    qkv = torch.full((L, rows, ld), GARBAGE)
    qkv[:, :, :N] = torch.randn(L, rows, N, generator=_gen(heads, dk, dv, N, L, seed, 11))
    return qkv


def decode_sequence_ref(qkv_seq, N, heads, L, dk, dv, ld, strict, dtype=torch.float64):
    """decode_step for p = 0 .. L-1 from zeroed caches; returns (o (L, V, N), k_cache, v_cache)."""
    kc = torch.zeros(N, heads * dk, L, dtype=dtype)
    vc = torch.zeros(N, heads * dv, L, dtype=dtype)
    outs = []
    for p in range(L):
        o, kc, vc = decode_step(qkv_seq[p], kc, vc, N, heads, L, p, dk, dv, ld, strict, dtype=dtype)
        outs.append(o[:, :N])
    return torch.stack(outs), kc, vc


def spike_case(heads, dk, dv, N, ld, L, p, score, where, seed):
    """Softmax-rescale inputs for step p: every key scores ~0 against q except ONE that scores `score`:
    where = "cache": the key cached at position 3 (keys after it are near 0, so the running maximum falls behind);
    where = "self":  the key of position p itself (the kernel's lane-0 register term, after lane 0's cached keys).
    Returns (qkv, k_cache, v_cache), caches filled for j < p and SENTINEL from p on."""
    g = _gen(heads, dk, dv, N, p, seed, 13)
    E, V = heads * dk, heads * dv
    qkv = torch.full((2 * E + V, ld), GARBAGE)
    q = torch.randn(E, N, generator=g)
    qh = q.reshape(heads, dk, N)
    spike = (qh * (score * math.sqrt(dk)) / (qh * qh).sum(1, keepdim=True)).reshape(E, N)  # q . spike / sqrt(dk) = score
    qkv[:E, :N] = q
    qkv[E:2 * E, :N] = spike if where == "self" else 0.01 * torch.randn(E, N, generator=g)
    qkv[2 * E:, :N] = torch.randn(V, N, generator=g)
    kc = torch.full((N, E, L), SENTINEL)
    vc = torch.full((N, V, L), SENTINEL)
    kc[:, :, :p] = 0.01 * torch.randn(N, E, L, generator=g)[:, :, :p]
    vc[:, :, :p] = torch.randn(N, V, L, generator=g)[:, :, :p]
    if where == "cache":
        assert p > 3
        kc[:, :, 3] = spike.t()
    return qkv, kc, vc


def onehot_value_step(heads, dk, dv, N, ld, p):
    """Admitted-set probe: q = k = 0 and the value of position p one-hot: sample n, channel j (of every head) marks key
    n * dv + j. After the step, o[h * dv + j, n] = P[p, n * dv + j] = 1 / count(p) on admitted keys, 0 elsewhere."""
    E, V = heads * dk, heads * dv
    qkv = torch.full((2 * E + V, ld), GARBAGE)
    qkv[:, :N] = 0
    n, j = divmod(p, dv)
    for h in range(heads):
        qkv[2 * E + h * dv + j, n] = 1.0
    return qkv


EMBED_HW = (4, 5)
EMBED_KERNELS = [(3, 3), (1, 1), (5, 3), (2, 2)]


def embed_inputs(N, Cin, Cout, KH, KW, seed=0):
    """canvas (N, Cin, 4, 5), pos (Cin, 4, 5), w (Cout, Cin, KH, KW) UNMASKED (every tap contributes), b (Cout) — fp32."""
    H, W = EMBED_HW
    g = _gen(N, Cin, Cout, KH, KW, seed, 17)
    canvas = torch.randn(N, Cin, H, W, generator=g)
    pos = 0.5 * torch.randn(Cin, H, W, generator=g)
    w = torch.randn(Cout, Cin, KH, KW, generator=g)
    b = torch.randn(Cout, generator=g)
    return canvas, pos, w, b
