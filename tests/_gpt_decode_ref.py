"""Float64 restatement of one K/V-cached decode step over ALL transformer blocks of ImageGPT (csrc/gpt_decode.hip), written
from oracle.models.image_gpt and oracle.ops — plain torch, no GPU. tests/test_gpt_decode_ref_cpu.py pins it against the
oracle's full forward; tests/test_gpu_gpt_decode.py compares the kernel with it.

`dtype` exists so that the CPU tier can run the very same statement in float32 and check that the GPU tier's bounds hold
for a correct fp32 evaluation of the inputs used there; the reference itself is the float64 default. The input builders
are shared by both tiers, so both look at the same numbers."""

import torch
import torch.nn.functional as F

import _sampling_ref as sref

EPS = 1e-5
SENTINEL = sref.SENTINEL
FIELDS = ("ln1_w", "ln1_b", "wqkv", "bqkv", "wproj", "bproj", "ln2_w", "ln2_b", "w1", "b1", "w2", "b2")

# (C, heads, blocks, L, n, ld): the smallest shapes that reach every branch of the kernel
SHAPES = [
    (64, 2, 2, 81, 3, 16),    # the recipe's block; L crosses one wave
    (24, 3, 1, 20, 5, 5),     # C not a power of two, ld == n
    (4, 2, 1, 9, 2, 16),      # head dim 2
    (16, 4, 2, 70, 3, 16),    # the benchmark shape on the new kernel
    (128, 1, 1, 70, 2, 2),    # head dim 128
    (256, 8, 1, 300, 1, 1),   # widest C; L crosses 256
]


def positions(L):
    return sorted({p for p in (0, 1, 63, 64, 65, L - 1) if p < L})


def block_step(prm, h, kc, vc, p, heads, strict, dtype=torch.float64, attention=True):
    """One block on the columns h (C, n): returns (h', kc', vc'), kc / vc (n, C, L) with column p replaced.
    attention=False: o = 0 (what strict = 1 gives at p = 0) without going through the attention step."""
    C, n = h.shape
    L = kc.shape[2]
    w = {k: v.to(dtype) for k, v in prm.items()}
    a = F.layer_norm(h.t(), (C,), w["ln1_w"], w["ln1_b"], EPS).t()
    qkv = torch.cat((w["wq"], w["wkv"])) @ a + torch.cat((w["bq"], w["bkv"]))[:, None]
    dk = C // heads
    o, kc, vc = sref.decode_step(qkv, kc, vc, n, heads, L, p, dk, dk, n, strict, dtype=dtype)
    if not attention:
        o = torch.zeros_like(o)
    b = h + w["wproj"] @ o + w["bproj"][:, None]
    m = F.layer_norm(b.t(), (C,), w["ln2_w"], w["ln2_b"], EPS).t()
    m = w["w2"] @ F.gelu(w["w1"] @ m + w["b1"][:, None]) + w["b2"][:, None]
    return h + (b + m), kc, vc  # the model loop adds x again (oracle/models.py image_gpt)


def step(params, x, k_cache, v_cache, p, heads, strict, dtype=torch.float64, attention=True):
    """All blocks of position p. x: (C, n) columns; k_cache, v_cache: (blocks, n, C, L). Returns (out (C, n), k', v')."""
    h = x.to(dtype)
    ks, vs = [], []
    for i, prm in enumerate(params):
        h, kc, vc = block_step(prm, h, k_cache[i], v_cache[i], p, heads, strict, dtype, attention)
        ks.append(kc)
        vs.append(vc)
    return h, torch.stack(ks), torch.stack(vs)


def pack(params):
    """The kernel's parameter buffer as include/pg_hip.h lays it out: per block the FIELDS in order, matrices (in, out)."""
    parts = []
    for w in params:
        parts += [w["ln1_w"], w["ln1_b"], torch.cat((w["wq"], w["wkv"])).t(), torch.cat((w["bq"], w["bkv"])),
                  w["wproj"].t(), w["bproj"], w["ln2_w"], w["ln2_b"], w["w1"].t(), w["b1"], w["w2"].t(), w["b2"]]
    return torch.cat([t.contiguous().reshape(-1).float() for t in parts])


# ---------------------------------------------------------------------------------------------
# inputs shared by the CPU tier (fp32-restatement check of the tolerances) and the GPU tier
def block_params(C, blocks, seed=0):
    """Per block: LayerNorm weights 1 + N(0, 0.3) and biases N(0, 0.2), projections N(0, 1 / in) with biases N(0, 0.1)."""
    g = sref._gen(C, blocks, seed, 19)

    def rn(*shape, scale=1.0):
        return scale * torch.randn(*shape, generator=g)

    out = []
    for _ in range(blocks):
        out.append({
            "ln1_w": 1 + rn(C, scale=0.3), "ln1_b": rn(C, scale=0.2),
            "wq": rn(C, C, scale=C ** -0.5), "bq": rn(C, scale=0.1),
            "wkv": rn(2 * C, C, scale=C ** -0.5), "bkv": rn(2 * C, scale=0.1),
            "wproj": rn(C, C, scale=C ** -0.5), "bproj": rn(C, scale=0.1),
            "ln2_w": 1 + rn(C, scale=0.3), "ln2_b": rn(C, scale=0.2),
            "w1": rn(4 * C, C, scale=C ** -0.5), "b1": rn(4 * C, scale=0.1),
            "w2": rn(C, 4 * C, scale=(4 * C) ** -0.5), "b2": rn(C, scale=0.1),
        })
    return out


def columns(C, n, ld, seed=0, fill=SENTINEL):
    """x (C, ld): seeded normal in columns < n, `fill` in the padding columns."""
    x = torch.full((C, ld), fill)
    x[:, :n] = torch.randn(C, n, generator=sref._gen(C, n, ld, seed, 23))
    return x


def caches(C, blocks, n, L, p, seed=0, future=SENTINEL):
    """(blocks, n, C, L) caches filled for j < p from a seeded normal, `future` in every column j >= p."""
    g = sref._gen(C, blocks, n, L, seed, 29)
    kc = torch.full((blocks, n, C, L), future)
    vc = torch.full((blocks, n, C, L), future)
    kc[..., :p] = torch.randn(blocks, n, C, L, generator=g)[..., :p]
    vc[..., :p] = torch.randn(blocks, n, C, L, generator=g)[..., :p]
    return kc, vc


def sequence_columns(C, n, ld, L, seed=0):
    """(L, C, ld): a fresh input column set for every step of a whole-sequence run."""
    x = torch.full((L, C, ld), SENTINEL)
    x[:, :, :n] = torch.randn(L, C, n, generator=sref._gen(C, n, ld, L, seed, 31))
    return x


def sequence_ref(params, xs, n, heads, strict, dtype=torch.float64):
    """step for p = 0 .. L-1 from zeroed caches; returns (outs (L, C, n), k_cache, v_cache)."""
    L, C, _ = xs.shape
    kc = torch.zeros(len(params), n, C, L, dtype=dtype)
    vc = torch.zeros(len(params), n, C, L, dtype=dtype)
    outs = []
    for p in range(L):
        o, kc, vc = step(params, xs[p, :, :n], kc, vc, p, heads, strict, dtype)
        outs.append(o)
    return torch.stack(outs), kc, vc


def spike_case(params, C, heads, n, L, p, where, score=60.0, seed=0):
    """Softmax-rescale inputs for step p of block 0 (causal): the cached keys of block 0 are chosen so that every admitted key
    scores ~0 against the step's q except the one at position `where`, which scores about `score` above them. The query is
    what the block computes from x (float64), so the spike is exact up to the kernel's own rounding of q.
    where == p spikes the position's OWN key, which the block computes itself: its key projection is then replaced by a
    zero weight and the spike as the bias (one sample only, the spike depends on the sample's q).
    Returns (params, x (C, n), k_cache, v_cache) for a ONE-block parameter list."""
    assert len(params) == 1 and 0 <= where <= p and (where < p or n == 1)
    params = [dict(params[0])]
    x = columns(C, n, n, seed=seed + 101)
    kc, vc = caches(C, 1, n, L, p, seed=seed + 103)
    w = {k: v.double() for k, v in params[0].items()}
    a = F.layer_norm(x.double().t(), (C,), w["ln1_w"], w["ln1_b"], EPS).t()
    q = (w["wq"] @ a + w["bq"][:, None]).reshape(heads, C // heads, n)  # (heads, dk, n)
    dk = C // heads
    kc[0, :, :, :p] *= 0.01
    spike = (q * (score * dk ** 0.5) / (q * q).sum(1, keepdim=True)).reshape(C, n)  # q . spike / sqrt(dk) = score
    if where < p:
        kc[0, :, :, where] = spike.t().float()
    else:
        wkv, bkv = params[0]["wkv"].clone(), params[0]["bkv"].clone()
        wkv[:C], bkv[:C] = 0, spike[:, 0].float()
        params[0]["wkv"], params[0]["bkv"] = wkv, bkv
    return params, x, kc, vc


def attention_weights(prm, x, kc, p, heads):
    """Causal softmax weights (n, heads, p + 1) of step p of ONE block in float64 (kc: (n, C, L) before the step)."""
    C, n = x.shape
    w = {k: v.double() for k, v in prm.items()}
    a = F.layer_norm(x.double().t(), (C,), w["ln1_w"], w["ln1_b"], EPS).t()
    qkv = torch.cat((w["wq"], w["wkv"])) @ a + torch.cat((w["bq"], w["bkv"]))[:, None]
    keys = kc.double().clone()
    keys[:, :, p] = qkv[C:2 * C].t()
    dk = C // heads
    s = torch.einsum("nhd,nhdj->nhj", qkv[:C].t().reshape(n, heads, dk), keys[:, :, :p + 1].reshape(n, heads, dk, p + 1))
    return torch.softmax(s / dk ** 0.5, dim=-1)


def single_case(shape, p, seed=0, future=SENTINEL):
    """(params, x (C, ld), k_cache, v_cache) of a single-step test at position p from random caches."""
    C, heads, blocks, L, n, ld = shape
    kc, vc = caches(C, blocks, n, L, p, seed=seed + p, future=future)
    return block_params(C, blocks, seed), columns(C, n, ld, seed=seed + p), kc, vc


SPIKE_SHAPES = [(64, 2, 81), (24, 3, 20), (256, 8, 300)]  # (C, heads, L); one block, one sample, p = L - 1


def spike_wheres(L):
    return (0, (L - 1) // 2, L - 1)  # the first, a middle and the last admitted key (the position's own)


# ---------------------------------------------------------------------------------------------
# a whole ImageGPT as a reference-keyed state_dict (for oracle.models.image_gpt)
def model_state(C, heads, blocks, H, W, in_ch=1, out_ch=1, seed=0, dtype=torch.float64):
    g = sref._gen(C, heads, blocks, H, W, seed, 37)
    params = block_params(C, blocks, seed)
    p = {"_pos": 0.1 * torch.randn(1, in_ch, H, W, generator=g),
         "_input.weight": torch.randn(C, in_ch, 3, 3, generator=g) / 3, "_input.bias": 0.1 * torch.randn(C, generator=g),
         "_ln.weight": 1 + 0.3 * torch.randn(C, generator=g), "_ln.bias": 0.2 * torch.randn(C, generator=g),
         "_out.weight": torch.randn(out_ch, C, 1, 1, generator=g) * C ** -0.5, "_out.bias": 0.1 * torch.randn(out_ch, generator=g)}
    names = {"ln1_w": "_ln1.weight", "ln1_b": "_ln1.bias", "wq": "_attn._q.weight", "bq": "_attn._q.bias",
             "wkv": "_attn._kv.weight", "bkv": "_attn._kv.bias", "wproj": "_attn._proj.weight", "bproj": "_attn._proj.bias",
             "ln2_w": "_ln2.weight", "ln2_b": "_ln2.bias", "w1": "_out.0.weight", "b1": "_out.0.bias",
             "w2": "_out.2.weight", "b2": "_out.2.bias"}
    for i, prm in enumerate(params):
        for k, v in prm.items():
            p[f"_transformer.{i}.{names[k]}"] = v.reshape(*v.shape, 1, 1) if v.dim() == 2 else v
    return {k: v.to(dtype) for k, v in p.items()}, params
