"""The case table of the causal-attention family tests: tests/test_attn_route_cpu.py asks `pg_attn_route` whether every case
lands on the kernel family and has the feature it is there for, tests/test_gpu_attention_families.py runs it against float64.

Softmax attention runs on three kernel families (csrc/attention.hip: attn_route decides):
  valu  the VALU row-owner kernels (attention.hip): whatever the other two decline
  m44   the d_k = d_v = 4 matrix-core kernels (attention_mfma.hip), kernel by kernel while their LDS planes fit 160 KB
  k4    the matrix-core kernels of attention_k4.hip: d_k in {4, 16, 32, 64} x d_v in {16, 32, 64}, L % 16 == 0, aligned planes
A case names the family of its forward, dQ, dK/dV launch and of the fused-backward request (with the switch on; "declined":
the two kernels follow) and the features it exercises; `FEATURES` turns a feature name into a predicate over the four routes, so
a case that a change of the dispatch moves elsewhere fails on the CPU, by name.

Inputs are seeded N(0, 1); a boosted case overwrites channel 0 of every head, q = 128 sqrt(d_k / 4) (1 +- clamp / 32) and k a
staircase of 0.25 per step at the key positions `boost` lists (the recipe of test_gpu_attn_partition._case, where it is derived,
with the factor sqrt(d_k / 4) keeping the score step at 16 (1 +- 5/32) natural units for every d_k): the scores step up by ~19
log2 units at those keys, which the kernels' running-max rescales must survive wherever the step falls in their tiling.
The reference is float64 `oracle.ops.causal_attention_core`, evaluated once per case in batch slices of <= 96 images."""

import collections
import functools
import math

import torch

FWD, DQ, DKV, BWD = 0, 1, 2, 3
KERNELS = ("fwd", "dq", "dkv", "bwd")
REF_SLICE = 96

Case = collections.namedtuple("Case", "name n heads dk dv h w strict boost merged families features")


def _c(name, n, heads, dk, dv, h, w, strict, families, features, boost=(), merged=False):
    if isinstance(families, str):
        families = {"valu": ("valu", "valu", "valu", "declined"), "k4": ("k4", "k4", "k4", "declined"),
                    "k4f": ("k4", "k4", "k4", "k4")}[families]
    return Case(name, n, heads, dk, dv, h, w, bool(strict), tuple(boost), merged, tuple(families), tuple(features))


# ---- features: name -> predicate(case, [route of fwd, dq, dkv, bwd]) -------------------------------------------------------
def _L(c):
    return c.h * c.w


def _nb(c):
    return -(-_L(c) // 64)


def _all3(pred):
    return lambda c, r: all(pred(x) for x in r[:3])


FEATURES = {
    # VALU row-owner kernels
    "slot_b": lambda c, r: _nb(c) >= 2 and all(x["family"] == "valu" for x in r[:3]),      # a wave owns two 64-row blocks
    "ragged_block": lambda c, r: _L(c) % 64 != 0,
    "odd_blocks": lambda c, r: _nb(c) % 2 == 1 and _nb(c) >= 3,                             # the middle wave owns one block
    "tiles2_all": _all3(lambda x: x["family"] == "valu" and x["tiles"] >= 2),             # kt < rows and kt2 < rows
    "tiles2_dkv": lambda c, r: r[DKV]["family"] == "valu" and r[DKV]["tiles"] >= 2,
    "grid2": lambda c, r: any(x["family"] == "valu" and x["grid_x"] >= 2 for x in r[:3]),  # first > 0, reversed workgroup order
    "grid3": lambda c, r: any(x["family"] == "valu" and x["grid_x"] >= 3 for x in r[:3]),
    "bpw16": lambda c, r: any(x["family"] == "valu" and x["blocks_per_wg"] == 16 for x in r[:3]),
    "cfg4_4": _all3(lambda x: x["family"] != "valu" or (x["t0"], x["t1"]) == (4, 4)),
    "cfg4_16": _all3(lambda x: (x["family"], x["t0"], x["t1"]) == ("valu", 4, 16)),
    "cfg4_32": _all3(lambda x: (x["family"], x["t0"], x["t1"]) == ("valu", 4, 32)),
    "cfg16_4": _all3(lambda x: (x["family"], x["t0"], x["t1"]) == ("valu", 16, 4)),
    "cfg16_16": _all3(lambda x: (x["family"], x["t0"], x["t1"]) == ("valu", 16, 16)),
    "not_mult16": lambda c, r: _L(c) % 16 != 0,
    # d_k = d_v = 4 hand-offs
    "m44_vec": lambda c, r: all(x["vec"] == 1 for x in r[:3] if x["family"] == "m44") and _L(c) % 4 == 0,
    "m44_scalar": lambda c, r: all(x["vec"] == 0 for x in r[:3] if x["family"] == "m44") and _L(c) % 4 != 0,
    "lse_m44_to_valu": lambda c, r: r[FWD]["family"] == "m44" and "valu" in (r[DQ]["family"], r[DKV]["family"]),
    "delta_valu_to_m44": lambda c, r: r[DQ]["family"] == "valu" and r[DKV]["family"] == "m44",
    "fused_declined_by_lds": lambda c, r: r[BWD]["family"] == "declined" and r[BWD]["fused_on"] == 1 and c.dk == c.dv == 4,
    "strided_views": lambda c, r: c.merged,
    # k4
    "qb4": _all3(lambda x: x["family"] == "k4" and x["qb"] == 4),
    "qb2": _all3(lambda x: x["family"] == "k4" and x["qb"] == 2),
    "qb1": _all3(lambda x: x["family"] == "k4" and x["qb"] == 1),
    "one_key_tile": lambda c, r: _L(c) == 16 and r[FWD]["family"] == "k4",
    "ragged_k4_block": lambda c, r: r[FWD]["family"] == "k4" and _L(c) % (16 * r[FWD]["qb"]) != 0,
    "k4_units_3072": lambda c, r: c.n * c.heads * ((_nb(c) + 1) // 2) >= 3072,
    "boost": lambda c, r: bool(c.boost),
}


def _k4_inst(dk, dv):
    return (1 if dk == 4 else dk // 4, dv // 16)


# ---- the table ---------------------------------------------------------------------------------------------------------------
M, V, D = "m44", "valu", "declined"
CASES = [
    # VALU row-owner kernels: everything the matrix-core families decline. Both mask kinds across the set.
    _c("valu-2x2-L100", 2, 1, 2, 2, 10, 10, False, "valu", ["slot_b", "ragged_block", "cfg4_4"]),
    _c("valu-8x8-L169", 2, 1, 8, 8, 13, 13, True, "valu", ["slot_b", "odd_blocks", "ragged_block", "cfg16_16"]),
    _c("valu-8x8-L576", 2, 2, 8, 8, 24, 24, False, "valu", ["tiles2_all", "odd_blocks", "cfg16_16"]),
    _c("valu-16x16-L529", 1, 1, 16, 16, 23, 23, True, "valu", ["tiles2_all", "not_mult16", "cfg16_16"]),
    _c("valu-8x8-L1089", 1, 1, 8, 8, 33, 33, True, "valu", ["grid2", "bpw16", "tiles2_all", "ragged_block"]),
    _c("valu-4x8-L784", 1, 2, 4, 8, 28, 28, False, "valu", ["cfg4_16", "tiles2_all", "odd_blocks"]),
    _c("valu-8x4-L784", 1, 2, 8, 4, 28, 28, True, "valu", ["cfg16_4", "tiles2_all", "odd_blocks"]),
    _c("valu-4x32-L462", 1, 1, 4, 32, 22, 21, True, "valu", ["cfg4_32", "tiles2_all", "not_mult16"]),
    _c("valu-4x16-L900", 1, 1, 4, 16, 30, 30, False, "valu", ["cfg4_16", "tiles2_all", "not_mult16"]),
    _c("valu-2x2-L2116", 1, 1, 2, 2, 46, 46, False, "valu", ["cfg4_4", "tiles2_all", "grid3", "bpw16"]),
    _c("valu-8x8-L169-qkv", 2, 1, 8, 8, 13, 13, False, "valu", ["strided_views", "slot_b", "cfg16_16"], merged=True),
    # d_k = d_v = 4 beyond the LDS budget of the matrix-core kernels, one case per band: families mix inside one
    # forward / backward (lse2 from an MFMA forward into a VALU dQ, delta from a VALU dQ into an MFMA dK/dV)
    _c("d4-L1856", 1, 2, 4, 4, 29, 64, False, (M, M, M, D), ["fused_declined_by_lds", "m44_vec"]),
    _c("d4-L2025", 1, 1, 4, 4, 45, 45, True, (M, V, M, D), ["lse_m44_to_valu", "delta_valu_to_m44", "m44_scalar"]),
    _c("d4-L2304", 1, 1, 4, 4, 36, 64, False, (M, V, V, D), ["lse_m44_to_valu", "m44_vec", "tiles2_dkv"]),
    _c("d4-L3481", 1, 1, 4, 4, 59, 59, True, (V, V, V, D), ["cfg4_4", "tiles2_all", "grid3"]),
    _c("d4-L2025-qkv", 1, 2, 4, 4, 45, 45, False, (M, V, M, D), ["strided_views", "delta_valu_to_m44"], merged=True),
    # ... and both sides of every band edge (test_attn_route_cpu finds the edges by scanning L and looks them up here)
    _c("d4-L1792", 1, 1, 4, 4, 28, 64, True, (M, M, M, M), ["m44_vec"]),
    _c("d4-L1793", 1, 1, 4, 4, 11, 163, False, (M, M, M, D), ["fused_declined_by_lds", "m44_scalar"]),
    _c("d4-L1984", 1, 1, 4, 4, 31, 64, False, (M, M, M, D), ["m44_vec"]),
    _c("d4-L1985", 1, 1, 4, 4, 5, 397, True, (M, V, M, D), ["delta_valu_to_m44", "m44_scalar"]),
    _c("d4-L2240", 1, 1, 4, 4, 35, 64, True, (M, V, M, D), ["delta_valu_to_m44", "m44_vec"]),
    _c("d4-L2241", 1, 1, 4, 4, 27, 83, False, (M, V, V, D), ["lse_m44_to_valu", "m44_scalar"]),
    _c("d4-L3392", 1, 1, 4, 4, 53, 64, False, (M, V, V, D), ["lse_m44_to_valu", "m44_vec"]),
    _c("d4-L3393", 1, 1, 4, 4, 39, 87, True, (V, V, V, D), ["cfg4_4", "grid3"]),
    # k4: one case per instantiation row of pg_attn_k4_route, 64 <= L <= 400
    _c("k4-4x16-L256", 2, 2, 4, 16, 16, 16, False, "k4f", ["qb2"]),
    _c("k4-4x32-L400", 1, 1, 4, 32, 20, 20, True, "k4f", ["qb2", "ragged_k4_block"]),
    _c("k4-4x64-L256", 2, 2, 4, 64, 16, 16, False, "k4", ["qb2"]),
    _c("k4-16x16-L144", 2, 1, 16, 16, 12, 12, True, "k4", ["qb2", "ragged_k4_block"]),
    _c("k4-16x32-L256", 2, 2, 16, 32, 16, 16, False, "k4", ["qb2"]),
    _c("k4-16x64-L256", 2, 1, 16, 64, 16, 16, True, "k4", ["qb1"]),
    _c("k4-32x16-L400", 1, 2, 32, 16, 20, 20, True, "k4", ["qb2", "ragged_k4_block"]),
    _c("k4-32x32-L144", 2, 2, 32, 32, 12, 12, False, "k4", ["qb2", "ragged_k4_block"]),
    _c("k4-32x64-L64", 2, 1, 32, 64, 8, 8, False, "k4", ["qb1"]),
    _c("k4-64x16-L192", 1, 2, 64, 16, 16, 12, False, "k4", ["qb1"]),
    _c("k4-64x32-L80", 1, 1, 64, 32, 10, 8, True, "k4", ["qb1"]),
    _c("k4-64x64-L144", 1, 2, 64, 64, 12, 12, True, "k4", ["qb1"]),
    _c("k4-4x32-L16", 2, 1, 4, 32, 4, 4, False, "k4f", ["one_key_tile", "qb2"]),
    # the 64-row blocks (QB = 4) need N * heads * ceil(ceil(L / 64) / 2) >= 3072 units: L = 144 is two whole blocks and a
    # ragged 16-row one. The fused k4 backward has its own fixed block size; the two-kernel backward runs <.., 4>.
    _c("k4-4x32-L144-qb4", 768, 2, 4, 32, 12, 12, True, "k4f", ["qb4", "k4_units_3072", "ragged_k4_block"]),
    _c("k4-4x16-L144-qb4", 768, 2, 4, 16, 12, 12, False, "k4f", ["qb4", "k4_units_3072", "ragged_k4_block"]),
    # large scores: steps on the tile boundary kt and a 64-row block boundary (VALU), on 16-key tile boundaries inside and
    # across query blocks (k4)
    _c("valu-8x8-L576-boost", 2, 2, 8, 8, 24, 24, False, "valu", ["boost", "tiles2_all"], boost=(64, 448, 512)),
    _c("valu-16x16-L529-boost", 1, 1, 16, 16, 23, 23, True, "valu", ["boost", "tiles2_all"], boost=(64, 448, 512)),
    _c("valu-4x32-L462-boost", 1, 1, 4, 32, 22, 21, True, "valu", ["boost", "tiles2_all"], boost=(64, 448)),
    _c("k4-4x32-L256-boost", 1, 1, 4, 32, 16, 16, True, "k4f", ["boost", "qb2"], boost=(16, 96, 208)),
    _c("k4-32x32-L144-boost", 2, 2, 32, 32, 12, 12, False, "k4", ["boost", "qb2"], boost=(16, 64, 112)),
    _c("k4-64x64-L64-boost", 2, 1, 64, 64, 8, 8, False, "k4", ["boost", "qb1"], boost=(16, 32, 48)),
]
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)


def family_of(case):
    """The family a case is filed under (its name's prefix): the one that changes what the test demands of a second run."""
    return {"valu": "valu", "d4": "m44", "k4": "k4"}[case.name.split("-")[0]]


# ---- routes ------------------------------------------------------------------------------------------------------------------
def routes(case):
    """[route of forward, dQ, dK/dV, fused request] as ops.attention_route dicts, with the flags of the op the case runs."""
    from pytorch_generative_amd import ops

    e, v = case.heads * case.dk, case.heads * case.dv
    flags = ops.attention_layout_flags(case.heads, e, v, case.h * case.w, case.merged)
    return [ops.attention_route(which, case.n, case.heads, case.h * case.w, case.dk, case.dv, flags) for which in range(4)]


def route_problems(case, rts, fused_on=True):
    """What keeps `case` from being the case its entry describes, as a list of strings (empty: all is as claimed)."""
    want = list(case.families)
    if not fused_on:
        want[BWD] = "declined"
    bad = [f"{KERNELS[i]}: on {rts[i]['family']}, the entry says {want[i]}" for i in range(4) if rts[i]["family"] != want[i]]
    bad += [f"status {r['status']}" for r in rts if r["status"] != 0]
    for i in range(3):
        if want[i] == "k4" and (rts[i]["t0"], rts[i]["t1"]) != _k4_inst(case.dk, case.dv):
            bad.append(f"{KERNELS[i]}: instantiation {rts[i]['t0'], rts[i]['t1']}")
    if fused_on:  # the features are claims about the default state of the switch
        bad += [f"feature {f} absent" for f in case.features if not FEATURES[f](case, rts)]
    return bad


# ---- inputs and the float64 reference ----------------------------------------------------------------------------------------
def _rand(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


@functools.lru_cache(maxsize=None)
def inputs(name):
    """(q, kv, d_o) of a case, float32 on the CPU. Never modified by the tests."""
    c = BY_NAME[name]
    e, v = c.heads * c.dk, c.heads * c.dv
    q, kv, d_o = _rand(c.n, e, c.h, c.w, seed=1), _rand(c.n, e + v, c.h, c.w, seed=2), _rand(c.n, v, c.h, c.w, seed=3)
    if c.boost:
        pos = torch.arange(c.h * c.w).reshape(1, 1, c.h, c.w)
        q[:, 0:e:c.dk] = 128.0 * math.sqrt(c.dk / 4) * (1.0 + q[:, 0:e:c.dk].clamp(-5.0, 5.0) / 32)
        kv[:, 0:e:c.dk] = sum((pos >= s).float() for s in c.boost) * 0.25
    return q, kv, d_o


def _reference_of(c, q, kv, d_o, dtype):
    from oracle import ops as oops

    e = c.heads * c.dk
    outs = []
    for i in range(0, c.n, REF_SLICE):
        qo = q[i:i + REF_SLICE].to(dtype).requires_grad_(True)
        kvo = kv[i:i + REF_SLICE].to(dtype).requires_grad_(True)
        oo = oops.causal_attention_core(qo, kvo[:, :e], kvo[:, e:], c.heads, c.strict)
        oo.backward(d_o[i:i + REF_SLICE].to(dtype))
        outs.append((oo.detach(), qo.grad, kvo.grad[:, :e], kvo.grad[:, e:]))
    return tuple(torch.cat(t) for t in zip(*outs))


@functools.lru_cache(maxsize=None)
def reference(name):
    """(o, dq, dk, dv) in float64, made once per case and shared by both backward modes."""
    return _reference_of(BY_NAME[name], *inputs(name), torch.float64)
