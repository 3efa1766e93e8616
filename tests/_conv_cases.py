"""The forward / data-gradient convolution cases shared by tests/test_conv_cases_cpu.py and tests/test_gpu_conv_families.py: one entry per
kernel instantiation and epilogue form the bf16x3 format can launch (csrc/conv_b3.hip: b3_route) and per edge of its dispatch, three
cases on the fp32-MFMA format (csrc/conv_mfma.hip) and six on the VALU tap kernels (csrc/conv_direct.hip), the inputs of five kinds, a
plain float64 reference, and a numpy emulation of the bf16x3 pieces.

A case is a convolution in the LAUNCH's coordinates: `in` (N, K, IH, IW) is contracted over K channels and the tap list into `out`
(N, M, OH, OW), out[n, m, r, c] = sum_t sum_k Wsel[m][k][t] in_act(in)[n, k, r + dr[t], c + dc[t]] (zero outside the input), followed by
the epilogue of its form. The weight is made in the torch layout of the convolution the launch belongs to:
  fwd    w (M, K, kh, kw), Wsel[m][k][t] = w[m][k][u_t][v_t], (dr, dc) = (u - ph, v - pw);
  dgrad  w (K, M, kh, kw) (the forward convolution maps M -> K channels), Wsel[m][k][t] = w[k][m][u_t][v_t] (the transposed pack),
         (dr, dc) = (ph - u, pw - v) (negated taps), as include/pg_hip.h says of the data gradient.
Taps are the full kh x kw grid with causal padding (PAD), the output is cropped to the input size.

Epilogue forms (include/pg_hip.h): v = out_act(conv + bias) * act'(dact_src) + res + res2 with the operands the form names; `gate`:
out = conv + bias + res, gate_out = gate_res + f(out[:, :M/2]) sigmoid(out[:, M/2:]); `dual`: d = conv * act'(dact_src),
out = d * elu'_from_output(dact_src - r), out2 = d * elu'_from_output(r).

Input kinds, every tensor seeded by the case's position:
  int     x integer in [-8, 8], w integer in [-4, 4] (about 28 % non-zero), unit 1;
  x3      x = +-(1 + b 2^-8 + c 2^-16), b, c in {1, 3}: three non-zero bf16 pieces under the TRUNCATION split of the kernels' staging
          (split8t); w in {-1, 0, 1}: one piece. Exercises w0.xh, w0.xm, w0.xl. Unit 2^-16;
  w3      w = +-(1 + 2^-9 + 2^-18): three non-zero pieces under the ROUND-TO-NEAREST split of the pack (split8); x in {-1, 0, 1}.
          Exercises w0.xh, w1.xh, w2.xh. Unit 2^-18;
  x2w2    both +-(1 + 2^-9): two pieces each. Exercises w0.xh, w0.xm, w1.xh, w1.xm. Unit 2^-18;
  random  seeded normals, weights scaled by 0.2, the activation ids rotated over the cases.
In the four exact kinds the activations are none / ReLU, bias and residuals are integer multiples of the unit, and every output
channel has at most NNZ[kind] non-zero weights: sum |w| |in_act(x)| + |bias| + |res| + |res2| stays below 2^24 units at every output
(asserted from the absolute reference by the CPU tier), so every product and every partial sum in ANY order is exact in fp32 — the
argument of tests/test_gpu_wgrad_families.py scaled by a power of two — and a kernel must return the float64 reference bit for bit.
A dropped, swapped or mis-indexed piece is at least one unit per affected product.
"""

import collections
import functools

import numpy as np
import torch
import torch.nn.functional as F

import _conv_b3_routes as R
import _small_ref

KINDS = ("int", "x3", "w3", "x2w2", "random")
EXACT_KINDS = KINDS[:4]
UNIT = {"int": 1.0, "x3": 2.0 ** -16, "w3": 2.0 ** -18, "x2w2": 2.0 ** -18}
NNZ = {"int": 1 << 20, "x3": 200, "w3": 56, "x2w2": 56}   # non-zero weights per output channel at most (int: a density instead)
OPERAND_UNITS = {"int": 64, "x3": 1 << 18, "w3": 1 << 18, "x2w2": 1 << 18}  # |bias|, |res|, |res2| <= this many units each
PRODUCTS = ("w0.xh", "w0.xm", "w0.xl", "w1.xh", "w1.xm", "w2.xh")          # the six the kernels evaluate (piece of w, piece of x)
DROPPED = ("w1.xl", "w2.xm", "w2.xl")
EXERCISES = {"int": ("w0.xh",), "x3": ("w0.xh", "w0.xm", "w0.xl"), "w3": ("w0.xh", "w1.xh", "w2.xh"),
             "x2w2": ("w0.xh", "w0.xm", "w1.xh", "w1.xm")}
ACTS = (None, "relu", "elu", "gelu", "elu_out")   # index = PG_ACT_* (elu_out: only as a derivative id)
ACT_GELU, ACT_ELU, ACT_ELU_OUT = 3, 2, 4
FMT_TAPS, FMT_F32, FMT_B3, FMT_B3_GATE = 0, 1, 2, 3
PAD = {1: 0, 2: 1, 3: 1}   # causal padding per filter extent (a 2-wide filter looks back one, a 3-wide one is centred)

# form -> the operands its launch has: PG_B3R_* flags of the route (the bf16x3 cases), gate
FORM_FLAGS = {
    "plain": 0,
    "two_residuals": R.RES | R.RES2,
    "same_residual_twice": R.RES | R.RES2 | R.RES2_SAME,
    "res_dact": R.RES | R.DACT_SRC,
    "res_strided": R.RES | R.RES_STRIDED,
    "dact": R.DACT_SRC,
    "gate": 0,
    "dual": R.RES | R.DACT_SRC | R.DUAL,
}

Case = collections.namedtuple("Case", "name backend orient n k ih iw m oh ow kh kw taps form acts mis want")


def C(name, n, k, m, kk, hw, form="plain", orient="fwd", acts=None, mis="", backend="b3", **want):
    kh, kw = kk
    ph, pw = PAD[kh], PAD[kw]
    sign = 1 if orient == "fwd" else -1
    taps = tuple((sign * (u - ph), sign * (v - pw), u, v) for u in range(kh) for v in range(kw))
    return Case(name, backend, orient, n, k, hw[0], hw[1], m, hw[0], hw[1], kh, kw, taps, form, acts or {}, mis, want)


ST, PW, PL, OV = 0, 1, 2, 3  # kernel ids of the route
CASES = [
    # ---- staged kernel (conv_b3_kernel): output tiles, chunk sizes -----------------------------------------------------------------
    C("staged-3x3-32to16", 2, 32, 16, (3, 3), (8, 8), kernel=ST, MT=1, CG=1, MS=0, CIB=16),
    C("staged-3x3-32to32", 3, 32, 32, (3, 3), (8, 8), kernel=ST, MT=2, CG=1, MS=0, CIB=16),
    C("staged-3x3-16to48", 2, 16, 48, (3, 3), (8, 8), kernel=ST, MT=3, CG=1, MS=0, CIB=8),
    C("staged-3x3-64to64", 2, 64, 64, (3, 3), (8, 8), kernel=ST, MT=4, CG=1, MS=0),
    C("staged-3x3-64to64-two-residuals", 3, 64, 64, (3, 3), (8, 8), "two_residuals", kernel=ST, MT=4, CG=1, MS=1),
    C("staged-3x3-64to64-same-residual-twice", 2, 64, 64, (3, 3), (8, 8), "same_residual_twice", kernel=ST, MT=4, CG=1, MS=1,
      res2_folded=0),
    C("staged-3x3-64to64-res-dact", 2, 64, 64, (3, 3), (8, 8), "res_dact", kernel=ST, MT=4, CG=1, MS=1),
    C("staged-3x3-64to64-res-strided", 3, 64, 64, (3, 3), (8, 8), "res_strided", kernel=ST, MT=4, CG=1, MS=1),
    C("staged-3x3-64to64-gelu", 2, 64, 64, (3, 3), (8, 8), acts={"in_act": ACT_GELU}, kernel=ST, MT=4, CG=1, MS=0),
    C("staged-wide-3x3-64to128", 2, 64, 128, (3, 3), (8, 8), kernel=ST, MT=4, CG=2, MS=0, GT=0, block=512),
    C("staged-wide-3x3-64to128-two-residuals", 3, 64, 128, (3, 3), (8, 8), "two_residuals", kernel=ST, MT=4, CG=2, MS=1, block=512),
    C("gate-3x3-64to128", 2, 64, 128, (3, 3), (8, 8), "gate", kernel=ST, CG=2, MS=0, GT=1, CIB=8),
    C("gate-2x3-64to128", 3, 64, 128, (2, 3), (8, 8), "gate", kernel=ST, CG=2, MS=0, GT=1, CIB=16),
    C("gate-1x3-32to128-12x12", 2, 32, 128, (1, 3), (12, 12), "gate", kernel=ST, CG=2, MS=0, GT=1, NT=3),
    C("staged-3x3-24to64-20x24-two-row-tiles", 3, 24, 64, (3, 3), (20, 24), kernel=ST, MT=4, CG=1, TR=10, tiles_per_img=2, NT=4),
    C("staged-2x3-40to72-20x24-partial-chunk", 3, 40, 72, (2, 3), (20, 24), kernel=ST, MT=4, CG=1, tiles_per_img=2, grid_y=2),
    C("staged-3x3-64to64-9x20-ragged-groups", 2, 64, 64, (3, 3), (9, 20), kernel=ST, MT=4, CG=1, NT=3),
    C("staged-3x3-32to32-4x4", 3, 32, 32, (3, 3), (4, 4), kernel=ST, MT=2, CG=1, tiles_per_img=1),
    C("staged-2x1-32to64-16x64-four-tiles", 2, 32, 64, (2, 1), (16, 64), kernel=ST, MT=4, CG=1, TR=4, tiles_per_img=4),
    C("staged-1x3-32to32-8x16-two-groups", 3, 32, 32, (1, 3), (8, 16), kernel=ST, MT=2, CG=1, NT=2),
    # ---- 1x1 kernel (conv_b3_pw_kernel) and what leaves it --------------------------------------------------------------------------------
    C("pw-16to16", 2, 16, 16, (1, 1), (8, 8), kernel=PW, MT=1, MS=0),
    C("pw-32to32", 3, 32, 32, (1, 1), (8, 8), kernel=PW, MT=2, MS=0),
    C("pw-64to64", 2, 64, 64, (1, 1), (8, 8), kernel=PW, MT=4, MS=0),
    C("pw-64to64-two-residuals", 3, 64, 64, (1, 1), (8, 8), "two_residuals", kernel=PW, MT=4, MS=1),
    C("pw-64to64-same-residual-twice", 2, 64, 64, (1, 1), (8, 8), "same_residual_twice", kernel=PW, MT=4, MS=0, res2_folded=1,
      res_scale=2),
    C("pw-64to64-dual", 2, 64, 64, (1, 1), (8, 8), "dual", orient="dgrad", kernel=PW, MT=4, MS=1),
    C("pw-64to160-6x10-two-residuals", 3, 64, 160, (1, 1), (6, 10), "two_residuals", kernel=PW, MT=4, MS=1, grid_y=3),
    C("pw-64to64-gelu", 2, 64, 64, (1, 1), (8, 8), acts={"in_act": ACT_GELU}, kernel=PW, MT=4, MS=0),
    C("1x1-64to64-7x7-odd-pixels", 2, 64, 64, (1, 1), (7, 7), kernel=ST, MT=4, CG=1),
    C("1x1-64to64-in-misaligned", 2, 64, 64, (1, 1), (8, 8), mis="in", kernel=ST, MT=4, CG=1),
    C("1x1-128to64-slab-above-24k", 2, 128, 64, (1, 1), (8, 8), kernel=ST, MT=4, CG=1),
    C("1x1-48to96-6x10", 3, 48, 96, (1, 1), (6, 10), kernel=ST, CIB=16),
    # ---- pipelined kernel (conv_b3p_kernel): four taps ---------------------------------------------------------------------------------------
    C("pipelined-2x2-64to64-8x8", 2, 64, 64, (2, 2), (8, 8), kernel=PL, waves=8, NT=1),
    C("pipelined-2x2-64to64-16x16", 3, 64, 64, (2, 2), (16, 16), kernel=PL, waves=8, NT=2),
    C("pipelined-2x2-40to56-12x20-partial-chunk", 3, 40, 56, (2, 2), (12, 20), kernel=PL, NT=2, grid_y=1),
    C("pipelined-2x2-64to160-two-residuals", 2, 64, 160, (2, 2), (8, 8), "two_residuals", kernel=PL, grid_y=3),
    C("pipelined-2x2-64to64-20x32-three-tiles", 2, 64, 64, (2, 2), (20, 32), kernel=PL, TR=7, tiles_per_img=3),
    C("pipelined-2x2-64to64-dgrad-res-dact", 3, 64, 64, (2, 2), (8, 8), "res_dact", orient="dgrad", kernel=PL),
    # ---- overlapped kernel (conv_b3q_kernel): two tiles per workgroup ------------------------------------------------------------------------
    C("overlapped-2x3-16to320-n2", 2, 16, 320, (2, 3), (16, 32), kernel=OV, two_tiles=1, grid_y=5),
    C("overlapped-2x3-16to320-n3-idle-half", 3, 16, 320, (2, 3), (16, 32), kernel=OV, two_tiles=1, grid_y=5),
    C("overlapped-2x3-16to320-two-residuals", 3, 16, 320, (2, 3), (16, 32), "two_residuals", kernel=OV, two_tiles=1),
    C("overlapped-2x3-256to64-12x32", 3, 256, 64, (2, 3), (12, 32), kernel=OV, two_tiles=1, TR=6),
    C("overlapped-2x3-16to320-20x24", 3, 16, 320, (2, 3), (20, 24), kernel=OV, two_tiles=1, TR=10),
    C("overlapped-3x3-16to320", 3, 16, 320, (3, 3), (16, 32), kernel=OV, two_tiles=1, CIB=8),
    # ---- data-gradient twins: the route decides where each lands (recorded here, asserted by the CPU tier) ---------------------------
    C("dgrad-3x3-64to64-staged", 2, 64, 64, (3, 3), (8, 8), orient="dgrad", kernel=ST, MT=4, CG=1, MS=0),
    C("dgrad-1x1-64to64-pw", 3, 64, 64, (1, 1), (8, 8), "res_dact", orient="dgrad", kernel=PW, MT=4, MS=1),
    C("dgrad-2x3-320to16-staged-narrow", 3, 320, 16, (2, 3), (16, 32), orient="dgrad", kernel=ST, MT=1, CG=1),
    # ---- fp32-MFMA format (conv_mfma_kernel) ---------------------------------------------------------------------------------------------------
    C("f32-1x1-69to36", 2, 69, 36, (1, 1), (8, 8), backend="f32"),
    C("f32-3x3-20to20-dact", 3, 20, 20, (3, 3), (8, 8), "dact", orient="dgrad", backend="f32"),
    C("f32-3x3-12to16", 2, 12, 16, (3, 3), (8, 8), backend="f32"),
    # ---- VALU tap kernels (conv_direct.hip), with their data gradients ------------------------------------------------------------------
    C("taps-1x1-5to3-7x7", 2, 5, 3, (1, 1), (7, 7), backend="taps"),
    C("taps-1x1-3to5-7x7-dgrad-dact", 2, 3, 5, (1, 1), (7, 7), "dact", orient="dgrad", backend="taps"),
    C("taps-2x2-36to20-6x10", 3, 36, 20, (2, 2), (6, 10), backend="taps"),
    C("taps-2x2-20to36-6x10-dgrad-dact", 3, 20, 36, (2, 2), (6, 10), "dact", orient="dgrad", backend="taps"),
    C("taps-3x3-32to32-2x2", 2, 32, 32, (3, 3), (2, 2), backend="taps"),
    C("taps-3x3-32to32-2x2-dgrad-dact", 3, 32, 32, (3, 3), (2, 2), "dact", orient="dgrad", backend="taps"),
]
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
B3_CASES = [c for c in CASES if c.backend == "b3"]
FMT_OF_BACKEND = {"b3": FMT_B3, "f32": FMT_F32, "taps": FMT_TAPS}
# one case per family also packs through pg_pack_conv_weight_frag2 (both orientations in one launch): same fragment bits
PACK2_CASES = ("staged-3x3-64to64", "staged-wide-3x3-64to128", "gate-2x3-64to128", "pw-64to64", "pipelined-2x2-64to64-8x8",
               "overlapped-2x3-16to320-n2", "dgrad-3x3-64to64-staged", "f32-3x3-12to16")


# ---- what a launch of (case, kind) passes ------------------------------------------------------------------------------------------------

def acts_of(c, kind):
    """{in_act, out_act, dact, gate}: none / ReLU alternate over the table for the exact kinds (a case that names GELU runs the exact
    kinds with ReLU: GELU of a non-zero number is not exact), every id rotates for the random kind. gate: PG_GATE_*."""
    i = CASES.index(c)
    has_dact = bool(FORM_FLAGS[c.form] & R.DACT_SRC)
    if kind != "random":
        a = {"in_act": i % 2, "out_act": (i // 2) % 2, "dact": 1 if has_dact else 0}
        if c.acts.get("in_act"):
            a["in_act"] = 1
    else:
        a = {"in_act": (i + 1) % 4, "out_act": (i // 3 + 2) % 4, "dact": (1, 2, 3, 4)[i % 4] if has_dact else 0}
        a.update(c.acts)
    a["gate"] = (i + KINDS.index(kind)) % 2
    if c.form == "gate":      # pg_conv2d_mfma_gate: no output activation, no GELU
        a["out_act"] = 0
        a["in_act"] %= 3
    if c.form == "dual":      # pg_conv2d_mfma_dual: the convolution alone, its own input activation's derivative is ELU
        a.update(in_act=0, out_act=0, dact=ACT_ELU)
    if c.backend == "taps":   # pg_conv2d_taps has no output activation and no ELU_OUT derivative, and its 1x1 kernel takes a
        a["out_act"] = 0      # derivative source only without an input activation (a data gradient has none)
        a["dact"] = a["dact"] if a["dact"] != ACT_ELU_OUT else 1
        if a["dact"]:
            a["in_act"] = 0
    return a


def gate_operands(c, kind):
    """(res given, gate_res given) of a gate case: both NULL paths and both fused paths over the kinds."""
    j = CASES.index(c) + KINDS.index(kind)
    return j % 2 == 0, j % 3 != 0


def flags_of(c, kind, fused_res=False):
    f = FORM_FLAGS[c.form] | (R.IN_MISALIGNED if "in" in c.mis else 0)
    if c.form == "gate" and gate_operands(c, kind)[0]:
        f |= R.RES
    if fused_res:
        f |= R.RES
    return f


def problem(c, kind, fused_res=False):
    """The dict tests/_conv_b3_routes.route takes."""
    a = acts_of(c, kind)
    return {"n": c.n, "kc": c.k, "ih": c.ih, "iw": c.iw, "m": c.m, "oh": c.oh, "ow": c.ow, "dr": [t[0] for t in c.taps],
            "dc": [t[1] for t in c.taps], "in_act": a["in_act"], "dact": a["dact"], "out_act": a["out_act"],
            "gate": 1 + a["gate"] if c.form == "gate" else 0, "flags": flags_of(c, kind, fused_res), "form": c.form}


def route(lib, c, kind, fused_res=False):
    rc, r = R.route(lib, problem(c, kind, fused_res))
    assert rc == 0, (c.name, kind, rc, lib.pg_last_error())
    return R.named(r)


KEY_FIELDS = ("kernel", "MT", "CG", "MS", "GT", "gelu", "two_tiles")


def key_of(r):
    """(kernel name, MT, CG, MS, GT, gelu, two_tiles, NT): the template arguments that name the instantiation."""
    return (R.KERNELS[r["kernel"]],) + tuple(r[f] for f in KEY_FIELDS[1:]) + (r["NT"],)


def route_problems(c, r, kind):
    """What the route shows that the case's entry does not say (empty = the case runs what it names)."""
    a = acts_of(c, kind)
    gelu = int(ACT_GELU in (a["in_act"], a["out_act"], a["dact"]))
    bad = [f"{k} = {r[k]} instead of {v}" for k, v in c.want.items() if r[k] != v]
    if r["gelu"] != gelu:
        bad.append(f"gelu = {r['gelu']} instead of {gelu}")
    return bad


def fmt_of(lib, c):
    hr = max(t[0] for t in c.taps) - min(t[0] for t in c.taps)
    hc = max(t[1] for t in c.taps) - min(t[1] for t in c.taps)
    return lib.pg_conv_mfma_supported(c.k, c.m, len(c.taps), c.oh, c.ow, c.iw, hr, hc)


# ---- inputs ------------------------------------------------------------------------------------------------------------------------------

def _signs(shape, g):
    return torch.randint(0, 2, shape, generator=g).float() * 2 - 1


def _sparse_rows(m, per_row, nnz, g):
    """(m, per_row) 0 / 1 mask with exactly min(nnz, per_row // 2 + 1) ones per row."""
    keep = min(nnz, per_row // 2 + 1)
    order = torch.rand(m, per_row, generator=g).argsort(dim=1)
    return (order < keep).float()


def weight_shape(c):
    return (c.m, c.k, c.kh, c.kw) if c.orient == "fwd" else (c.k, c.m, c.kh, c.kw)


def wsel_of(c, w):
    """Wsel (M, K, T) of a weight in its torch layout."""
    sel = torch.stack([w[:, :, u, v] for _, _, u, v in c.taps], dim=2)
    return sel if c.orient == "fwd" else sel.transpose(0, 1).contiguous()


def _weight_from_rows(c, rows):
    """rows (M, K * T) in the order [k][t] -> the torch layout."""
    sel = rows.reshape(c.m, c.k, len(c.taps))
    w = torch.zeros(weight_shape(c))
    for t, (_, _, u, v) in enumerate(c.taps):
        if c.orient == "fwd":
            w[:, :, u, v] = sel[:, :, t]
        else:
            w[:, :, u, v] = sel[:, :, t].t()
    return w


@functools.lru_cache(maxsize=None)
def inputs(name, kind):
    """dict of float32 CPU tensors: x (N, K, IH, IW), w (torch layout), bias (M) or None (data gradients have none), res, res2 (N, M,
    OH, OW), dact_src (same), gate_res (N, M / 2, OH, OW), r (dual). Every form finds what it needs; what it does not name it ignores."""
    c = BY_NAME[name]
    i = CASES.index(c)
    g = torch.Generator().manual_seed(104729 * i + 17 * KINDS.index(kind) + 3)
    xs, os_ = (c.n, c.k, c.ih, c.iw), (c.n, c.m, c.oh, c.ow)
    kt = c.k * len(c.taps)
    d = {}
    if kind == "random":
        d["x"] = torch.randn(xs, generator=g)
        d["w"] = torch.randn(weight_shape(c), generator=g) * 0.2
        d["bias"] = torch.randn(c.m, generator=g)
        for k in ("res", "res2", "dact_src"):
            d[k] = torch.randn(os_, generator=g)
        d["gate_res"] = torch.randn((c.n, max(c.m // 2, 1), c.oh, c.ow), generator=g)
        # dual: dact_src = elu(a) + r with r = elu(b), as PixelSNAIL's block tail stores them
        d["r"] = _small_ref.elu(torch.randn(os_, generator=g), torch.float32)
        if c.form == "dual":
            d["dact_src"] = _small_ref.elu(torch.randn(os_, generator=g), torch.float32) + d["r"]
    else:
        unit, ou = UNIT[kind], OPERAND_UNITS[kind]
        if kind == "int":
            d["x"] = torch.randint(-8, 9, xs, generator=g).float()
            rows = torch.randint(-4, 5, (c.m, kt), generator=g).float() * (torch.rand(c.m, kt, generator=g) < 0.28).float()
        elif kind == "x3":
            b = torch.randint(0, 2, xs, generator=g).float() * 2 + 1
            cc = torch.randint(0, 2, xs, generator=g).float() * 2 + 1
            d["x"] = _signs(xs, g) * (1 + b * 2.0 ** -8 + cc * 2.0 ** -16)
            rows = _signs((c.m, kt), g) * _sparse_rows(c.m, kt, NNZ[kind], g)
        elif kind == "w3":
            d["x"] = torch.randint(-1, 2, xs, generator=g).float()
            rows = _signs((c.m, kt), g) * (1 + 2.0 ** -9 + 2.0 ** -18) * _sparse_rows(c.m, kt, NNZ[kind], g)
        else:
            d["x"] = _signs(xs, g) * (1 + 2.0 ** -9)
            rows = _signs((c.m, kt), g) * (1 + 2.0 ** -9) * _sparse_rows(c.m, kt, NNZ[kind], g)
        d["w"] = _weight_from_rows(c, rows)
        d["bias"] = torch.randint(-ou, ou + 1, (c.m,), generator=g).float() * unit
        for k in ("res", "res2"):
            d[k] = torch.randint(-ou, ou + 1, os_, generator=g).float() * unit
        d["gate_res"] = torch.randint(-ou, ou + 1, (c.n, max(c.m // 2, 1), c.oh, c.ow), generator=g).float() * unit
        d["dact_src"] = torch.randint(-3, 4, os_, generator=g).float()
        d["r"] = torch.randint(-2, 4, os_, generator=g).float()
        if c.form == "dual":  # dact_src > 0 and dact_src - r an integer >= -2: every ELU derivative is -1, 0 or 1
            d["dact_src"] = torch.randint(1, 5, os_, generator=g).float()
    if c.orient == "dgrad":
        d["bias"] = None
    return d


# ---- the float64 reference ---------------------------------------------------------------------------------------------------------------

def act64(t, act):
    return t.double() if not act else _small_ref.ACT_FWD[ACTS[act]](t)


def act_grad64(t, act):
    if not act:
        return torch.ones_like(t, dtype=torch.float64)
    if act == ACT_ELU_OUT:
        return _small_ref.elu_grad_from_out(t)
    return _small_ref.ACT_GRAD[ACTS[act]](t)


def conv64(c, x64, wsel64):
    """sum_t sum_k Wsel[m][k][t] x[n, k, r + dr[t], c + dc[t]], zero outside the input: (N, M, OH, OW) float64."""
    out = torch.zeros(c.n, c.m, c.oh, c.ow, dtype=torch.float64)
    for t, (dr, dc, _, _) in enumerate(c.taps):
        r0, r1 = max(0, -dr), min(c.oh, c.ih - dr)
        c0, c1 = max(0, -dc), min(c.ow, c.iw - dc)
        if r1 > r0 and c1 > c0:
            out[:, :, r0:r1, c0:c1] += torch.einsum("mk,nkpq->nmpq", wsel64[:, :, t], x64[:, :, r0 + dr:r1 + dr, c0 + dc:c1 + dc])
    return out


def epilogue64(c, kind, conv, d, a, fused_res=False):
    """The case's epilogue on a float64 convolution result -> {"out": ..} (+ "gate_out" / "out2")."""
    v = conv if d["bias"] is None else conv + d["bias"].double().reshape(1, -1, 1, 1)
    v = act64(v, a["out_act"])
    flags = FORM_FLAGS[c.form]
    if c.form == "dual":
        dd = v * act_grad64(d["dact_src"], a["dact"])
        return {"out": dd * _small_ref.elu_grad_from_out(d["dact_src"], d["r"]), "out2": dd * _small_ref.elu_grad_from_out(d["r"])}
    if flags & R.DACT_SRC:
        v = v * act_grad64(d["dact_src"], a["dact"])
    if c.form == "gate":
        has_res, has_gate_res = gate_operands(c, kind)
        if has_res:
            v = v + d["res"].double()
        return {"out": v, "gate_out": _small_ref.gated_fwd(v, a["gate"], d["gate_res"] if has_gate_res else None)}
    if flags & R.RES or fused_res:
        v = v + d["res"].double()
    if flags & R.RES2:
        v = v + (d["res"] if flags & R.RES2_SAME else d["res2"]).double()
    return {"out": v}


def reference_of(c, kind, d, fused_res=False, absolute=False):
    """The float64 reference of (case, kind) on the inputs d. absolute = True: sum |w| |in_act(x)| + |bias| + |res| + |res2| per output
    (the bound on every partial sum of any summation order; dual: the sum alone, its two outputs are it times -1, 0 or 1)."""
    a = acts_of(c, kind)
    x64, wsel = act64(d["x"], a["in_act"]), wsel_of(c, d["w"]).double()
    if not absolute:
        return epilogue64(c, kind, conv64(c, x64, wsel), d, a, fused_res)
    b = conv64(c, x64.abs(), wsel.abs())
    if c.form == "dual":
        return {"out": b}
    if d["bias"] is not None:
        b = b + d["bias"].double().abs().reshape(1, -1, 1, 1)
    flags = FORM_FLAGS[c.form]
    if flags & R.RES or fused_res or (c.form == "gate" and gate_operands(c, kind)[0]):
        b = b + d["res"].double().abs()
    if flags & R.RES2:
        b = b + (d["res"] if flags & R.RES2_SAME else d["res2"]).double().abs()
    return {"out": b}


@functools.lru_cache(maxsize=None)
def reference(name, kind, fused_res=False):
    return reference_of(BY_NAME[name], kind, inputs(name, kind), fused_res)


def torch_reference(c, kind, d, fused_res=False, dtype=torch.float64):
    """The same statement through torch's own operators, in `dtype`: F.conv2d (autograd for the data gradients), F.relu / F.elu /
    F.gelu, their derivatives by autograd, torch.tanh / torch.sigmoid. In float64 it guards the hand-written reference against a slip
    (tests/test_conv_cases_cpu.py); in float32 it is the "fp32 torch-CPU convolution" whose error the GPU tier records beside the
    kernels'."""
    a = acts_of(c, kind)
    fn = {0: lambda t: t, 1: F.relu, 2: F.elu, 3: F.gelu}
    x, w = fn[a["in_act"]](d["x"].to(dtype)), d["w"].to(dtype)
    pad = (PAD[c.kh], PAD[c.kw])
    if c.orient == "fwd":
        conv = F.conv2d(x, w, None, padding=pad)[:, :, :c.oh, :c.ow]
    else:
        xf = torch.zeros(c.n, c.m, c.oh, c.ow, dtype=dtype, requires_grad=True)
        F.conv2d(xf, w, None, padding=pad)[:, :, :c.ih, :c.iw].backward(x)
        conv = xf.grad
    v = conv if d["bias"] is None else conv + d["bias"].to(dtype).view(1, -1, 1, 1)
    v = fn[a["out_act"]](v)

    def grad_of(src, act):
        if act == ACT_ELU_OUT:
            s = src.to(dtype)
            return torch.where(s > 0, torch.ones_like(s), s + 1)
        s = src.to(dtype).clone().requires_grad_(True)
        fn[act](s).sum().backward()
        return s.grad

    flags = FORM_FLAGS[c.form]
    if c.form == "dual":
        dd = v * grad_of(d["dact_src"], a["dact"])
        return {"out": dd * grad_of(d["dact_src"].to(dtype) - d["r"].to(dtype), ACT_ELU_OUT), "out2": dd * grad_of(d["r"], ACT_ELU_OUT)}
    if flags & R.DACT_SRC:
        v = v * grad_of(d["dact_src"], a["dact"])
    if c.form == "gate":
        has_res, has_gate_res = gate_operands(c, kind)
        if has_res:
            v = v + d["res"].to(dtype)
        h = c.m // 2
        y = (torch.tanh(v[:, :h]) if a["gate"] == 0 else v[:, :h]) * torch.sigmoid(v[:, h:])
        return {"out": v, "gate_out": y + d["gate_res"].to(dtype) if has_gate_res else y}
    if flags & R.RES or fused_res:
        v = v + d["res"].to(dtype)
    if flags & R.RES2:
        v = v + (d["res"] if flags & R.RES2_SAME else d["res2"]).to(dtype)
    return {"out": v}


# ---- the bf16 pieces, emulated -------------------------------------------------------------------------------------------------------------

def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def _bf16_rne(x):
    """float32 -> the nearest bf16 (ties to even), as a float32 array."""
    b = _bits(x)
    b = (b + np.uint32(0x7FFF) + ((b >> np.uint32(16)) & np.uint32(1))) & np.uint32(0xFFFF0000)
    return b.view(np.float32)


def _bf16_trunc(x):
    return (_bits(x) & np.uint32(0xFFFF0000)).view(np.float32)


def split8(x):
    """The pack's split (csrc/conv_b3_kernels.h: split8), round to nearest: (h, m, l) float32 arrays that are bf16 values."""
    x = np.asarray(x, dtype=np.float32)
    h = _bf16_rne(x)
    r1 = (x - h).astype(np.float32)
    m = _bf16_rne(r1)
    return h, m, _bf16_rne((r1 - m).astype(np.float32))


def split8t(x):
    """The staging split (split8t), truncation: h = top 16 bits of x, m = top 16 bits of x - h, l = top 16 bits of x - h - m."""
    x = np.asarray(x, dtype=np.float32)
    h = _bf16_trunc(x)
    r1 = (x - h).astype(np.float32)
    m = _bf16_trunc(r1)
    return h, m, _bf16_trunc((r1 - m).astype(np.float32))


def six_products(c, kind, d, without=(), only=None):
    """The case's result with the convolution formed as the kernels form it: sum over PRODUCTS of conv(piece of w, piece of
    in_act(x)), each in float64 (a bf16 x bf16 product and their sums are exact there), then the epilogue. `without`: products left
    out; `only`: the products to sum instead."""
    a = acts_of(c, kind)
    xa = act64(d["x"], a["in_act"]).float().numpy()
    wp = dict(zip(("w0", "w1", "w2"), (torch.from_numpy(p.copy()).double() for p in split8(wsel_of(c, d["w"]).numpy()))))
    xp = dict(zip(("xh", "xm", "xl"), (torch.from_numpy(p.copy()).double() for p in split8t(xa))))
    conv = torch.zeros(c.n, c.m, c.oh, c.ow, dtype=torch.float64)
    for p in (only if only is not None else PRODUCTS):
        if p not in without:
            wn, xn = p.split(".")
            conv += conv64(c, xp[xn], wp[wn])
    return conv if only is not None else epilogue64(c, kind, conv, d, a)
