"""The weight-gradient cases shared by tests/test_wgrad_route_cpu.py and tests/test_gpu_wgrad_families.py: one entry per kernel
instantiation `pg_conv2d_wgrad` can launch (csrc/conv_wgrad.hip: wgrad_route) and per edge of its dispatch, the inputs of both kinds,
and a plain float64 reference.

A case names the family and the template integers its launch must show (the CPU test and the GPU test both ask
`pg_conv2d_wgrad_route` first). The problem is a convolution (kh x kw filter, padding ph / pw, output cropped to oh x ow) with an
optional list of active taps: tap (u, v) reads x at row offset u - ph and column offset v - pw.

Inputs, per case:
  exact   x integer-valued in [-8, 8], dy integer-valued in [-4, 4] with about a quarter non-zero, activation none or ReLU: every
          product and every partial sum is an integer below 2^24 (asserted from the reference), so bf16x3 and fp32 kernels must return
          the float64 reference bit for bit in any summation order;
  random  seeded normal x and dy, the four activations rotated over the cases.
"""

import collections
import functools

import torch

import _small_ref

FAMILIES = ("x-copy", "ring", "shifted-dy", "1x1", "input", "generic")
FIELDS = ["family", "t0", "t1", "t2", "t3", "grid_x", "grid_y", "grid_z", "block", "lds_bytes", "G", "TR", "tiles_per_img", "total",
          "nseg", "seg_rows", "PBR", "vec_dy", "vec_x", "red_grid", "hr", "copies", "passes", "max_rows"]
HAS_BIAS, X_MISALIGNED, DY_MISALIGNED = 1, 2, 4  # include/pg_hip.h: PG_WGR_*
ACTS = (None, "relu", "elu", "gelu")              # index = PG_ACT_*
KINDS = ("exact", "random")
N_INST = {"x-copy": 4, "ring": 3, "shifted-dy": 2, "1x1": 2, "input": 0, "generic": 3}  # template integers that identify a kernel
LDS_LIMIT = {"x-copy": 76 * 1024, "ring": 150 * 1024, "shifted-dy": 76 * 1024, "1x1": 64 * 1024, "input": 64 * 1024,
             "generic": 160 * 1024}

Case = collections.namedtuple("Case", "name family inst n cin ih iw cout kh kw ph pw oh ow active mis want")


def C(name, family, inst, n, cin, h, w, cout, k, out=None, active=None, mis="", **want):
    kh, kw, ph, pw = k
    oh, ow = out or (h, w)
    assert oh <= h + 2 * ph - kh + 1 and ow <= w + 2 * pw - kw + 1, name
    return Case(name, family, tuple(inst), n, cin, h, w, cout, kh, kw, ph, pw, oh, ow, active, mis, want)


K11, K12, K13, K21, K22, K23, K33 = (1, 1, 0, 0), (1, 2, 0, 1), (1, 3, 0, 1), (2, 1, 1, 0), (2, 2, 1, 1), (2, 3, 1, 1), (3, 3, 1, 1)
K55, K77, K14 = (5, 5, 2, 2), (7, 7, 3, 3), (1, 4, 0, 3)
MASK_A = [(0, 0), (0, 1), (0, 2), (1, 0)]            # 3x3 type A: an L-shaped list, not a full grid
MASK_B = MASK_A + [(1, 1)]                           # 3x3 type B: five taps
SCATTER3 = [(0, 0), (1, 2), (2, 1)]                  # three taps of a 3x3 that form no grid
SCATTER6 = [(0, 1), (0, 2), (1, 2), (2, 0), (2, 1), (2, 2)]  # six taps of a 3x3 that form no grid
COLUMNS9 = [(u, v) for u in (0, 2, 4) for v in (1, 2, 3)]  # nine taps of a 5x5 over five rows: no 3x3 grid

CASES = [
    # ---- x-copy bf16x3: conv_wgrad_b3_kernel<T, MR, waves, CIT> --------------------------------------------------------------------
    C("xcopy-1tap-32to64", "x-copy", (1, 2, 8, 2), 3, 32, 8, 8, 64, K11),
    C("xcopy-1tap-96to64", "x-copy", (1, 2, 8, 2), 2, 96, 8, 8, 64, K11),
    C("xcopy-1tap-big-64to64", "x-copy", (1, 2, 8, 4), 3, 64, 8, 8, 64, K11),
    C("xcopy-1tap-big-64to128", "x-copy", (1, 4, 8, 4), 2, 64, 16, 16, 128, K11),
    C("xcopy-2tap-big", "x-copy", (2, 2, 8, 4), 3, 64, 12, 16, 64, K21),
    C("xcopy-2tap", "x-copy", (2, 2, 8, 2), 3, 32, 12, 16, 64, K21),
    C("xcopy-3tap", "x-copy", (3, 2, 8, 2), 2, 32, 10, 16, 128, K13),
    C("xcopy-4tap", "x-copy", (4, 2, 8, 2), 3, 32, 8, 8, 64, K22),
    C("xcopy-6tap", "x-copy", (6, 2, 4, 2), 2, 64, 12, 8, 64, K23),
    C("xcopy-L-4tap-32out", "x-copy", (4, 1, 4, 2), 3, 32, 8, 8, 32, K33, active=MASK_A),
    C("xcopy-L-4tap-64out", "x-copy", (4, 2, 8, 2), 2, 32, 16, 16, 64, K33, active=MASK_A),
    C("xcopy-1x2-32out", "x-copy", (2, 1, 4, 2), 3, 32, 8, 16, 32, K12),
    C("xcopy-scatter3-32out", "x-copy", (3, 1, 4, 2), 2, 32, 8, 8, 32, K33, active=SCATTER3),
    C("xcopy-scatter6-32out", "x-copy", (6, 1, 4, 2), 2, 32, 8, 8, 32, K33, active=SCATTER6),
    C("xcopy-9tap-5rows-64out", "x-copy", (9, 2, 4, 2), 2, 32, 8, 8, 64, K55, active=COLUMNS9),
    C("xcopy-9tap-5rows-32out", "x-copy", (9, 1, 4, 2), 2, 32, 8, 8, 32, K55, active=COLUMNS9),
    C("xcopy-w12", "x-copy", (4, 2, 8, 2), 3, 32, 12, 12, 64, K22),
    C("xcopy-w20", "x-copy", (2, 2, 8, 2), 2, 32, 6, 20, 64, K21),
    C("xcopy-w28-ragged-rows", "x-copy", (2, 2, 8, 2), 2, 96, 7, 28, 64, K21),
    C("xcopy-one-row-per-tile-w64", "x-copy", (4, 2, 8, 2), 1, 32, 6, 64, 64, K22),
    # ---- row ring (OW == 32): conv_wgrad_b3r_kernel<T, WM, WN> -------------------------------------------------------------------------
    C("ring-2tap-n1-segments", "ring", (2, 1, 2), 1, 64, 32, 32, 64, K21, nseg=4, seg_rows=8),
    C("ring-3tap", "ring", (3, 1, 2), 2, 64, 32, 32, 64, K13),
    C("ring-4tap-n3", "ring", (4, 1, 2), 3, 64, 32, 32, 64, K22, nseg=4),
    C("ring-6tap", "ring", (6, 1, 2), 3, 128, 32, 32, 64, K23),
    C("ring-L-4tap", "ring", (4, 1, 2), 2, 64, 32, 32, 64, K33, active=MASK_A),
    C("ring-4tap-n20", "ring", (4, 1, 2), 20, 64, 32, 32, 64, K22, nseg=4, G=80),
    C("ring-2tap-128x64", "ring", (2, 2, 2), 2, 128, 32, 32, 256, K21),
    C("ring-3tap-128x64", "ring", (3, 2, 2), 2, 64, 32, 32, 128, K13),
    C("ring-4tap-128x64", "ring", (4, 2, 2), 2, 64, 32, 32, 128, K22),
    C("ring-2tap-256x64", "ring", (2, 4, 2), 2, 256, 32, 32, 256, K12),
    C("ring-1tap-128x128", "ring", (1, 2, 4), 2, 128, 32, 32, 128, K11),
    C("ring-16-rows", "ring", (2, 1, 2), 1, 64, 16, 32, 64, K21, nseg=2, seg_rows=8),
    # ---- shifted dy: conv_wgrad_b3s_kernel<NR, NC> -----------------------------------------------------------------------------------------
    C("shifted-3x3-32out", "shifted-dy", (3, 3), 3, 32, 8, 8, 32, K33),
    C("shifted-3x3-96out", "shifted-dy", (3, 3), 2, 32, 12, 12, 96, K33),
    C("shifted-3x3-64out", "shifted-dy", (3, 3), 3, 64, 16, 16, 64, K33),
    C("shifted-2x2-32out", "shifted-dy", (2, 2), 5, 32, 16, 32, 32, K22),
    C("shifted-2x2-96out", "shifted-dy", (2, 2), 2, 32, 8, 8, 96, K22),
    C("shifted-1x3-32out-w20", "shifted-dy", (1, 3), 3, 32, 10, 20, 32, K13),
    C("shifted-1x3-96out", "shifted-dy", (1, 3), 2, 64, 8, 8, 96, K13),
    C("shifted-2x1-32out", "shifted-dy", (2, 1), 3, 32, 9, 16, 32, K21),
    C("shifted-2x1-96out", "shifted-dy", (2, 1), 3, 32, 9, 16, 96, K21),
    C("shifted-2x3-32out-ragged-rows", "shifted-dy", (2, 3), 3, 64, 8, 16, 32, K23, TR=6),
    C("shifted-2x3-96out-w28", "shifted-dy", (2, 3), 2, 32, 7, 28, 96, K23),
    C("shifted-3x3-w64-one-row", "shifted-dy", (3, 3), 1, 32, 5, 64, 32, K33),
    # ---- fp32 1x1: conv_wgrad_pw_kernel<NCOT, NCIT, ACT> -----------------------------------------------------------------------------------
    C("pw-1x1", "1x1", (1, 1), 3, 16, 8, 8, 16, K11),
    C("pw-1x2", "1x1", (1, 2), 2, 32, 8, 8, 16, K11),
    C("pw-1x4", "1x1", (1, 4), 2, 64, 16, 16, 16, K11),
    C("pw-2x1", "1x1", (2, 1), 3, 16, 14, 14, 32, K11),
    C("pw-2x2", "1x1", (2, 2), 2, 24, 8, 8, 32, K11),
    C("pw-2x4", "1x1", (2, 4), 4, 128, 8, 8, 32, K11),
    C("pw-3x1", "1x1", (3, 1), 2, 12, 8, 8, 48, K11),
    C("pw-3x2", "1x1", (3, 2), 2, 32, 6, 6, 48, K11),
    C("pw-3x4-48out", "1x1", (3, 4), 2, 64, 8, 8, 48, K11),
    C("pw-3x4-ragged-69to36", "1x1", (3, 4), 2, 69, 16, 16, 36, K11),
    C("pw-4x1", "1x1", (4, 1), 3, 16, 28, 28, 64, K11),
    C("pw-4x2", "1x1", (4, 2), 2, 24, 8, 8, 64, K11),
    C("pw-4x4", "1x1", (4, 4), 2, 48, 10, 10, 72, K11),
    # ---- input layers: conv_wgrad_small_kernel ---------------------------------------------------------------------------------------------
    C("input-7x7-1ch", "input", (), 2, 1, 28, 28, 64, K77),
    C("input-3x3-3ch", "input", (), 2, 3, 32, 32, 64, K33),
    C("input-1x4-3ch", "input", (), 2, 3, 12, 12, 32, K14),
    # ---- generic fp32: conv_wgrad_kernel<NT, NC, prefetch> ---------------------------------------------------------------------------------
    C("generic-1tap-L49", "generic", (1, 1, 0), 2, 5, 7, 7, 3, K11),
    C("generic-1tap-2ci-L49", "generic", (1, 2, 0), 2, 24, 7, 7, 40, K11),
    C("generic-1tap-pf", "generic", (1, 1, 1), 2, 8, 8, 8, 16, K33, active=[(1, 1)]),
    C("generic-1tap-2ci-pf", "generic", (1, 2, 1), 2, 24, 8, 8, 16, K33, active=[(0, 1)]),
    C("generic-2tap", "generic", (2, 1, 0), 2, 16, 9, 11, 16, K21),
    C("generic-2tap-2ci", "generic", (2, 2, 0), 2, 24, 9, 10, 40, K12),
    C("generic-2tap-pf", "generic", (2, 1, 1), 2, 16, 12, 12, 32, K21),
    C("generic-2tap-2ci-pf", "generic", (2, 2, 1), 2, 40, 12, 12, 32, K12),
    C("generic-3tap", "generic", (3, 1, 0), 2, 8, 9, 11, 24, K13),
    C("generic-3tap-2ci", "generic", (3, 2, 0), 2, 33, 6, 6, 10, K13),
    C("generic-3tap-pf", "generic", (3, 1, 1), 2, 16, 12, 12, 32, K13),
    C("generic-3tap-2ci-pf", "generic", (3, 2, 1), 2, 48, 8, 12, 40, K13),
    C("generic-4tap", "generic", (4, 1, 0), 2, 16, 7, 7, 16, K22),
    C("generic-4tap-2ci", "generic", (4, 2, 0), 2, 40, 7, 9, 24, K22),
    C("generic-4tap-pf", "generic", (4, 1, 1), 2, 16, 8, 8, 16, K22),
    C("generic-4tap-2ci-pf", "generic", (4, 2, 1), 2, 24, 8, 16, 72, K22),
    C("generic-5tap-4+1", "generic", (4, 1, 0), 2, 5, 9, 11, 7, K33, active=MASK_B, passes=2),
    C("generic-5tap-4+1-2ci-pf", "generic", (4, 2, 1), 2, 24, 8, 8, 40, K33, active=MASK_B, passes=2),
    C("generic-9tap", "generic", (9, 1, 0), 2, 5, 9, 11, 7, K33),
    C("generic-9tap-2ci", "generic", (9, 2, 0), 2, 20, 6, 7, 24, K33),
    C("generic-9tap-pf-64x64", "generic", (9, 1, 1), 1, 4, 64, 64, 8, K33),
    C("generic-9tap-2ci-pf", "generic", (9, 2, 1), 2, 24, 8, 8, 24, K33),
    C("generic-25tap-9+9+7", "generic", (9, 1, 1), 2, 8, 8, 8, 16, K55, passes=3),
    C("generic-25tap-2ci", "generic", (9, 2, 0), 2, 20, 7, 7, 24, K55, passes=3),
    C("generic-49tap-8ch", "generic", (9, 1, 1), 2, 8, 12, 12, 16, K77, passes=6),
    C("generic-49tap-2ci", "generic", (9, 2, 0), 1, 24, 9, 9, 8, K77, passes=6),
    C("generic-oh-plus-1", "generic", (2, 2, 1), 2, 32, 8, 8, 32, K21, out=(9, 8)),
    C("generic-oh-plus-1-small", "generic", (2, 1, 0), 3, 8, 5, 6, 16, K21, out=(6, 6)),
    C("generic-valid-3x3", "generic", (9, 2, 0), 2, 32, 10, 10, 32, (3, 3, 0, 0), out=(8, 8)),
    C("generic-valid-3x3-64ch", "generic", (9, 2, 0), 2, 64, 12, 14, 64, (3, 3, 0, 0), out=(10, 12)),
    # ---- misaligned operands: every fast family declines -----------------------------------------------------------------------------------
    C("misaligned-x-3x3", "generic", (9, 2, 0), 2, 32, 8, 8, 32, K33, mis="x", vec_x=0, vec_dy=1),
    C("misaligned-dy-2x2-ring-shape", "generic", (4, 2, 0), 1, 64, 32, 32, 64, K22, mis="dy", vec_x=1, vec_dy=0),
    C("misaligned-both-1x1", "generic", (1, 2, 0), 2, 64, 8, 8, 64, K11, mis="xdy", vec_x=0, vec_dy=0),
    C("misaligned-x-1x1-pw-shape", "generic", (1, 1, 0), 2, 16, 8, 8, 16, K11, mis="x", vec_x=0, vec_dy=1),
    C("misaligned-x-input-layer", "input", (), 2, 3, 12, 12, 32, K33, mis="x"),
    C("misaligned-dy-input-layer", "generic", (9, 1, 0), 2, 3, 12, 12, 32, K33, mis="dy", vec_dy=0),
    # ---- the reduction's row loop: G = 1, G % 4 != 0, 32 < G < 64 with a remainder, G at the family's cap -------------------------------
    C("rows-1-generic", "generic", (9, 1, 1), 1, 8, 8, 8, 16, K33, G=1),
    C("rows-1-pw", "1x1", (1, 1), 1, 16, 4, 4, 16, K11, G=1),
    C("rows-3-shifted", "shifted-dy", (3, 3), 3, 32, 8, 8, 32, K33, G=3),
    C("rows-5-input", "input", (), 5, 3, 8, 8, 32, K33, G=5),
    C("rows-45-generic", "generic", (4, 1, 1), 45, 8, 4, 4, 16, K22, G=45),
    C("rows-45-xcopy", "x-copy", (2, 2, 8, 2), 45, 32, 4, 8, 64, K21, G=45),
    C("rows-37-shifted", "shifted-dy", (2, 2), 37, 32, 4, 8, 32, K22, G=37),
    C("rows-cap-generic", "generic", (3, 2, 1), 130, 40, 4, 4, 72, K13, G=128),
    C("rows-cap-xcopy", "x-copy", (2, 2, 8, 4), 70, 128, 4, 8, 256, K21, G=64),
    C("rows-cap-shifted", "shifted-dy", (2, 1), 90, 64, 4, 8, 96, K21, G=85),
    C("rows-cap-pw", "1x1", (4, 4), 64, 72, 16, 16, 256, K11, G=64),
    C("rows-cap-ring", "ring", (4, 2, 2), 33, 128, 32, 32, 256, K22, G=64),
    C("rows-cap-input", "input", (), 260, 3, 4, 4, 128, K33, G=256),
]
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)


def taps(c):
    """[(dr, dc, u, v)] of the case's active taps, in the order the C ABI gets them."""
    act = c.active if c.active is not None else [(u, v) for u in range(c.kh) for v in range(c.kw)]
    return [(u - c.ph, v - c.pw, u, v) for u, v in act]


def flags_of(c, bias=True):
    return (HAS_BIAS if bias else 0) | (X_MISALIGNED if "x" in c.mis else 0) | (DY_MISALIGNED if "dy" in c.mis else 0)


def in_act(c, kind):
    """Activation id of the case's `kind`: none / ReLU alternate over the table for the exact inputs, all four rotate for the random."""
    i = CASES.index(c)
    return (i % 2) if kind == "exact" else (i + 1) % 4


def route_problem(lib, n, cin, ih, iw, cout, oh, ow, kh, kw, dr, dc, act=0, flags=HAS_BIAS):
    """(status, {field: int}) from pg_conv2d_wgrad_route."""
    import ctypes

    out = (ctypes.c_int * len(FIELDS))()
    ia = ctypes.c_int * len(dr)
    rc = lib.pg_conv2d_wgrad_route(n, cin, ih, iw, cout, oh, ow, kh, kw, len(dr), ia(*dr), ia(*dc), act, flags, out, len(FIELDS))
    return rc, dict(zip(FIELDS, out))


def route(lib, c, kind="exact", bias=True):
    t = taps(c)
    rc, r = route_problem(lib, c.n, c.cin, c.ih, c.iw, c.cout, c.oh, c.ow, c.kh, c.kw, [a[0] for a in t], [a[1] for a in t],
                          in_act(c, kind), flags_of(c, bias))
    assert rc == 0, (c.name, rc, lib.pg_last_error())
    return r


def key_of(r):
    """(family name, the template integers that name the kernel): the 1x1 kernel's activation argument is the problem's own."""
    fam = FAMILIES[r["family"]]
    return (fam,) + tuple(r[f"t{i}"] for i in range(N_INST[fam]))


def route_problems(c, r, kind="exact"):
    """What the route shows that the case's entry does not say (empty = the case runs what it names)."""
    bad = []
    if key_of(r) != (c.family,) + c.inst:
        bad.append(f"kernel {key_of(r)} instead of {(c.family,) + c.inst}")
    if c.family == "1x1" and r["t2"] != in_act(c, kind):
        bad.append(f"activation argument {r['t2']}")
    bad += [f"{k} = {r[k]} instead of {v}" for k, v in c.want.items() if r[k] != v]
    return bad


# ---- inputs and the float64 reference ------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def inputs(name, kind):
    """(x, dy) float32 on the CPU, seeded by the case's position."""
    c = BY_NAME[name]
    g = torch.Generator().manual_seed(7919 * CASES.index(c) + (1 if kind == "exact" else 2))
    xs, ds = (c.n, c.cin, c.ih, c.iw), (c.n, c.cout, c.oh, c.ow)
    if kind == "exact":
        x = torch.randint(-8, 9, xs, generator=g).float()
        dy = torch.randint(-4, 5, ds, generator=g).float() * (torch.rand(ds, generator=g) < 0.28).float()
        return x, dy
    return torch.randn(xs, generator=g), torch.randn(ds, generator=g)


def activation64(x, act):
    return x.double() if not act else _small_ref.ACT_FWD[ACTS[act]](x)


def reference_of(x, dy, c, act, absolute=False):
    """dw (Cout, Cin, kh, kw), db (Cout) in float64: dw[co, ci, u, v] = sum_{n, r, c} dy[n, co, r, c] * act(x)[n, ci, r + u - ph,
    c + v - pw] over the pixels where the shifted x lies inside the image, zero at the taps that are not active. absolute = True:
    the same sums over |dy| and |act(x)| (the bound on every partial sum of any summation order)."""
    ax, d = activation64(x, act), dy.double()
    if absolute:
        ax, d = ax.abs(), d.abs()
    dw = torch.zeros(c.cout, c.cin, c.kh, c.kw, dtype=torch.float64)
    for dr, dc, u, v in taps(c):
        r0, r1 = max(0, -dr), min(c.oh, c.ih - dr)
        c0, c1 = max(0, -dc), min(c.ow, c.iw - dc)
        if r1 > r0 and c1 > c0:
            dw[:, :, u, v] = torch.einsum("nopq,nipq->oi", d[:, :, r0:r1, c0:c1], ax[:, :, r0 + dr:r1 + dr, c0 + dc:c1 + dc])
    return dw, d.sum(dim=(0, 2, 3))


@functools.lru_cache(maxsize=None)
def reference(name, kind):
    c = BY_NAME[name]
    x, dy = inputs(name, kind)
    return reference_of(x, dy, c, in_act(c, kind))


def prefill(shape):
    """Known small integers for dw / db before the call (the reduction ADDS to them)."""
    n = 1
    for s in shape:
        n *= s
    return ((torch.arange(n) * 5) % 7 - 3).float().reshape(shape)


# ---- the bench workloads ---------------------------------------------------------------------------------------------------------------

def bench_problems():
    """Every convolution of the eight bench workloads at every resolution its model runs it, enumerated like
    test_weight_gradient_planner_takes_every_layer_of_the_bench_workloads (tests/test_host_cpu.py), at batch 1 and 64:
    [(label, [n, cin, ih, iw, cout, oh, ow, kh, kw, dr list, dc list, bias])]."""
    import bench
    import pytorch_generative_amd as pg

    rows = []
    for name, w in bench.WORKLOADS.items():
        model = getattr(pg.models, w["ctor"])(**w["kw"])
        side = w["chw"][1]
        sides = [side] if name in ("image_gpt", "image_gpt_repro", "pixel_snail", "gated_pixel_cnn", "pixel_cnn") else \
            [s for s in (64, 32, 16, 8, 4, 2, 1) if s <= side]
        seen = set()
        for label, mod in model.named_modules():
            if not hasattr(mod, "_conv_spec") or getattr(mod, "weight", None) is None or mod.weight.dim() != 4:
                continue
            sp = mod._conv_spec()
            cout, cin = (int(v) for v in mod.weight.shape[:2])
            bias = int(getattr(mod, "bias", None) is not None)
            for s in sides:
                oh, ow = sp.full_out(s, s)
                oh, ow = min(oh, s), min(ow, s)  # the causal layers crop their output back to the input size
                key = (cin, cout, sp.kh, sp.kw, sp.pad_h, sp.pad_w, len(sp.wg_taps), s, oh, ow, bias)
                if key in seen or oh < 1 or ow < 1:
                    continue
                seen.add(key)
                for n in (1, 64):
                    rows.append((f"{name} {label} {s}x{s} N={n}",
                                 [n, cin, s, s, cout, oh, ow, sp.kh, sp.kw, list(sp.w_dr), list(sp.w_dc), bias]))
    return rows


def bench_routes(lib):
    """[[label, problem, route as a list in the order of FIELDS]] of bench_problems()."""
    out = []
    for label, pr in bench_problems():
        rc, r = route_problem(lib, *pr[:11], act=0, flags=HAS_BIAS if pr[11] else 0)
        assert rc == 0, (label, rc, lib.pg_last_error())
        out.append([label, pr, [r[f] for f in FIELDS]])
    return out
