"""GPU: every HIP kernel, called through the C-ABI (ctypes ops), against the CPU oracle on the
same seeded inputs. Tolerance for fp32 results: 1e-4 relative to the tensor's max magnitude
(BASELINE.json north_star); masks / positional encodings are bit-exact.

The convolutions here go through the Python layer at shapes chosen model by model, against an fp32 oracle. Every kernel family,
instantiation and epilogue form of the forward / data-gradient convolution is held to a float64 reference — bit for bit on inputs
that fill all three bf16 pieces — by tests/test_gpu_conv_families.py (cases: tests/_conv_cases.py), the weight gradient by
tests/test_gpu_wgrad_families.py."""

import os

import pytest
import torch
import torch.nn.functional as F

import _util
from oracle import ops as oops

pytestmark = pytest.mark.gpu

TOL = 1e-4


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need the MI355X"
    from pytorch_generative_amd import _lib

    _lib.load()  # fail loudly if the extension is missing
    return torch.device("cuda:0")


def _rand(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


CONV_CASES = [
    # (N, Cin, H, W, Cout, kh, kw, ph, pw, crop, active, in_act, use_res, use_bias)
    (2, 1, 28, 28, 16, 3, 3, 1, 1, None, "A", None, False, True),       # ImageGPT input conv
    (2, 3, 32, 32, 64, 3, 3, 1, 1, None, "A", None, False, True),       # PixelSNAIL input conv
    (2, 1, 28, 28, 64, 7, 7, 3, 3, None, "A", None, False, True),       # PixelCNN input conv
    (2, 32, 28, 28, 32, 3, 3, 1, 1, None, "B", "relu", False, True),    # PixelCNN residual conv
    (2, 64, 32, 32, 128, 2, 2, 1, 1, "hw", None, "elu", False, True),   # PixelSNAIL 2x2 (cropped)
    (2, 16, 12, 12, 32, 1, 3, 0, 1, None, None, None, False, True),     # gated vstack 1xN
    (2, 16, 12, 12, 32, 2, 1, 2, 0, "hw", None, None, False, True),     # gated vstack Nx1 (crop rows)
    (2, 16, 12, 12, 32, 1, 2, 0, 1, "hw", None, None, True, True),      # gated hstack 1xN + link res
    (2, 3, 12, 12, 32, 1, 4, 0, 4, "hw", None, None, False, True),      # gated input layer (k=7, mask_center)
    (3, 16, 28, 28, 64, 1, 1, 0, 0, None, None, None, False, True),     # 1x1 (vector path)
    (3, 64, 28, 28, 16, 1, 1, 0, 0, None, None, "gelu", True, True),    # 1x1 + fused gelu + residual
    (2, 69, 32, 32, 36, 1, 1, 0, 0, None, None, None, False, True),     # SNAIL _kv 69->36 (ragged channels)
    (2, 5, 7, 7, 3, 1, 1, 0, 0, None, None, "relu", False, False),      # L % 4 != 0 scalar path, no bias
    (2, 5, 9, 11, 7, 3, 3, 1, 1, None, "B", None, True, True),          # odd sizes, OW % 4 != 0
    (1, 4, 64, 64, 8, 3, 3, 1, 1, None, None, None, False, True),       # 64x64: several row tiles
    (17, 32, 4, 4, 32, 3, 3, 1, 1, None, None, "gelu", True, True),     # 4x4 images: 15 per tile, partial last group
    # shapes the bf16x3 weight-gradient kernels take (Cout % 64 == 0, Cin % 32 == 0, W % 8 == 0); which one, per row, is what
    # pg_conv2d_wgrad_route says (the weight gradient always runs ALL kh * kw taps here: wgrad_all) - tests/_wgrad_cases.py asserts it
    (3, 32, 16, 16, 64, 3, 3, 1, 1, None, "B", "relu", False, True),    # 9 taps: the full 3x3 grid goes to the shifted-dy kernel first
    (2, 64, 12, 8, 64, 2, 3, 1, 1, "hw", None, None, False, False),     # 6 taps, W = 8, no bias
    (2, 32, 10, 16, 128, 1, 3, 0, 1, None, None, "gelu", True, True),   # 3 taps, two co chunks
    (2, 96, 7, 24, 64, 2, 1, 2, 0, "hw", None, "elu", False, True),     # 2 taps, ragged last row tile
    (1, 32, 64, 64, 64, 2, 2, 1, 1, "hw", None, None, False, True),     # 64 wide: one row per tile
    # round 6: the row-ring weight-gradient kernel (conv_wgrad_b3r_kernel: 32-wide rows, 64 x 64 channels, x rows kept in an LDS ring).
    # Few images = row segments that start mid-image (their halo rows are loaded, not zero); 3 images = an idle tail of the grid
    (3, 64, 32, 32, 64, 2, 2, 1, 1, "hw", None, "elu", False, True),     # 2x2: two column copies, one halo row; 4 segments per image
    (1, 128, 32, 32, 64, 2, 1, 2, 0, "hw", None, "relu", True, True),    # 2x1: two taps, one copy, two ci chunks
    (2, 64, 32, 32, 128, 1, 3, 0, 1, None, None, None, False, True),     # 1x3: three copies, no halo (ring of one row), two co chunks
    (20, 64, 32, 32, 64, 2, 2, 1, 1, "hw", None, None, False, False),    # 20 images: whole-image units + segments, no bias
    (3, 128, 32, 32, 64, 2, 3, 1, 1, "hw", None, "relu", True, True),    # 2x3: six taps, three copies, 84 KB ring (one workgroup per CU)
    (2, 64, 32, 32, 64, 3, 3, 1, 1, None, "A", None, False, True),       # masked 3x3 type A: four taps forward; the weight gradient runs all nine, on the shifted-dy kernel (not the ring)
    (2, 128, 32, 32, 256, 2, 1, 2, 0, "hw", None, None, False, True),    # two taps: 128 x 64 wave tiles, two ci chunks
    (2, 256, 32, 32, 256, 1, 2, 0, 1, "hw", None, "elu", False, True),   # two taps 256 -> 256: the 256 x 64 tile
    # round 6: the overlapped 16-wave kernel (conv_b3q_kernel.h), two tiles per workgroup sharing one weight slab: 6 taps with >= 256
    # channels on one side (PixelCNN++'s 2x3 convolutions); odd batch = an idle half in the last round, Cout % 64 != 0 = a partial chunk
    (3, 320, 32, 32, 160, 2, 3, 1, 1, "hw", None, None, False, True),    # forward on Q (Cin 320), data gradient 160 -> 320 on Q too
    (5, 160, 32, 32, 320, 2, 3, 1, 1, "hw", None, "elu", True, True),    # + residual + fused input activation
    (2, 256, 24, 32, 96, 2, 3, 1, 1, "hw", None, None, False, False),    # 24 rows: ragged last row tile, 96 output channels
    # bench regime: N * tiles_per_img above the persistent grid -> several tiles per workgroup, ragged last round
    (300, 64, 32, 32, 64, 2, 2, 1, 1, "hw", None, "elu", True, True),   # PixelSNAIL 2x2 64->64: 1200 tiles / 512
    (150, 64, 32, 32, 128, 2, 2, 1, 1, "hw", None, "elu", False, True),  # 64->128: 600 tiles / 256 per chunk row
    (140, 69, 32, 32, 36, 1, 1, 0, 0, None, None, None, False, True),   # fp32-MFMA kernel (ragged channels), 560 tiles
    (30, 32, 64, 64, 64, 3, 3, 1, 1, None, None, "relu", False, True),  # 64x64 3x3: 22 row tiles per image
    (700, 32, 28, 28, 32, 3, 3, 1, 1, None, "B", "relu", False, True),  # PixelCNN residual conv at bench batch
    # 32 output channels on the bf16x3 weight-gradient kernels (round 3: one MFMA row tile per wave; these full 3x3 grids have since
    # moved to the shifted-dy kernel, the x-copy kernel's <T, 1> keeps the tap lists that are no grid)
    (3, 32, 16, 16, 32, 3, 3, 1, 1, None, "B", "relu", False, True),
    (20, 64, 32, 32, 32, 3, 3, 1, 1, None, None, "gelu", True, True),
    (2, 32, 8, 8, 32, 3, 3, 1, 1, None, None, "gelu", False, True),     # VD-VAE 8x8 level
    # 1x1 shapes the bf16x3 weight-gradient kernel takes since round 3 (T = 1)
    (3, 64, 16, 16, 128, 1, 1, 0, 0, None, None, "elu", True, True),
    (130, 32, 32, 32, 64, 1, 1, 0, 0, None, None, None, False, True),   # several pixel tiles per workgroup
    # 1x1 on the barrier-free bf16x3 kernel (conv_b3_pw_kernel): 1-4 output tiles, partial K groups, ragged pixel tiles
    (5, 64, 32, 32, 64, 1, 1, 0, 0, None, None, "elu", True, True),     # PixelSNAIL's 64 -> 64 + residual
    (4, 128, 32, 32, 32, 1, 1, 0, 0, None, None, "relu", False, True),  # four channel chunks, 32 output channels
    (3, 48, 14, 22, 96, 1, 1, 0, 0, None, None, "gelu", True, True),    # 16-channel chunks, partial co chunk, L = 308
    (600, 64, 28, 28, 32, 1, 1, 0, 0, None, None, "relu", False, True),  # PixelCNN 64 -> 32 at bench batch, ragged tiles
    (2, 32, 16, 16, 16, 1, 1, 0, 0, None, None, None, False, False),    # one output tile, no bias
    (2, 32, 16, 16, 72, 1, 1, 0, 0, None, None, "relu", True, True),      # second co chunk holds 8 channels: one lane half idle
    # the "shifted dy" bf16x3 weight-gradient kernel (32 output channels per workgroup, full tap grids, W % 4 == 0)
    (6, 32, 64, 64, 32, 3, 3, 1, 1, None, None, "gelu", False, True),   # VD-VAE 64x64: one row per tile
    (4, 64, 64, 64, 64, 3, 3, 1, 1, None, None, "relu", False, True),   # 64 -> 64 on 64-wide rows: x copies overflow LDS
    (5, 32, 32, 32, 32, 2, 2, 1, 1, "hw", None, "elu", False, True),    # 2 x 2 grid, column shifts {-1, 0}
    (3, 32, 12, 12, 32, 3, 3, 1, 1, None, "B", None, False, True),      # W = 12: two pixel blocks, the second half full
    (3, 32, 10, 20, 32, 1, 3, 0, 1, None, None, "relu", False, False),  # 1 x 3 grid, W = 20, no bias
    (3, 32, 9, 16, 96, 2, 1, 2, 0, "hw", None, None, False, True),      # 2 x 1 grid, three co chunks
    (3, 64, 8, 24, 32, 2, 3, 1, 1, "hw", None, "gelu", True, True),     # 2 x 3 grid, two ci chunks: on 24-wide rows neither bf16x3 kernel's tile fits LDS, the generic fp32 kernel runs
    # half pixel blocks (W % 8 == 4) on the x-copy bf16x3 weight-gradient kernel (64 output channels)
    (40, 32, 28, 28, 64, 1, 1, 0, 0, None, None, "relu", False, True),  # PixelCNN's 1x1 32 -> 64
    (3, 32, 12, 12, 64, 2, 2, 1, 1, "hw", None, "elu", False, True),    # 2x2, two blocks per row
    (3, 64, 20, 20, 128, 1, 3, 0, 1, None, None, None, True, True),     # 1x3, W = 20: three x copies do not fit LDS, the shifted-dy kernel runs
    # big tiles of the bf16x3 weight gradient (round 5: at most 2 taps, Cin % 64 == 0 -> 64 x channels per workgroup;
    # one tap with Cout % 128 == 0 -> 128 x 64 channels). Since round 6 the 32-wide rows among them run on the row-ring kernel.
    (10, 128, 32, 32, 256, 1, 1, 0, 0, None, None, None, False, True),   # GatedPixelCNN's 1x1 128 -> 256: the ring's 128 x 128 one-tap tile
    (6, 64, 28, 28, 128, 1, 1, 0, 0, None, None, "relu", False, True),   # 128 x 64, half pixel blocks (W = 28)
    (3, 64, 12, 16, 64, 2, 1, 2, 0, "hw", None, "elu", False, True),     # 64 x 64, two taps (row shift)
    (5, 128, 32, 32, 256, 2, 1, 2, 0, "hw", None, None, False, True),    # GatedPixelCNN's 2x1 128 -> 256 (ring, 128 x 64 tile)
    (3, 128, 10, 32, 128, 1, 2, 0, 1, "hw", None, None, True, False),    # 1x2: two column copies, no bias (ring, 128 x 64 tile, 10-row images: no segments)
    (2, 192, 8, 8, 128, 1, 1, 0, 0, None, None, "gelu", False, True),    # 8-wide rows: TR = 8, three ci chunks
    # 4 taps where the GENERIC planner arrives at the pipelined kernel's chunk shape (Cin % 16 != 0, two output chunks):
    # stays on conv_b3_kernel (B3Plan::pipelined is set by the PG_CONV_B3P branch only); the data gradient (K = 128,
    # M = 24 -> two co tiles) takes the generic plan as well
    (3, 24, 32, 32, 128, 2, 2, 1, 1, "hw", None, "elu", True, True),
    (3, 40, 16, 32, 64, 2, 2, 1, 1, "hw", None, None, False, True),     # pipelined forward with Cin = 40: five 8-channel chunks
    (3, 64, 32, 32, 56, 2, 2, 1, 1, "hw", None, "elu", False, True),    # pipelined kernel, partial output chunk (56 of 64)
    # round 5: odd numbers of output chunks (PixelCNN++'s widths; the wide kernel for them was measured and dropped: 684 -> 642 images/s)
    (3, 64, 16, 16, 160, 2, 3, 1, 1, "hw", None, "elu", True, True),     # forward: 3 chunks (64 + 64 + 32 channels)
    (2, 320, 16, 16, 64, 1, 3, 0, 1, None, None, "relu", False, True),   # data gradient: M = 320 = 5 chunks
    (70, 64, 32, 32, 320, 2, 3, 1, 1, "hw", None, None, True, False),    # 5 chunks, several tiles per workgroup, no bias
    # round 5: images below 256 pixels on the bf16x3 kernels (one image = a partial tile)
    (9, 64, 8, 8, 64, 2, 3, 1, 1, "hw", None, "elu", True, True),       # 8 x 8, six taps
    (530, 32, 8, 8, 32, 3, 3, 1, 1, None, None, "gelu", False, True),   # VD-VAE's 8 x 8 level: more images than workgroups
    (33, 32, 4, 4, 64, 3, 3, 1, 1, None, None, "relu", True, True),     # 4 x 4 images: 16 of a tile's 256 pixels
    (12, 320, 8, 8, 160, 2, 2, 1, 1, "hw", None, None, False, True),    # PixelCNN++'s coarsest level, pipelined 4-tap kernel
    (5, 128, 8, 8, 256, 1, 1, 0, 0, None, None, "relu", True, True),    # 1x1 on 64-pixel images (wide kernel)
    # round 5: the pipelined kernel with several output chunks when the wide kernel does not apply (Cout % 128 != 0)
    (3, 64, 32, 32, 160, 2, 2, 1, 1, "hw", None, "elu", True, True),    # PixelCNN++'s widths: chunks of 64 + 64 + 32
    (70, 320, 16, 16, 320, 2, 2, 1, 1, "hw", None, None, False, True),  # 320 -> 320 on 16 x 16, several tiles per workgroup
]


def _active(kind, kh, kw):
    if kind is None:
        return None
    m = oops.causal_mask(kh, kw, kind == "A")
    return [(u, v) for u in range(kh) for v in range(kw) if m[u, v] != 0]


@pytest.mark.parametrize("case", CONV_CASES, ids=lambda c: "x".join(str(v) for v in c[:9]))
def test_conv_fwd_dgrad_wgrad(dev, case):
    from pytorch_generative_amd import ops

    n, cin, h, w, cout, kh, kw, ph, pw, crop, active, in_act, use_res, use_bias = case
    x = _rand(n, cin, h, w, seed=1)
    wt = _rand(cout, cin, kh, kw, seed=2, scale=0.2)
    b = _rand(cout, seed=3) if use_bias else None
    act_fn = {None: lambda t: t, "relu": F.relu, "elu": F.elu, "gelu": F.gelu}[in_act]
    taps = _active(active, kh, kw)
    mask = torch.ones(kh, kw) if taps is None else oops.causal_mask(kh, kw, active == "A")
    spec = ops.ConvSpec(kh, kw, ph, pw, active=taps, wgrad_all=True)
    oh, ow = (h, w) if crop == "hw" else spec.full_out(h, w)
    res = _rand(n, cout, oh, ow, seed=4) if use_res else None

    # oracle (reference semantics: weight already masked in place -> full wgrad)
    xo = x.clone().requires_grad_(True)
    wo = (wt * mask).clone().requires_grad_(True)
    bo = b.clone().requires_grad_(True) if use_bias else None
    yo = F.conv2d(act_fn(xo), wo, bo, padding=(ph, pw))[:, :, :oh, :ow]
    if use_res:
        yo = yo + res
    dy = _rand(*yo.shape, seed=5)
    yo.backward(dy)

    xg = x.to(dev).requires_grad_(True)
    wg = (wt * mask).to(dev).requires_grad_(True)
    bg = b.to(dev).requires_grad_(True) if use_bias else None
    yg = ops.conv2d_taps(xg, wg, bg, spec, out_hw=(oh, ow),
                         in_act=ops._ACT_IDS[in_act], res=None if res is None else res.to(dev))
    _util.assert_close(yg, yo, TOL, "conv fwd")
    yg.backward(dy.to(dev))
    _util.assert_close(xg.grad, xo.grad, TOL, "conv dgrad")
    _util.assert_close(wg.grad, wo.grad, TOL, "conv wgrad")
    if use_bias:
        _util.assert_close(bg.grad, bo.grad, TOL, "conv bgrad")


def _random_conv_case(seed):
    import random

    r = random.Random(seed)
    kh, kw, ph, pw, crop = r.choice([(1, 1, 0, 0, None), (1, 1, 0, 0, None), (3, 3, 1, 1, None), (2, 2, 1, 1, "hw"),
                                     (1, 3, 0, 1, None), (2, 1, 2, 0, "hw"), (2, 3, 1, 1, "hw")])
    cin = r.choice([16, 24, 32, 40, 48, 64, 96, 128])
    cout = r.choice([16, 24, 32, 36, 48, 64, 96, 128])
    h = r.choice([6, 10, 12, 16, 18, 20, 28, 32, 36])
    w = r.choice([8, 12, 16, 20, 24, 28, 32, 36, 64])
    n = r.choice([1, 2, 3, 5, 9])
    in_act = r.choice([None, "relu", "elu", "gelu"])
    active = "B" if (kh, kw) == (3, 3) and r.random() < 0.3 else None
    return (n, cin, h, w, cout, kh, kw, ph, pw, crop, active, in_act, r.random() < 0.5, r.random() < 0.8)


# Round 3 kept the next two tests opt-in: with them in the full `pytest tests -m gpu` sequence the process had died twice
# later on (a GPU memory fault in the reference suite's GatedPixelCNN reproduce test). Round 4 (profiles/README.md, round 4,
# item 1): the sequence with them ran green in every one of this round's runs, on the default allocator and under the
# canary allocator of tests/guard/ (every tensor its own allocation between NaN-filled margins: no out-of-bounds write,
# no read of never-written memory anywhere in the tier) — they are part of the default tier again.
@pytest.mark.parametrize("seed", range(32))
def test_conv_random_shapes(dev, seed):
    """Seeded random shapes through whatever kernel the dispatch picks (1x1 barrier-free, staged, 9-slot, fp32-MFMA,
    VALU; x-copy / shifted-dy / fp32 weight gradients): forward, data gradient, weight and bias gradient."""
    test_conv_fwd_dgrad_wgrad(dev, _random_conv_case(1000 + seed))


def _family_cases():
    import _conv_b3_routes as R

    return R.FAMILY_CASES


@pytest.mark.parametrize("what,case,want", _family_cases(), ids=[c[0] for c in _family_cases()])
def test_conv_b3_kernel_families(dev, what, case, want):
    """One small convolution per bf16x3 kernel family (staged narrow / wide, 1x1, pipelined, overlapped): pg_conv_b3_route says the
    forward launch lands on the named instantiation, then forward and data gradient against the oracle as in
    test_conv_fwd_dgrad_wgrad."""
    import _conv_b3_routes as R
    from pytorch_generative_amd import _lib

    rc, r = R.route(_lib.load(), R.family_problem(case))
    got = R.named(r)
    assert rc == 0 and {k: got[k] for k in want} == want, (what, got)
    test_conv_fwd_dgrad_wgrad(dev, case)


SKIP_CASES = [
    # (N, C, H, W, Cmid, k, in_act): x -> conv1 (k x k, C -> Cmid, n_skip = 2) -> conv2 (1x1, Cmid -> C, res, res2)
    (3, 64, 28, 28, 32, 1, "relu"),   # PixelCNN's block: barrier-free 1x1 kernel, multi-stream epilogues both ways
    (3, 64, 16, 16, 64, 2, "elu"),    # staged kernel with the multi-stream epilogue (2x2 taps)
    (2, 128, 16, 20, 64, 1, None),    # 128 channels: data gradient on the staged kernel
    (3, 64, 32, 32, 32, 3, "gelu"),   # 3x3 data gradient with 64 output channels: 9-weight-slot plan + GELU derivative
    (3, 32, 16, 16, 32, 1, "relu"),   # < 64 channels: the add fallback
    (4, 64, 8, 8, 32, 3, "relu"),     # < 256 pixels per image: fp32-MFMA kernels, add fallback
]


@pytest.mark.parametrize("case", SKIP_CASES, ids=lambda c: "x".join(str(v) for v in c))
def test_conv_skip_aliases_and_two_residuals(dev, case):
    """y, x1, x2 = conv1(x, n_skip=2); z = conv2(y, res=x1, res2=x2) against conv2(conv1(act(x))) + 2 x: the
    pass-through aliases (skip gradients added in conv1's data-gradient epilogue) and the two-residual epilogue."""
    from pytorch_generative_amd import nn as pg_nn

    n, c, h, w, cmid, k, in_act = case
    torch.manual_seed(0)
    pad = 1 if k > 1 else 0
    conv1 = pg_nn.Conv2d(c, cmid, k, padding=pad)
    conv2 = pg_nn.Conv2d(cmid, c, 1)
    x = _rand(n, c, h, w, seed=1)
    g = _rand(n, c, h, w, seed=2)
    act_fn = {None: lambda t: t, "relu": F.relu, "elu": F.elu, "gelu": F.gelu}[in_act]
    # oracle
    xo = x.clone().requires_grad_(True)
    w1, b1 = conv1.weight.detach().clone().requires_grad_(True), conv1.bias.detach().clone().requires_grad_(True)
    w2, b2 = conv2.weight.detach().clone().requires_grad_(True), conv2.bias.detach().clone().requires_grad_(True)
    yo = F.conv2d(act_fn(xo), w1, b1, padding=pad)[:, :, :h, :w]
    zo = F.conv2d(yo, w2, b2) + xo + xo
    zo.backward(g)
    # HIP path
    conv1, conv2 = conv1.to(dev), conv2.to(dev)
    xg = x.to(dev).requires_grad_(True)
    y, x1, x2 = conv1(xg, crop=(h, w), in_act=in_act, n_skip=2)
    z = conv2(y, res=x1, res2=x2)
    _util.assert_close(z, zo, TOL, "fwd")
    z.backward(g.to(dev))
    _util.assert_close(xg.grad, xo.grad, TOL, "dx")
    _util.assert_close(conv1.weight.grad, w1.grad, TOL, "dw1")
    _util.assert_close(conv1.bias.grad, b1.grad, TOL, "db1")
    _util.assert_close(conv2.weight.grad, w2.grad, TOL, "dw2")
    _util.assert_close(conv2.bias.grad, b2.grad, TOL, "db2")


def test_conv_weight_grad_sink_accumulates(dev):
    """With a `_pg_grad` sink the wgrad kernel accumulates into it and autograd sees None."""
    from pytorch_generative_amd import nn as pg_nn

    torch.manual_seed(0)
    conv = pg_nn.Conv2d(8, 8, kernel_size=1).to(dev)
    x = _rand(2, 8, 8, 8, seed=1).to(dev)
    conv(x).sum().backward()
    g_ref = conv.weight.grad.clone()
    conv.weight.grad = None
    conv.weight._pg_grad = torch.ones_like(conv.weight)
    conv.bias._pg_grad = torch.zeros_like(conv.bias)
    conv(x).sum().backward()
    assert conv.weight.grad is None
    _util.assert_close(conv.weight._pg_grad - 1.0, g_ref, TOL, "sink")


@pytest.mark.parametrize("n,c,h,w", [(3, 16, 28, 28), (2, 8, 7, 7), (2, 64, 9, 9), (1, 70, 5, 5)])
def test_nchw_layernorm(dev, n, c, h, w):
    from pytorch_generative_amd import ops

    x = _rand(n, c, h, w, seed=1, scale=3.0) + 0.5
    gam, bet = _rand(c, seed=2) + 1.0, _rand(c, seed=3)
    dy = _rand(n, c, h, w, seed=4)
    xo, go, bo = (t.clone().requires_grad_(True) for t in (x, gam, bet))
    yo = oops.nchw_layernorm(xo, go, bo)
    yo.backward(dy)
    xg, gg, bg = (t.to(dev).requires_grad_(True) for t in (x, gam, bet))
    yg = ops.nchw_layernorm(xg, gg, bg, 1e-5)
    assert yg.is_contiguous()
    _util.assert_close(yg, yo, TOL, "ln fwd")
    yg.backward(dy.to(dev))
    _util.assert_close(xg.grad, xo.grad, TOL, "ln dx")
    _util.assert_close(gg.grad, go.grad, TOL, "ln dgamma")
    _util.assert_close(bg.grad, bo.grad, TOL, "ln dbeta")


ATTN_CASES = [
    # (N, heads, dk, dv, H, W, strict)
    (2, 4, 4, 4, 28, 28, False),   # ImageGPT baseline block
    (2, 1, 4, 32, 32, 32, True),   # PixelSNAIL block
    (2, 2, 32, 32, 12, 12, False),  # ImageGPT reproduce() head dims (2 heads x 32): matrix-core path since round 3
    (2, 2, 32, 32, 28, 28, False),  # ... at the reproduce() image size, L = 784 (49 query groups: ragged last block)
    (1, 1, 32, 32, 20, 20, True),   # ... strict mask, L = 400
    (2, 2, 2, 2, 7, 7, False),     # reference MultipleChannelsTests (L=49, ragged chunks)
    (1, 1, 4, 4, 5, 5, True),      # matrix-core path (d_k = d_v = 4), L < 64, strict, L % 8 != 0
    (2, 3, 8, 16, 9, 7, True),     # odd everything: VALU row-owner kernels, L = 63
    (1, 2, 48, 40, 8, 8, False),   # head dims zero-padded to 64 / 64 (attention_k4.hip)
    (1, 1, 4, 4, 18, 18, True),    # matrix-core path, L = 324: six query blocks, the short one first
    (3, 2, 4, 4, 28, 28, True),    # matrix-core path (d_k = d_v = 4), strict mask
    (1, 3, 4, 4, 7, 9, False),     # matrix-core path, L = 63: scalar staging, ragged last group
    (1, 1, 4, 4, 32, 32, False),   # matrix-core path, L = 1024: 16 blocks = 8 waves
    (1, 2, 4, 4, 36, 36, True),    # matrix-core path, L = 1296: 21 blocks on the 8 waves of ONE workgroup per (n, head)
    # round 4: head dims beyond (4, <= 32) / (<= 16, <= 16) on the matrix-core kernels of attention_k4.hip
    # (instantiated for d_k in {4, 16, 32, 64} x d_v in {16, 32, 64}), other sizes zero-padded by ops.causal_attention
    (2, 1, 64, 64, 16, 16, False),  # 64 / 64: 16-row blocks
    (1, 2, 64, 64, 12, 12, True),   # ... strict, L = 144
    (2, 1, 16, 64, 16, 16, True),   # 16 / 64
    (2, 2, 4, 64, 16, 16, False),   # 4 / 64: VALU dQ / dK accumulation with 64 value channels
    (1, 2, 64, 16, 16, 12, False),  # 64 / 16, L = 192
    (2, 1, 64, 4, 8, 8, True),      # 64 / 4: value channels padded to 16
    (2, 2, 16, 32, 16, 16, False),  # 16 / 32
    (1, 2, 32, 16, 20, 20, True),   # 32 / 16, L = 400
    (2, 1, 32, 64, 8, 8, False),    # 32 / 64
    (2, 2, 16, 32, 7, 7, False),    # L = 49 padded to 64
    (1, 1, 24, 40, 9, 5, True),     # 24 / 40 at L = 45: every dimension padded (32 / 64, L = 48)
    (1, 2, 8, 20, 16, 16, False),   # d_k = 8 padded to 16, d_v = 20 to 32
]


ALLOWED_SET_CASES = [
    # (heads, dk, dv, H, W, strict)
    (4, 4, 4, 28, 28, False),   # ImageGPT (BASELINE configs[1]): attention_mfma.hip, L = 784
    (4, 4, 4, 28, 28, True),
    (1, 4, 32, 32, 32, True),   # PixelSNAIL (configs[3]): attention_k4.hip, L = 1024, strict
    (1, 4, 32, 32, 32, False),
    (2, 32, 32, 28, 28, False),  # ImageGPT reproduce() head dims, ragged last 32-row block
    (1, 4, 4, 36, 36, True),    # attention_mfma.hip, L = 1296: 21 blocks on the 8 waves of one workgroup
    (2, 2, 2, 7, 7, False),     # VALU row-owner kernels, L = 49
]


@pytest.mark.parametrize("deterministic", [False, True], ids=["fused-bwd", "two-kernel-bwd"])
@pytest.mark.parametrize("case", ALLOWED_SET_CASES, ids=lambda c: "-".join(str(int(v)) for v in c))
def test_attention_allowed_set_is_bit_exact(dev, case, deterministic):
    """north_star: "bit-exact for the causal mask indices". No L x L mask exists on the HIP path, so the set of (query, key)
    pairs the kernels admit is read back FROM the kernels and compared with `_get_causal_mask`
    (reference nn/attention.py:60-63 = oracle.ops.attention_mask) by torch.equal:
      * q = k = 0 makes every admitted score 0, so P[l, m] = 1 / count(l) on admitted pairs and 0 elsewhere;
      * V one-hot over key positions (image n, channel j marks key n * d_v + j) turns the forward output into
        O[n, j, l] = P[l, n * d_v + j]: non-zero exactly on the forward kernels' admitted set;
      * dO one-hot over QUERY positions turns dV into dV[n, j, m] = P[n * d_v + j, m]: the backward kernels' admitted set
        (fused backward, and the two-kernel backward under ops.set_deterministic).
    The recovered values are also checked: P * count == 1 to fp32 rounding, the strict mask's empty row is exactly zero."""
    from pytorch_generative_amd import ops

    heads, dk, dv, h, w, strict = case
    L, e, v = h * w, heads * dk, heads * dv
    n = -(-L // dv)
    pos = torch.arange(n * dv).reshape(n, 1, dv, 1)                                     # position marked by (image, channel)
    onehot = (pos == torch.arange(L).reshape(1, 1, 1, L)).float().expand(n, heads, dv, L)  # every head sees the same marks
    onehot = onehot.reshape(n, v, h, w).contiguous()
    q = torch.zeros(n, e, h, w, device=dev)
    kv = torch.cat([torch.zeros(n, e, h, w), onehot], dim=1).to(dev).requires_grad_(True)
    want = oops.attention_mask(L, strict)                                               # [query l, key m]
    was = ops.set_deterministic(deterministic)
    try:
        o = ops.causal_attention(q, kv, heads, e, v, strict)
        o.backward(onehot.to(dev))
    finally:
        ops.set_deterministic(was)
    count = want.sum(1)
    for hd in range(heads):
        # forward: P[l, m] = O[n(m), hd * dv + j(m), l]
        p_fwd = o.detach().cpu().reshape(n, heads, dv, L)[:, hd].reshape(n * dv, L)[:L].t().contiguous()
        assert torch.equal((p_fwd != 0).float(), want), f"forward allowed set, head {hd}"
        assert float((p_fwd * count[:, None] - want).abs().max()) <= 5e-6, "forward P * count != 1"
        # backward: P[l, m] = dV[n(l), hd * dv + j(l), m]
        p_bwd = kv.grad[:, e:].cpu().reshape(n, heads, dv, L)[:, hd].reshape(n * dv, L)[:L].contiguous()
        assert torch.equal((p_bwd != 0).float(), want), f"backward allowed set, head {hd}"
        assert float((p_bwd * count[:, None] - want).abs().max()) <= 5e-6, "backward P * count != 1"
    if strict:
        assert float(o[:, :, 0, 0].abs().max()) == 0.0
    assert float(kv.grad[:, :e].abs().max()) == 0.0  # dK = dS^T q with q = 0


@pytest.mark.parametrize("case", ATTN_CASES, ids=lambda c: "-".join(str(int(v)) for v in c))
def test_causal_attention_core(dev, case):
    from pytorch_generative_amd import ops

    n, heads, dk, dv, h, w, strict = case
    e, v = heads * dk, heads * dv
    q = _rand(n, e, h, w, seed=1)
    kv = _rand(n, e + v, h, w, seed=2)
    d_o = _rand(n, v, h, w, seed=3)
    qo, kvo = q.clone().requires_grad_(True), kv.clone().requires_grad_(True)
    oo = oops.causal_attention_core(qo, kvo[:, :e], kvo[:, e:], heads, strict)
    oo.backward(d_o)
    qg, kvg = q.to(dev).requires_grad_(True), kv.to(dev).requires_grad_(True)
    og = ops.causal_attention(qg, kvg, heads, e, v, strict)
    _util.assert_close(og, oo, TOL, "attn fwd")
    if strict:  # the row with no allowed key is exactly zero (reference: NaN -> masked_fill 0)
        assert torch.equal(og[:, :, 0, 0].cpu(), torch.zeros(n, v))
    og.backward(d_o.to(dev))
    _util.assert_close(qg.grad, qo.grad, TOL, "attn dq")
    _util.assert_close(kvg.grad[:, :e], kvo.grad[:, :e], TOL, "attn dk")
    _util.assert_close(kvg.grad[:, e:], kvo.grad[:, e:], TOL, "attn dv")


@pytest.mark.parametrize("case", [(3, 2, 28, 28, True), (1, 3, 7, 9, False), (1, 1, 32, 32, False),
                                  (1, 2, 36, 36, True), (40, 4, 28, 28, False)],
                         ids=lambda c: "-".join(str(int(v)) for v in c))
@pytest.mark.parametrize("fused", [True, False], ids=["fused_bwd", "two_kernel_bwd"])
def test_attention_m44_backward_paths(dev, case, fused):
    """d_k = d_v = 4: the fused backward (dQ, dK, dV in one pass, attn_bwd_m44_kernel) and the two-kernel
    backward (ops.set_deterministic) against the oracle; the batch-40 case has several workgroups per
    CU and every wave of a workgroup depositing into the same dQ planes."""
    from pytorch_generative_amd import ops

    n, heads, h, w, strict = case
    e = v = heads * 4
    q, kv, d_o = _rand(n, e, h, w, seed=1), _rand(n, e + v, h, w, seed=2), _rand(n, v, h, w, seed=3)
    qo, kvo = q.clone().requires_grad_(True), kv.clone().requires_grad_(True)
    oops.causal_attention_core(qo, kvo[:, :e], kvo[:, e:], heads, strict).backward(d_o)
    was = ops.set_deterministic(not fused)
    try:
        qg, kvg = q.to(dev).requires_grad_(True), kv.to(dev).requires_grad_(True)
        ops.causal_attention(qg, kvg, heads, e, v, strict).backward(d_o.to(dev))
        torch.cuda.synchronize()
    finally:
        ops.set_deterministic(was)
    _util.assert_close(qg.grad, qo.grad, TOL, "attn dq")
    _util.assert_close(kvg.grad[:, :e], kvo.grad[:, :e], TOL, "attn dk")
    _util.assert_close(kvg.grad[:, e:], kvo.grad[:, e:], TOL, "attn dv")


@pytest.mark.parametrize("case", [(2, 1, 4, 32, 32, 32, True), (3, 2, 4, 16, 16, 16, False), (1, 1, 4, 32, 20, 20, True),
                                  (70, 1, 4, 32, 16, 16, True)],
                         ids=lambda c: "-".join(str(int(v)) for v in c))
@pytest.mark.parametrize("fused", [True, False], ids=["fused_bwd", "two_kernel_bwd"])
def test_attention_k4_backward_paths(dev, case, fused):
    """d_k = 4, d_v = 16 / 32 (PixelSNAIL): the fused backward (attn_delta_k4_kernel + attn_bwd_k4_kernel: dQ through a
    transposed dS tile and fp32 atomics, dK / dV in registers; round 4) and the two-kernel backward against the oracle
    — L = 400 ends in a ragged 32-key block, 70 units span two groups of 64."""
    from pytorch_generative_amd import ops

    n, heads, dk, dv, h, w, strict = case
    e, v = heads * dk, heads * dv
    q = _rand(n, e, h, w, seed=1)
    kv = _rand(n, e + v, h, w, seed=2)
    d_o = _rand(n, v, h, w, seed=3)
    qo, kvo = q.clone().requires_grad_(True), kv.clone().requires_grad_(True)
    oops.causal_attention_core(qo, kvo[:, :e], kvo[:, e:], heads, strict).backward(d_o)
    was = ops.set_deterministic(not fused)
    try:
        qg, kvg = q.to(dev).requires_grad_(True), kv.to(dev).requires_grad_(True)
        ops.causal_attention(qg, kvg, heads, e, v, strict).backward(d_o.to(dev))
        torch.cuda.synchronize()
    finally:
        ops.set_deterministic(was)
    _util.assert_close(qg.grad, qo.grad, TOL, "attn dq")
    _util.assert_close(kvg.grad[:, :e], kvo.grad[:, :e], TOL, "attn dk")
    _util.assert_close(kvg.grad[:, e:], kvo.grad[:, e:], TOL, "attn dv")


@pytest.mark.parametrize("case", [(1, 1, 4, 32, 28, 28), (3, 2, 4, 16, 16, 16)], ids=["snail28", "two_heads"])
def test_attention_backward_replayed_graph_equals_eager(dev, case):
    """A captured forward + fused backward replayed SEVERAL times returns the eager gradients every time. (Round 4,
    found under the canary allocator: dQ used to be zeroed by a hipMemset2DAsync node, which wrote zeros on the first
    launch of the executable graph and a stale value afterwards; the delta pre-pass zeroes dQ now. One replay — what
    the older graph tests looked at — cannot see that.)"""
    from pytorch_generative_amd import ops

    n, heads, dk, dv, h, w = case
    e, v = heads * dk, heads * dv
    qkv0 = _rand(n, 2 * e + v, h, w, seed=4).to(dev)
    d_o = _rand(n, v, h, w, seed=5).to(dev)

    def run(t):
        o = ops.causal_attention_qkv(t, heads, e, v, True)
        (g,) = torch.autograd.grad(o, t, d_o)
        return o.detach(), g

    o_e, g_e = run(qkv0.clone().requires_grad_(True))
    static = qkv0.clone().requires_grad_(True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run(static)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr, capture_error_mode="thread_local"):
        o_g, g_g = run(static)
    for it in range(4):
        gr.replay()
        torch.cuda.synchronize()
        assert torch.equal(o_g, o_e), f"replay {it}: output"
        assert torch.equal(g_g[:, e:], g_e[:, e:]), f"replay {it}: dK / dV"
        # dQ: fp32 atomics, arrival order may differ between launches
        _util.assert_close(g_g[:, :e], g_e[:, :e], 1e-5, f"replay {it}: dQ")


def test_attention_large_scores_stay_finite(dev):
    """Online-softmax rescale branch: a spike late in the key sequence forces the running max to
    jump; compare with the oracle on the same data."""
    from pytorch_generative_amd import ops

    q = _rand(1, 4, 16, 16, seed=1)
    kv = _rand(1, 8, 16, 16, seed=2)
    kv[0, :4, 9, 3] = 40.0   # one huge key
    q[0, :, 12, 0] = 30.0    # one query that loves it
    oo = oops.causal_attention_core(q, kv[:, :4], kv[:, 4:], 1, False)
    og = ops.causal_attention(q.to(dev), kv.to(dev), 1, 4, 4, False)
    assert torch.isfinite(og).all()
    _util.assert_close(og, oo, TOL, "attn spike")


def test_attention_uniform_values_property(dev):
    """Full size property (L=1024, N=8): with V constant over positions the output equals V for
    every query that has at least one allowed key, whatever q/k are."""
    from pytorch_generative_amd import ops

    n, e, v, h, w = 8, 4, 32, 32, 32
    q = _rand(n, e, h, w, seed=1, scale=3.0).to(dev)
    kv = _rand(n, e + v, h, w, seed=2, scale=3.0).to(dev)
    const = _rand(n, v, 1, 1, seed=3).to(dev)
    kv[:, e:] = const
    out = ops.causal_attention(q, kv, 1, e, v, True)
    want = const.expand(n, v, h, w).clone()
    want[:, :, 0, 0] = 0
    assert float((out - want).abs().max()) < 1e-5


@pytest.mark.parametrize("act", ["relu", "elu", "gelu"])
def test_activations(dev, act):
    from pytorch_generative_amd import ops

    fn = {"relu": F.relu, "elu": F.elu, "gelu": F.gelu}[act]
    x = _rand(3, 5, 7, 9, seed=1, scale=2.0)
    dy = _rand(3, 5, 7, 9, seed=2)
    xo = x.clone().requires_grad_(True)
    yo = fn(xo)
    yo.backward(dy)
    xg = x.to(dev).requires_grad_(True)
    yg = getattr(ops, act)(xg)
    _util.assert_close(yg, yo, 1e-5, act)
    yg.backward(dy.to(dev))
    _util.assert_close(xg.grad, xo.grad, 1e-5, act + " grad")


@pytest.mark.parametrize("kind", ["tanh", "identity"])
def test_gated_activation(dev, kind):
    from pytorch_generative_amd import ops

    x = _rand(2, 12, 6, 5, seed=1)
    dy = _rand(2, 6, 6, 5, seed=2)
    xo = x.clone().requires_grad_(True)
    yo = oops.gated_activation(xo, kind)
    yo.backward(dy)
    xg = x.to(dev).requires_grad_(True)
    yg = ops.gated_activation(xg, ops.GATE_TANH if kind == "tanh" else ops.GATE_IDENTITY)
    _util.assert_close(yg, yo, 1e-5, "gate")
    yg.backward(dy.to(dev))
    _util.assert_close(xg.grad, xo.grad, 1e-5, "gate grad")


GATED_CONV_CASES = [
    # (N, Cin, H, W, Cout, k, pad, mask_center, kind, in_act, use_res)
    (3, 64, 32, 32, 64, 2, 1, None, "identity", "elu", True),    # PixelSNAIL ResidualBlock (pixel_snail.py:41-56)
    (2, 128, 16, 16, 128, 3, 1, False, "tanh", None, False),     # GatedPixelCNN-style masked stack (type B)
    (2, 16, 12, 12, 8, 3, 1, True, "tanh", None, False),         # type A, narrow: fp32-MFMA / VALU kernels
    (2, 64, 28, 28, 32, 1, 0, None, "tanh", "relu", True),       # 1x1
    # round 6: 128 output channels on the wide kernel = the gate (and res) in the convolution's epilogue (Conv2d.gate_ok)
    (1, 64, 28, 28, 64, 2, 1, None, "identity", "elu", False),   # batch 1, no residual, 28 wide (ragged pixel tiles)
    (5, 32, 12, 12, 64, 3, 1, False, "tanh", None, True),        # masked type B: 5 taps, tanh gate, several images per tile
    (2, 128, 9, 11, 64, 3, 1, True, "tanh", "relu", True),       # type A: 4 taps, odd sizes
]
FUSED_GATE_CASES = {0, 1, 4, 5, 6}  # indices of GATED_CONV_CASES the fused epilogue must take (asserted: a routing change is a finding)


@pytest.mark.parametrize("case", GATED_CONV_CASES, ids=lambda c: "x".join(str(v) for v in c))
def test_gated_conv(dev, case):
    """nn.GatedConv (north_star's operator name) = convolution to 2 Cout channels + GatedActivation (+ residual)
    against the same composition in torch on the CPU: output, dx, dweight, dbias."""
    from torch import nn as tnn

    from pytorch_generative_amd import nn as pg_nn

    n, cin, h, w, cout, k, pad, mc, kind, in_act, use_res = case
    torch.manual_seed(0)
    fn = torch.tanh if kind == "tanh" else tnn.Identity()
    m = pg_nn.GatedConv(cin, cout, k, padding=pad, mask_center=mc, activation_fn=fn)
    x, g = _rand(n, cin, h, w, seed=1), _rand(n, cout, h, w, seed=2)
    res = _rand(n, cout, h, w, seed=3) if use_res else None
    act_fn = {None: lambda t: t, "relu": F.relu, "elu": F.elu}[in_act]
    mask = m.conv.mask if mc is not None else torch.ones_like(m.conv.weight)
    xo = x.clone().requires_grad_(True)
    wo = (m.conv.weight.detach() * mask).clone().requires_grad_(True)
    bo = m.conv.bias.detach().clone().requires_grad_(True)
    yo = oops.gated_activation(F.conv2d(act_fn(xo), wo, bo, padding=pad)[:, :, :h, :w], kind)
    if use_res:
        yo = yo + res
    yo.backward(g)
    m = m.to(dev)
    xg = x.to(dev).requires_grad_(True)
    assert m.conv.gate_ok(xg, (h, w)) == (GATED_CONV_CASES.index(case) in FUSED_GATE_CASES)
    rg = None if res is None else res.to(dev).requires_grad_(True)
    yg = m(xg, crop=(h, w), in_act=in_act, res=rg)
    _util.assert_close(yg, yo, TOL, "gated conv")
    yg.backward(g.to(dev))
    _util.assert_close(xg.grad, xo.grad, TOL, "dx")
    _util.assert_close(m.conv.weight.grad, wo.grad, TOL, "dw")
    _util.assert_close(m.conv.bias.grad, bo.grad, TOL, "db")
    if rg is not None:
        assert torch.equal(rg.grad.cpu(), g), "the residual's gradient is dy itself"


@pytest.mark.parametrize("case", [GATED_CONV_CASES[i] for i in sorted(FUSED_GATE_CASES)],
                         ids=lambda c: "x".join(str(v) for v in c))
def test_gated_conv_fused_gate_equals_separate_kernels(dev, case, monkeypatch):
    """The gate in the convolution's epilogue against the same convolution followed by the standalone gate kernel (PG_FUSE_GATE=0):
    same accumulators, so output and every gradient agree to rounding of the sigmoid (1e-6), and the pre-gate tensor kept for
    backward is bit-identical to the unfused convolution's output."""
    from torch import nn as tnn

    from pytorch_generative_amd import nn as pg_nn
    from pytorch_generative_amd.ops import conv as ops_conv

    n, cin, h, w, cout, k, pad, mc, kind, in_act, use_res = case
    torch.manual_seed(0)
    fn = torch.tanh if kind == "tanh" else tnn.Identity()
    m = pg_nn.GatedConv(cin, cout, k, padding=pad, mask_center=mc, activation_fn=fn).to(dev)
    x, g = _rand(n, cin, h, w, seed=1).to(dev), _rand(n, cout, h, w, seed=2).to(dev)
    res = _rand(n, cout, h, w, seed=3).to(dev) if use_res else None
    got = {}
    for fused in (True, False):
        monkeypatch.setattr(ops_conv, "FUSE_GATE", fused)
        m.zero_grad(set_to_none=True)
        xg = x.clone().requires_grad_(True)
        assert m.conv.gate_ok(xg, (h, w)) == fused
        y = m(xg, crop=(h, w), in_act=in_act, res=res)
        y.backward(g)
        got[fused] = (y.detach(), xg.grad, m.conv.weight.grad.clone(), m.conv.bias.grad.clone())
    for a, b, what in zip(got[True], got[False], ("y", "dx", "dw", "db")):
        _util.assert_close(a, b.cpu(), 2e-6, what)


@pytest.mark.parametrize("case", [(2, 128, 32, 32, 128, 1, 1, 0, 0, 0), (3, 128, 32, 32, 128, 1, 2, 0, 1, 1), (1, 64, 12, 20, 64, 2, 2, 1, 1, 0)],
                         ids=["gated_vstack_1x1", "gated_hstack_1x2_alias", "ragged"])
def test_gate_behind_a_convolution_with_its_own_residual(dev, case, monkeypatch):
    """GatedPixelCNN's two gates (gated_pixel_cnn.py:63-96): gate(conv(x) + r) with r the link / vertical-stack sum, fused into the
    convolution's epilogue (2C = 256 channels: two pairs of gate-interleaved chunks) against torch on the CPU — y, dx, dr, dw, db, the
    pass-through alias of x — and against the unfused kernels."""
    from pytorch_generative_amd import nn as pg_nn
    from pytorch_generative_amd import ops
    from pytorch_generative_amd.ops import conv as ops_conv

    n, cin, h, w, c, kh, kw, ph, pw, n_skip = case
    torch.manual_seed(0)
    conv = pg_nn.Conv2d(cin, 2 * c, (kh, kw), padding=(ph, pw))
    x, r, g = _rand(n, cin, h, w, seed=1), _rand(n, 2 * c, h, w, seed=2), _rand(n, c, h, w, seed=3)
    g2 = _rand(n, cin, h, w, seed=4)
    xo, ro = x.clone().requires_grad_(True), r.clone().requires_grad_(True)
    wo, bo = conv.weight.detach().clone().requires_grad_(True), conv.bias.detach().clone().requires_grad_(True)
    z = F.conv2d(xo, wo, bo, padding=(ph, pw))[:, :, :h, :w] + ro
    yo = torch.tanh(z[:, :c]) * torch.sigmoid(z[:, c:])
    (yo * g).sum().backward() if not n_skip else ((yo * g).sum() + (xo * g2).sum()).backward()
    conv = conv.to(dev)
    got = {}
    for fused in (True, False):
        monkeypatch.setattr(ops_conv, "FUSE_GATE", fused)
        conv.zero_grad(set_to_none=True)
        xg, rg = x.to(dev).requires_grad_(True), r.to(dev).requires_grad_(True)
        assert conv.gate_ok(xg, (h, w)) == fused
        if fused:
            out = conv(xg, crop=(h, w), res=rg, n_skip=n_skip, gate=ops.GATE_TANH)
        else:
            out = conv(xg, crop=(h, w), res=rg, n_skip=n_skip)
            out = (ops.gated_activation(out[0], ops.GATE_TANH),) + tuple(out[1:]) if n_skip else ops.gated_activation(out, ops.GATE_TANH)
        y = out[0] if n_skip else out
        loss = (y * g.to(dev)).sum() + ((out[1] * g2.to(dev)).sum() if n_skip else 0.0)
        loss.backward()
        got[fused] = [y.detach(), xg.grad, rg.grad, conv.weight.grad.clone(), conv.bias.grad.clone()]
    for a, b, what in zip(got[True], [yo.detach(), xo.grad, ro.grad, wo.grad, bo.grad], ("y", "dx", "dr", "dw", "db")):
        _util.assert_close(a, b, TOL, what + " (fused vs torch)")
    for a, b, what in zip(got[True], got[False], ("y", "dx", "dr", "dw", "db")):
        _util.assert_close(a, b.cpu(), 5e-6, what + " (fused vs separate kernels)")


@pytest.mark.parametrize("n,c,ca,h,w", [(3, 64, 32, 32, 32), (2, 64, 32, 9, 10), (1, 64, 64, 4, 4)])
def test_dual_data_gradient_of_block_tail(dev, n, c, ca, h, w, monkeypatch):
    """PixelSNAIL's block tail (pixel_snail.py:109-119): r = elu(conv_r(elu(x1))), both = elu(conv_a(elu(x2))) + r,
    out = elu(conv_o(elu(both))) + x3 with the dual data gradient (ops.GradSlot: conv_o's epilogue writes both producers'
    gradients, they skip pg_act_bwd_from_out) against the same composition in torch on the CPU — output and every gradient —
    and against the unfused graph (PG_FUSE_DUAL=0) on the GPU."""
    from pytorch_generative_amd import nn as pg_nn
    from pytorch_generative_amd import ops
    from pytorch_generative_amd.ops import conv as ops_conv

    torch.manual_seed(0)
    conv_r, conv_a, conv_o = pg_nn.Conv2d(c, c, 1), pg_nn.Conv2d(ca, c, 1), pg_nn.Conv2d(c, c, 1)
    x1, x2, x3 = _rand(n, c, h, w, seed=1), _rand(n, ca, h, w, seed=2), _rand(n, c, h, w, seed=3)
    g = _rand(n, c, h, w, seed=4)
    ref_in = [t.clone().requires_grad_(True) for t in (x1, x2, x3)]
    ref_p = [p.detach().clone().requires_grad_(True) for m in (conv_r, conv_a, conv_o) for p in (m.weight, m.bias)]
    r = F.elu(F.conv2d(F.elu(ref_in[0]), ref_p[0], ref_p[1]))
    both = F.elu(F.conv2d(F.elu(ref_in[1]), ref_p[2], ref_p[3])) + r
    want = F.elu(F.conv2d(F.elu(both), ref_p[4], ref_p[5])) + ref_in[2]
    want.backward(g)
    mods = [m.to(dev) for m in (conv_r, conv_a, conv_o)]
    got = {}
    for fused in (True, False):
        monkeypatch.setattr(ops_conv, "FUSE_DUAL", fused)
        for m in mods:
            m.zero_grad(set_to_none=True)
        xs = [t.to(dev).requires_grad_(True) for t in (x1, x2, x3)]
        dual = mods[2].dual_ok(xs[0])
        assert dual == fused, "the 1x1 64 -> 64 data gradient is on the bf16x3 1x1 kernel: the dual epilogue must take it"
        r_g = mods[0](xs[0], in_act="elu", out_act="elu", out_pre_scaled=dual)
        if dual:
            slot = ops.GradSlot()
            both_g = mods[1](xs[1], in_act="elu", out_act="elu", res=r_g, out_pre_scaled=True, res_slot=slot)
            out = mods[2](both_g, in_act="elu", out_act="elu", res=xs[2], in_sum=(r_g, slot))
        else:
            both_g = mods[1](xs[1], in_act="elu", out_act="elu", res=r_g)
            out = mods[2](both_g, in_act="elu", out_act="elu", res=xs[2])
        out.backward(g.to(dev))
        got[fused] = [out.detach()] + [t.grad for t in xs] + [p.grad.clone() for m in mods for p in (m.weight, m.bias)]
    want_all = [want.detach()] + [t.grad for t in ref_in] + [p.grad for p in ref_p]
    names = ["out", "dx1", "dx2", "dx3", "dw_r", "db_r", "dw_a", "db_a", "dw_o", "db_o"]
    for a, b, what in zip(got[True], want_all, names):
        _util.assert_close(a, b, TOL, what + " (dual vs torch)")
    for a, b, what in zip(got[True], got[False], names):
        _util.assert_close(a, b.cpu(), 5e-6, what + " (dual vs separate kernels)")


def test_add_and_broadcast_add(dev):
    from pytorch_generative_amd import ops

    a, b = _rand(2, 3, 5, 7, seed=1), _rand(2, 3, 5, 7, seed=2)
    assert torch.equal(ops.add(a.to(dev), b.to(dev)).cpu(), a + b)
    p = _rand(1, 3, 5, 7, seed=3)
    dy = _rand(2, 3, 5, 7, seed=4)
    pg = p.to(dev).requires_grad_(True)
    y = ops.add_broadcast_batch(a.to(dev), pg)
    assert torch.equal(y.cpu(), a + p)
    y.backward(dy.to(dev))
    _util.assert_close(pg.grad, dy.sum(0, keepdim=True), 1e-6, "dpos")


_POSENC = _util.load_golden("posenc")


@pytest.mark.parametrize("shape", sorted(_POSENC["cases"]), ids=lambda s: "x".join(map(str, s)))
def test_positional_encoding_bit_exact(dev, shape):
    """Bit-exact against the planes the REAL reference produced (tests/golden/make_posenc_golden.py: `torch.arange` of the
    AVX-512 ATen build, whose rounding the kernel reproduces — elementwise.hip `arange_like_torch_cpu`). The oracle runs
    `torch.arange` on whatever host the GPU box has, so against IT one ulp is allowed; against the fixture nothing is."""
    from pytorch_generative_amd import nn as pg_nn

    got = pg_nn.image_positional_encoding(shape, dev).cpu()
    want = _POSENC["cases"][shape].expand(shape[0], -1, -1, -1)
    assert torch.equal(got, want)
    live = oops.image_positional_encoding(shape)
    assert float((got - live).abs().max()) <= 6e-8


def test_causal_mask_buffers_bit_exact_and_inplace_masking(dev):
    from pytorch_generative_amd import nn as pg_nn

    for k, mc in [(3, True), (3, False), (7, True), (5, False)]:
        conv = pg_nn.CausalConv2d(mc, 2, 3, kernel_size=k, padding=k // 2).to(dev)
        assert torch.equal(conv.mask[0, 0].cpu(), oops.causal_mask(k, k, mc))
        w0 = conv.weight.detach().clone()
        conv(torch.zeros(1, 2, 8, 8, device=dev))
        # reference side effect: weight.data *= mask on every forward (nn/convolution.py:42)
        assert torch.equal(conv.weight.detach(), w0 * conv.mask)


def test_bce_loss(dev):
    from pytorch_generative_amd import ops

    z = _rand(4, 1, 28, 28, seed=1, scale=3.0)
    x = torch.bernoulli(torch.full((4, 1, 28, 28), 0.13), generator=torch.Generator().manual_seed(2))
    zo = z.clone().requires_grad_(True)
    lo = oops.bce_sum_mean(zo, x)
    lo.backward()
    zg = z.to(dev).requires_grad_(True)
    lg = ops.bce_with_logits_sum_mean(zg, x.to(dev))
    _util.assert_close(lg, lo, 1e-5, "bce")
    lg.backward()
    _util.assert_close(zg.grad, zo.grad, 1e-5, "bce grad")


def test_layernorm_skip_folds_residual_gradient(dev):
    """y, xs = LN(x, skip): the gradient reaching xs is added inside the LN backward kernel."""
    from pytorch_generative_amd import ops

    x = _rand(2, 16, 9, 7, seed=1)
    g, b = _rand(16, seed=2) + 1.0, _rand(16, seed=3)
    dy, ds = _rand(2, 16, 9, 7, seed=4), _rand(2, 16, 9, 7, seed=5)
    xo, go, bo = (t.clone().requires_grad_(True) for t in (x, g, b))
    yo = oops.nchw_layernorm(xo, go, bo, 1e-5)
    (yo * dy).sum().backward()
    want_dx = xo.grad + ds
    xg, gg, bg = (t.to(dev).requires_grad_(True) for t in (x, g, b))
    yg, xs = ops.nchw_layernorm_skip(xg, gg, bg, 1e-5)
    ((yg * dy.to(dev)).sum() + (xs * ds.to(dev)).sum()).backward()
    _util.assert_close(yg, yo, TOL, "ln skip fwd")
    _util.assert_close(xg.grad, want_dx, TOL, "ln skip dx")
    _util.assert_close(gg.grad, go.grad, TOL, "ln skip dgamma")
    _util.assert_close(bg.grad, bo.grad, TOL, "ln skip dbeta")


def test_merged_qkv_projection_matches_separate_convs(dev):
    """With FlatAdam's adjacent layout CausalAttention runs q and kv as one convolution; outputs and
    every gradient equal the separate-convolution path."""
    from pytorch_generative_amd import nn as pg_nn, ops, optim

    torch.manual_seed(0)
    ref = pg_nn.CausalAttention(in_channels=16, n_heads=4, embed_channels=16, out_channels=16).to(dev)
    fused = pg_nn.CausalAttention(in_channels=16, n_heads=4, embed_channels=16, out_channels=16).to(dev)
    fused.load_state_dict(ref.state_dict())
    if not ops.FUSE_PAIR:
        pytest.skip("PG_FUSE_PAIR=0")
    opt = optim.FlatAdam(fused.parameters(), lr=1e-3)
    assert ops.conv_pair_views(fused._q, fused._kv) is not None
    assert ops.conv_pair_views(ref._q, ref._kv) is None
    x = _rand(2, 16, 12, 12, seed=7).to(dev)
    d_o = _rand(2, 16, 12, 12, seed=8).to(dev)
    xr, xf = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
    ref(xr).backward(d_o)
    opt.zero_grad()
    out_f = fused(xf)
    out_f.backward(d_o)
    _util.assert_close(out_f, ref(xr), TOL, "pair fwd")
    _util.assert_close(xf.grad, xr.grad, TOL, "pair dx")
    for (name, pr), (_, pf) in zip(ref.named_parameters(), fused.named_parameters()):
        _util.assert_close(pf.grad, pr.grad, TOL, f"pair grad {name}")


@pytest.mark.parametrize("n,h,w,use_res", [(2, 28, 28, True), (3, 4, 4, False), (1, 32, 32, True)])
def test_fused_mlp_gelu_matches_unfused_oracle(dev, n, h, w, use_res):
    """conv1x1(16->64) -> exact GELU -> conv1x1(64->16) (+ res), fused forward and backward, against
    the oracle's three separate operators (reference image_gpt.py:43-52)."""
    import torch.nn.functional as F
    from pytorch_generative_amd import nn as pg_nn, ops

    torch.manual_seed(0)
    c1, c2 = pg_nn.Conv2d(16, 64, kernel_size=1).to(dev), pg_nn.Conv2d(64, 16, kernel_size=1).to(dev)
    x, res, dy = _rand(n, 16, h, w, seed=1), _rand(n, 16, h, w, seed=2), _rand(n, 16, h, w, seed=3)
    ps = [p.detach().cpu().clone().requires_grad_(True) for p in (c1.weight, c1.bias, c2.weight, c2.bias)]
    xo, ro = x.clone().requires_grad_(True), res.clone().requires_grad_(True)
    yo = F.conv2d(F.gelu(F.conv2d(xo, ps[0], ps[1])), ps[2], ps[3])
    if use_res:
        yo = yo + ro
    yo.backward(dy)
    xg, rg = x.to(dev).requires_grad_(True), res.to(dev).requires_grad_(True)
    if not ops.FUSE_MLP:
        pytest.skip("PG_FUSE_MLP=0")
    assert ops.mlp_gelu_supported(xg, c1, c2)
    yg = ops.mlp_gelu(xg, c1, c2, res=rg if use_res else None)
    yg.backward(dy.to(dev))
    _util.assert_close(yg, yo, TOL, "mlp fwd")
    _util.assert_close(xg.grad, xo.grad, TOL, "mlp dx")
    if use_res:
        _util.assert_close(rg.grad, ro.grad, TOL, "mlp dres")
    for got, want, name in zip((c1.weight, c1.bias, c2.weight, c2.bias), ps, ("dw1", "db1", "dw2", "db2")):
        _util.assert_close(got.grad, want.grad, TOL, f"mlp {name}")


@pytest.mark.parametrize("n,hw", [(2, 28), (1, 4), (3, 12)])
def test_fused_gpt_block_matches_operator_composition(dev, n, hw):
    """forward_plus_input (head / attention / tail kernels of gpt_block.hip) against the same block
    evaluated operator by operator: output, input gradient and all 16 parameter gradients."""
    from pytorch_generative_amd import ops
    from pytorch_generative_amd.models.autoregressive import image_gpt

    torch.manual_seed(0)
    blk = image_gpt.TransformerBlock(16, 4).to(dev)
    with torch.no_grad():
        for p in blk.parameters():
            p.add_(0.05 * torch.randn_like(p))
    x = _rand(n, 16, hw, hw, seed=1).to(dev)
    d = _rand(n, 16, hw, hw, seed=2).to(dev)
    xa = x.clone().requires_grad_(True)
    if not ops.FUSE_BLOCK:
        pytest.skip("PG_FUSE_BLOCK=0")
    assert blk._fused_ok(xa)
    ya = blk.forward_plus_input(xa)
    ya.backward(d)
    ga = {k: p.grad.clone() for k, p in blk.named_parameters()}
    blk.zero_grad()
    xb = x.clone().requires_grad_(True)
    yb = ops.add(xb, blk.forward(xb))
    yb.backward(d)
    _util.assert_close(ya, yb, TOL, "block fwd")
    _util.assert_close(xa.grad, xb.grad, TOL, "block dx")
    for k, p in blk.named_parameters():
        _util.assert_close(ga[k], p.grad, TOL, f"block grad {k}")


PROTOCOL_SHAPES = [
    # (name, N, C, H, W, Cmid, k): conv1 k x k C -> Cmid, conv2 1x1 Cmid -> C
    ("b3_2x2_64", 3, 64, 16, 16, 64, 2),      # bf16x3: pipelined 4-tap kernel + barrier-free 1x1, multi-stream epilogues
    ("b3_3x3_128", 2, 128, 16, 16, 64, 3),    # bf16x3 staged kernels (9 taps; 128 -> 64 and the 1x1 back to 128)
    ("f32_3x3_24", 2, 24, 16, 16, 40, 3),     # channel counts not multiples of 8 in one direction: fp32-MFMA kernels
    ("small_8x8", 4, 64, 8, 8, 32, 3),        # < 256 pixels per image: fp32-MFMA, add fallbacks
    ("valu_3ch", 2, 3, 12, 12, 16, 3),        # 3 input channels: VALU tap kernels, no fused output activations
]


@pytest.mark.parametrize("shape", PROTOCOL_SHAPES, ids=lambda s: s[0])
def test_conv_protocol_matrix(dev, shape):
    """Every combination of the fusion protocols of nn.Conv2d.forward — in_act x (out_act, out_pre_scaled / in_post) x
    n_skip x res — through a two-convolution chain  z = conv2(A(conv1(act(x))) [+ r1]) + skips  on each dispatch class,
    against the same composition in torch on the CPU (output, dx, both weight and bias gradients). A combination the
    shape's kernels cannot take must raise ValueError AT FORWARD TIME (the documented contract: out_pre_scaled / in_post
    without the matrix-core path, or with a residual behind the activation) — never return silently wrong gradients.
    (Round 4: the first run of this matrix found exactly such a hole — out_pre_scaled + res was accepted and returned
    wrong dx / dw / db; no model used it; it raises now.)"""
    import itertools

    from pytorch_generative_amd import nn as pg_nn

    name, n, c, h, w, cmid, k = shape
    torch.manual_seed(0)
    pad = 1
    conv1 = pg_nn.Conv2d(c, cmid, k, padding=pad)
    conv2 = pg_nn.Conv2d(cmid, c, 1)
    x = _rand(n, c, h, w, seed=1)
    g = _rand(n, c, h, w, seed=2)
    r1 = _rand(n, cmid, h, w, seed=3)
    acts = {None: lambda t: t, "relu": F.relu, "elu": F.elu}
    conv1d, conv2d = conv1.to(dev), conv2.to(dev)
    pair_ok = conv1d.mfma_ok(x.to(dev), (h, w)) and conv2d.mfma_ok(torch.empty(n, cmid, h, w, device=dev))
    bad, refused, ran = [], 0, 0
    for in_act, (out_act, paired), n_skip, use_r1 in itertools.product(
            (None, "relu", "elu"), ((None, False), ("elu", False), ("elu", True)), (0, 1, 2), (False, True)):
        combo = f"in_act={in_act} out_act={out_act} paired={paired} n_skip={n_skip} res={use_r1}"
        # oracle
        xo = x.clone().requires_grad_(True)
        ws = [t.detach().cpu().clone().requires_grad_(True) for t in (conv1.weight, conv1.bias, conv2.weight, conv2.bias)]
        yo = F.conv2d(acts[in_act](xo), ws[0], ws[1], padding=pad)[:, :, :h, :w]
        if out_act:
            yo = F.elu(yo)
        if use_r1:
            yo = yo + r1
        zo = F.conv2d(yo, ws[2], ws[3]) + n_skip * xo
        zo.backward(g)
        # HIP path
        for m in (conv1d, conv2d):
            m.weight.grad = m.bias.grad = None
        xg = x.to(dev).requires_grad_(True)
        try:
            out = conv1d(xg, crop=(h, w), in_act=in_act, out_act=out_act, out_pre_scaled=paired, n_skip=n_skip,
                         res=r1.to(dev) if use_r1 else None)
            y, aliases = (out[0], list(out[1:])) if n_skip else (out, [])
            kw = {"in_post": "elu"} if paired else {}
            if n_skip == 2:
                z = conv2d(y, res=aliases[0], res2=aliases[1], **kw)
            elif n_skip == 1:
                z = conv2d(y, res=aliases[0], **kw)
            else:
                z = conv2d(y, **kw)
        except ValueError as e:
            # the documented refusals: the paired activation without matrix-core kernels, or with a residual behind it
            if not (paired and (not pair_ok or use_r1)):
                bad.append(f"{combo}: unexpected ValueError: {e}")
            refused += 1
            continue
        z.backward(g.to(dev))
        ran += 1
        for what, got, want in (("z", z, zo), ("dx", xg.grad, xo.grad), ("dw1", conv1d.weight.grad, ws[0].grad),
                                ("db1", conv1d.bias.grad, ws[1].grad), ("dw2", conv2d.weight.grad, ws[2].grad),
                                ("db2", conv2d.bias.grad, ws[3].grad)):
            e = _util.rel_err(got, want)
            if not e <= 2 * TOL:
                bad.append(f"{combo}: {what} rel err {e:.2e}")
    assert not bad, f"{name}: {len(bad)} protocol combinations wrong:\n" + "\n".join(bad[:20])
    assert ran >= 36, f"{name}: only {ran} combinations ran ({refused} refused)"
    assert refused == (9 if pair_ok else 18), f"{name}: {refused} refusals (paired activation: 9 with a residual, 18 without matrix-core kernels)"
