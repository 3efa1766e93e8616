"""CPU: the fused head + categorical likelihood (csrc/linear_categorical.hip) without a device — the float64 restatement of
tests/_linear_categorical_ref.py pinned against torch autograd, the planner's geometry and the argument checks of the entry
points over a sweep of random problems, and the public surface (DeferredLogits, defer_head, the bindings)."""

import ctypes
import os
import random
import re

import pytest
import torch

import _linear_categorical_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("pg_linear_categorical_plan", "pg_linear_categorical_nll_fwd", "pg_linear_categorical_nll_bwd",
                "pg_linear_categorical_reduce")
TRANSFORM_ID = {"none": 0, "relu": 1, "ln": 2}
LDS_LIMIT = 160 * 1024
_no_gpu = pytest.mark.skipif(torch.cuda.is_available(), reason="sweeps the launches with fake pointers: CPU box only")


# ---- the float64 restatement -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("transform", ref.TRANSFORMS)
@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("shape", [(1, 4, 2, 1, 1, 1), (3, 20, 7, 3, 2, 3), (2, 16, 33, 1, 4, 4), (4, 8, 5, 2, 1, 5)],
                         ids=lambda s: "x".join(map(str, s)))
def test_chain_rule_matches_autograd(shape, bias, transform):
    case = ref.make_case(shape, transform, bias=bias)
    for grad_output in (1.0, 0.5):
        mine = ref.reference(case, grad_output)
        auto = ref.reference(case, grad_output, fn=ref.by_autograd)
        assert set(mine) == set(auto)
        for name in mine:
            assert mine[name].dtype == torch.float64 and mine[name].shape == auto[name].shape, name
            scale = float(auto[name].abs().max().clamp_min(1e-300))
            err = float((mine[name] - auto[name]).abs().max()) / scale
            assert err <= 1e-12, f"{shape} {transform} bias={bias} {name}: {err:.2e}"


@pytest.mark.parametrize("variant", ["wide", "equal"])
def test_variants_do_what_they_say(variant):
    for shape in ((3, 20, 7, 3, 2, 3), (2, 16, 256, 1, 4, 4)):
        for transform in ref.TRANSFORMS:
            case = ref.make_case(shape, transform, variant)
            z = ref.logits(case["h"], case["w"], case["b"], transform, case["ln_w"], case["ln_b"], case["eps"])
            n, cin, k, c, hh, ww = shape
            t = ref.cref.classes(case["images"], k)
            assert int(t.min()) == 0 and int(t.max()) == k - 1
            if variant == "wide":
                assert float(z.abs().max()) > 89.0, "exp(z) must overflow fp32 without the max subtraction"
            else:
                spread = (z.view(n, k, c, hh * ww).max(dim=1).values - z.view(n, k, c, hh * ww).min(dim=1).values)
                equal = spread == 0
                assert 0.3 <= float(equal.double().mean()) <= 0.7, "about half the sub-pixels have K equal logits"


def test_wide_logits_leave_the_gate_to_the_kernel():
    """Rounding the wide logits to fp32 (what any fp32 evaluation of W h + b does at best) moves the gradients by a small
    part of the element-wise gate of tests/_util.GradReport: the GPU test's wide variant tests the kernel, not the gate."""
    import _util

    worst = 0.0
    for shape in ((3, 20, 7, 3, 2, 3), (2, 16, 256, 1, 4, 4)):
        for transform in ref.TRANSFORMS:
            case = ref.make_case(shape, transform, "wide")
            want = ref.reference(case)
            y = ref.transformed(case["h"], transform, case["ln_w"], case["ln_b"], case["eps"])
            z32 = ref.logits(case["h"], case["w"], case["b"], transform, case["ln_w"], case["ln_b"], case["eps"]).float()
            _, dz = ref.cref.loss_and_grad(z32, case["images"], case["k"])
            got = {"dW": torch.einsum("nohw,nchw->oc", dz, y), "db": dz.sum(dim=(0, 2, 3))}
            for name, g in got.items():
                m = float(want[name].abs().max())
                ratio = float(((g - want[name]).abs() / (_util.GRAD_TOL * want[name].abs() + _util.GRAD_FLOOR * m)).max())
                worst = max(worst, ratio)
    print(f"[linear_categorical] fp32 rounding of the wide logits uses {worst:.3f} of the element-wise gate")
    assert worst <= 0.14


# ---- bindings and argument checks ----------------------------------------------------------------------------------------

def test_header_and_signatures_name_the_entry_points(lib):
    from pytorch_generative_amd import _lib

    header = open(os.path.join(ROOT, "include", "pg_hip.h")).read()
    for name in ENTRY_POINTS:
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", header)
        assert m, f"{name} not declared in include/pg_hip.h"
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
        assert len(_lib.SIGNATURES[name][1]) == len(m.group(1).split(",")), f"{name}: argument count differs from the header"
    assert [int(re.search(r"#define PG_LC_" + n + r" (\d)", header).group(1)) for n in ("NONE", "RELU", "LN")] == [0, 1, 2]
    from pytorch_generative_amd.ops import linear_categorical as lc

    assert (lc.TRANSFORM_NONE, lc.TRANSFORM_RELU, lc.TRANSFORM_LN) == (0, 1, 2)


def _plan(lib, n, c, k, cin, hw, transform):
    ppt, rows, lds = ctypes.c_int(-7), ctypes.c_int(-7), ctypes.c_int(-7)
    ws = ctypes.c_size_t(7)
    rc = lib.pg_linear_categorical_plan(n, c, k, cin, hw, transform, ctypes.byref(ppt), ctypes.byref(rows), ctypes.byref(lds),
                                        ctypes.byref(ws))
    return rc, ppt.value, rows.value, lds.value, ws.value


def _fwd(lib, p, n, c, k, cin, hw, transform, ln=True):
    lnp = p if ln else None
    return lib.pg_linear_categorical_nll_fwd(p, p, p, lnp, lnp, 1e-5, p, p, None, p, n, c, k, cin, hw, transform, None)


def _bwd(lib, p, n, c, k, cin, hw, transform, ws_floats, ln=True):
    lnp = p if ln else None
    return lib.pg_linear_categorical_nll_bwd(p, p, p, lnp, lnp, 1e-5, p, p, p, p, n, c, k, cin, hw, transform, p, ws_floats, None)


def _fake_ptr():
    import numpy as np

    buf = np.zeros(1 << 12, dtype=np.float32)
    return buf, ctypes.c_void_p((buf.ctypes.data + 255) // 256 * 256)


def _in_domain(n, c, k, cin, hw, transform):
    return (n >= 1 and c >= 1 and hw >= 1 and 2 <= k <= 4096 and cin % 4 == 0 and 4 <= cin <= 256 and transform in (0, 1, 2)
            and c * hw < 2 ** 31 and n * c * hw < 2 ** 31 and n * c * hw * k < 2 ** 40 and n * hw + 16 < 2 ** 31
            and k * c * (cin + 1) + 2 * cin < 2 ** 31)


def test_entry_points_reject_bad_arguments(lib):
    """Shape errors -2, null or misaligned operands and a short workspace -1; nothing is launched (the operands are fake)."""
    keep, p = _fake_ptr()
    good = (4, 1, 8, 16, 16, 2)  # N, C, K, Cin, HW, transform
    bad = [(0, 1, 8, 16, 16, 2), (4, 0, 8, 16, 16, 2), (4, 1, 1, 16, 16, 2), (4, 1, 4097, 16, 16, 2), (4, 1, 8, 0, 16, 2),
           (4, 1, 8, 6, 16, 2), (4, 1, 8, 2, 16, 0), (4, 1, 8, 260, 16, 2), (4, 1, 8, 16, 0, 2), (4, 1, 8, 16, 16, 3),
           (4, 1, 8, 16, 16, -1), (1 << 20, 1, 4096, 16, 1 << 10, 0)]
    for what in bad:
        rc, ppt, rows, lds, ws = _plan(lib, *what)
        assert rc == -2 and (ppt, rows, lds, ws) == (-7, -7, -7, 7), what
        assert _fwd(lib, p, *what) == -2, what
        assert _bwd(lib, p, *what, 1 << 30) == -2, what
    assert lib.pg_linear_categorical_reduce(p, 0, 8, 16, 2, p, p, p, p, None) == -2
    assert lib.pg_linear_categorical_reduce(p, 1, 8, 6, 2, p, p, p, p, None) == -2
    assert lib.pg_linear_categorical_reduce(p, 1, 8, 16, 5, p, p, p, p, None) == -2
    assert lib.pg_linear_categorical_reduce(None, 1, 8, 16, 2, p, p, p, p, None) == -1
    assert lib.pg_linear_categorical_reduce(p, 1, 8, 16, 2, None, p, p, p, None) == -1
    n, c, k, cin, hw, tr = good
    rc, ppt, rows, lds, ws = _plan(lib, *good)
    assert rc == 0
    assert lib.pg_linear_categorical_plan(n, c, k, cin, hw, tr, None, None, None, None) == -1
    assert _fwd(lib, p, *good, ln=False) == -1, "LayerNorm without its parameters"
    assert _bwd(lib, p, *good, ws, ln=False) == -1
    assert _bwd(lib, p, *good, ws - 1) == -1, "a short workspace"
    odd = ctypes.c_void_p(p.value + 4)
    assert lib.pg_linear_categorical_nll_fwd(p, odd, p, p, p, 1e-5, p, p, None, p, n, c, k, cin, hw, tr, None) == -1, "misaligned w"
    for hole in (0, 1, 6, 7, 9):  # h, w, x, lse, loss
        args = [p, p, p, p, p, 1e-5, p, p, None, p]
        args[hole] = None
        assert lib.pg_linear_categorical_nll_fwd(*args, n, c, k, cin, hw, tr, None) == -1, hole
    for hole in (0, 1, 6, 7, 8, 9):  # h, w, x, lse, g, dh
        args = [p, p, p, p, p, 1e-5, p, p, p, p]
        args[hole] = None
        assert lib.pg_linear_categorical_nll_bwd(*args, n, c, k, cin, hw, tr, p, ws, None) == -1, hole
    assert lib.pg_linear_categorical_nll_bwd(p, p, p, p, p, 1e-5, p, p, p, p, n, c, k, cin, hw, tr, None, ws, None) == -1
    del keep


@pytest.mark.parametrize("seed", range(4))
def test_plan_sweep(lib, seed):
    """1500 random problems per seed. Accepted: the rows' tile ranges cover every pixel exactly once, LDS within 160 KB, the
    workspace is rows times the documented row length and within a quarter of the logits unless one row alone exceeds that.
    Outside the domain: PG_ESHAPE from the planner and both launches."""
    keep, p = _fake_ptr()
    r = random.Random(seed)
    accepted = refused = 0
    for _ in range(1500):
        n = r.choice([1, 2, 3, 5, 64, 70, 1024, 0, -1])
        c = r.choice([1, 1, 1, 2, 3, 0])
        k = r.choice([2, 3, 7, 16, 17, 255, 256, 257, 512, 1000, 4096, 1, 4097])
        cin = r.choice([4, 8, 12, 16, 20, 32, 64, 100, 128, 252, 256, 0, 2, 6, 18, 260])
        hw = r.choice([1, 5, 15, 16, 17, 35, 64, 784, 1024, 0])
        tr = r.choice([0, 1, 2, 2, 3])
        what = (n, c, k, cin, hw, tr)
        rc, ppt, rows, lds, ws = _plan(lib, *what)
        if not _in_domain(*what):
            assert rc == -2, what
            assert _fwd(lib, p, *what) == -2 and _bwd(lib, p, *what, 1 << 40) == -2, what
            refused += 1
            continue
        assert rc == 0, what
        accepted += 1
        pixels = n * hw
        tiles = -(-pixels // ppt)
        assert ppt == 16 and 1 <= rows <= tiles, (what, ppt, rows)
        tpr = -(-tiles // rows)
        covered = 0
        for row in range(rows):  # row `row` owns the tiles [row * tpr, min((row + 1) * tpr, tiles))
            t0, t1 = row * tpr, min((row + 1) * tpr, tiles)
            assert t0 < t1, (what, "an empty row")
            assert t0 * ppt == covered, (what, "a gap or an overlap")
            covered = min(t1 * ppt, pixels)
        assert covered == pixels, what
        row_len = k * c * cin + k * c + 2 * cin
        assert ws == rows * row_len, what
        cap = n * k * c * hw // 4
        assert ws <= cap or rows == 1, (what, ws, cap)
        assert 0 < lds <= LDS_LIMIT, (what, lds)
    assert accepted >= 300 and refused >= 300, (accepted, refused)
    del keep


@_no_gpu
@pytest.mark.parametrize("seed", range(2))
def test_accepted_problems_reach_the_launch(lib, seed):
    """Without a device a launch fails with a positive HIP status after every host-side check has passed."""
    keep, p = _fake_ptr()
    r = random.Random(100 + seed)
    for _ in range(300):
        what = (r.choice([1, 3, 64]), r.choice([1, 3]), r.choice([2, 7, 256, 257, 4096]), r.choice([4, 16, 20, 64, 256]),
                r.choice([1, 5, 16, 784]), r.choice([0, 1, 2]))
        rc, ppt, rows, lds, ws = _plan(lib, *what)
        assert rc == 0, what
        assert _fwd(lib, p, *what) > 0, what
        assert _bwd(lib, p, *what, ws) > 0, what
        n, c, k, cin, hw, tr = what
        assert lib.pg_linear_categorical_reduce(p, rows, k * c, cin, tr, p, p, p, p, None) > 0, what
    del keep


# ---- the public surface ----------------------------------------------------------------------------------------------------

def _models():
    import pytorch_generative_amd as pg

    m = pg.models
    return {
        "ImageGPT": lambda: m.ImageGPT(in_channels=1, out_channels=8, in_size=8, n_transformer_blocks=1, n_attention_heads=2,
                                       n_embedding_channels=4),
        "PixelCNN": lambda: m.PixelCNN(in_channels=1, out_channels=8, n_residual=1, residual_channels=4, head_channels=8),
        "GatedPixelCNN": lambda: m.GatedPixelCNN(in_channels=1, out_channels=8, n_gated=1, gated_channels=4, head_channels=8),
        "PixelSNAIL": lambda: m.PixelSNAIL(in_channels=1, out_channels=8, n_channels=8, n_pixel_snail_blocks=1,
                                           n_residual_blocks=1, attention_key_channels=2, attention_value_channels=4),
    }


@pytest.mark.parametrize("name", ["ImageGPT", "PixelCNN", "GatedPixelCNN", "PixelSNAIL"])
def test_defer_head_is_an_attribute_and_off_by_default(name):
    import inspect

    from pytorch_generative_amd.models import base

    assert base.AutoregressiveModel.defer_head is False
    model = _models()[name]()
    assert model.defer_head is False and "defer_head" not in vars(model)
    assert "defer_head" not in inspect.signature(type(model).__init__).parameters
    keys = list(model.state_dict())
    model.defer_head = True
    assert list(model.state_dict()) == keys and not any("defer" in key for key in keys)


def test_deferred_logits_surface():
    from pytorch_generative_amd import nn as pg_nn
    from pytorch_generative_amd import ops, recipes

    conv = pg_nn.Conv2d(in_channels=8, out_channels=24, kernel_size=1)
    ln = pg_nn.NCHWLayerNorm(8)
    h = torch.zeros(2, 8, 3, 5)
    d = ops.DeferredLogits(h, conv, pre_ln=ln)
    assert not torch.is_tensor(d)
    assert d.shape == (2, 24, 3, 5) and isinstance(d.shape, torch.Size)
    assert ops.DeferredLogits(h, conv, in_act="relu").in_act == "relu"
    with pytest.raises(ValueError):
        ops.DeferredLogits(h, conv, in_act="relu", pre_ln=ln)
    with pytest.raises(ValueError):
        ops.DeferredLogits(torch.zeros(2, 4, 3, 5), conv)
    assert not ops.linear_categorical_supported(h, conv, None, ln), "CPU features are not supported"
    images = torch.zeros(2, 3, 3, 5)
    with pytest.raises(RuntimeError, match="cuda"):  # no CPU path: the dense route it falls to raises as always
        ops.categorical_nll_sum_mean(d, images, 8)
    with pytest.raises(RuntimeError, match="cuda"):
        ops.categorical_nll_per_sample(d, images, 8)
    with pytest.raises(RuntimeError, match="cuda"):
        recipes.categorical_loss(8)(images, None, d)
    with pytest.raises(ValueError):
        ops.categorical_nll_sum_mean(d, images, 7)  # 24 channels are not 7 classes of 3
    with pytest.raises(ValueError):
        ops.categorical_nll_sum_mean(d, images, 4097)


def test_recipes_run_takes_defer_head():
    import inspect

    from pytorch_generative_amd import recipes

    p = inspect.signature(recipes.run).parameters["defer_head"]
    assert p.default is False and p.kind is inspect.Parameter.KEYWORD_ONLY
