"""CPU: the categorical pixel likelihood without a device — the float64 reference helpers against themselves, the header /
binding entries, the argument checks of the four entry points (no launch for a rejected call), the planner's geometry
over a sweep of shapes, and the public surface (ops on CPU tensors raise, nn.CategoricalSampler, recipes, the alias)."""

import ctypes
import itertools
import os
import re

import pytest
import torch

import _categorical_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("pg_categorical_plan", "pg_categorical_nll_fwd", "pg_categorical_nll_bwd", "pg_categorical_sample")


def test_level_round_trip_is_exact():
    for k in range(2, 520):
        lv = ref.levels(k)
        assert lv.dtype == torch.float32
        assert torch.equal(ref.classes(lv, k), torch.arange(k)), k
        assert torch.equal(ref.to_level(torch.arange(k), k), lv), k
    # out-of-range values (the -1 of an unfilled canvas, dequantisation noise) clamp to the end classes
    assert ref.classes(torch.tensor([-1.0, -0.2, 1.2, 7.0]), 5).tolist() == [0, 0, 4, 4]


@pytest.mark.parametrize("k,c,temperature", [(2, 1, 1.0), (7, 3, 0.5), (256, 1, 1.0), (257, 2, 2.0)])
def test_pick_agrees_with_searchsorted(k, c, temperature):
    g = torch.Generator().manual_seed(k * 13 + c)
    n = 50
    logits = torch.randn(n, k * c, generator=g) * 3
    u = torch.rand(n, c, generator=g)
    run, total = ref.cdf(logits, k, temperature)
    assert run.dtype == torch.float64 and run.shape == (n, c, k)
    # first index with run > u * total  ==  number of entries <= u * total  ==  searchsorted(..., right=True)
    want = torch.searchsorted(run, (u.double() * total).unsqueeze(2), right=True).squeeze(2).clamp(max=k - 1)
    got = ref.pick(logits, u, k, temperature)
    assert torch.equal(got, want)
    assert int(got.min()) >= 0 and int(got.max()) <= k - 1


def test_pick_edge_cases():
    k = 5
    logits = torch.zeros(1, k)
    logits[0, 0] = -200.0  # e_0 = exp(-200) is positive in float64: the threshold has to lie above it to reach class 1
    assert ref.pick(logits, torch.tensor([[1e-30]]), k).item() == 1
    trailing = torch.tensor([[0.0, 0.0, 0.0, -2000.0, -2000.0]])  # the last two classes have no mass in float64 either
    u1 = torch.nextafter(torch.tensor([[1.0]]), torch.tensor([[0.0]]))
    assert ref.pick(trailing, u1, k).item() == 2
    assert ref.pick(trailing, torch.tensor([[0.0]]), k).item() == 0


def test_reference_loss_and_gradient():
    g = torch.Generator().manual_seed(0)
    n, c, k, h, w = 3, 2, 5, 2, 3
    logits = torch.randn(n, k * c, h, w, generator=g)
    images = ref.to_level(torch.randint(0, k, (n, c, h, w), generator=g), k)
    z = logits.double().view(n, k, c, h, w)
    t = ref.classes(images, k)
    by_hand = (torch.logsumexp(z, 1) - z.gather(1, t.unsqueeze(1)).squeeze(1)).sum((1, 2, 3))
    assert torch.allclose(ref.nll_per_sample(logits, images, k), by_hand, rtol=1e-12, atol=1e-12)
    assert torch.allclose(ref.lse(logits, k), torch.logsumexp(z, 1))
    loss, grad = ref.loss_and_grad(logits, images, k, grad_output=0.5)
    assert torch.allclose(loss, by_hand.mean())
    onehot = torch.zeros_like(z).scatter_(1, t.unsqueeze(1), 1.0)
    want = 0.5 / n * (torch.softmax(z, 1) - onehot)
    assert torch.allclose(grad, want.view(n, k * c, h, w), rtol=1e-12, atol=1e-15)


def test_header_and_signatures_name_the_entry_points(lib):
    from pytorch_generative_amd import _lib

    header = open(os.path.join(ROOT, "include", "pg_hip.h")).read()
    for name in ENTRY_POINTS:
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), f"{name} not declared in include/pg_hip.h"
        assert name in _lib.SIGNATURES, name
        assert hasattr(lib, name), name
    assert _lib.ABI_VERSION == 3 and lib.pg_abi_version() == 3


def test_entry_points_reject_bad_arguments(lib):
    """Shape errors -2, null operands -1, for every entry point; nothing is launched (there is no device here, and the
    operands of the shape cases are the address 1)."""
    from pytorch_generative_amd import _lib

    lanes, vec = ctypes.c_int(-7), ctypes.c_int(-7)
    good = (4, 1, 8, 16)
    bad = [(0, 1, 8, 16), (-1, 1, 8, 16), (4, 0, 8, 16), (4, -3, 8, 16), (4, 1, 0, 16), (4, 1, -2, 16), (4, 1, 1, 16),
           (4, 1, 4097, 16), (4, 1, 8, 0), (4, 1, 8, -5)]
    for n, c, k, hw in bad:
        what = (n, c, k, hw)
        rc = lib.pg_categorical_plan(n, c, k, hw, ctypes.byref(lanes), ctypes.byref(vec))
        assert rc == -2, what
        with pytest.raises(ValueError):
            _lib.check(rc, "pg_categorical_plan")
        assert lib.pg_categorical_nll_fwd(1, 1, 1, 1, 1, n, c, k, hw, 0) == -2, what
        assert lib.pg_categorical_nll_bwd(1, 1, 1, 1, 1, n, c, k, hw, 0) == -2, what
        if hw == good[3]:  # the sampler has no HW
            assert lib.pg_categorical_sample(1, k * max(c, 1), 1, 1, 1, n, c, k, 1.0, 0) == -2, what
    assert (lanes.value, vec.value) == (-7, -7), "a rejected plan must not write its outputs"
    n, c, k, hw = good
    assert lib.pg_categorical_plan(n, c, k, hw, None, ctypes.byref(vec)) == -1
    assert lib.pg_categorical_plan(n, c, k, hw, ctypes.byref(lanes), None) == -1
    for hole in range(5):  # logits, x, lse, per_sample, loss: only per_sample may be null — and then there is a launch, so it is not tried
        if hole == 3:
            continue
        ptrs = [1] * 5
        ptrs[hole] = 0
        assert lib.pg_categorical_nll_fwd(*ptrs, n, c, k, hw, 0) == -1, hole
    for hole in range(5):  # logits, x, lse, g, dlogits
        ptrs = [1] * 5
        ptrs[hole] = 0
        assert lib.pg_categorical_nll_bwd(*ptrs, n, c, k, hw, 0) == -1, hole
    for hole in range(3):  # logits, uniforms, out
        ptrs = [1] * 3
        ptrs[hole] = 0
        assert lib.pg_categorical_sample(ptrs[0], k * c, 1, ptrs[1], ptrs[2], n, c, k, 1.0, 0) == -1, hole
    for sn, sk in ((0, 1), (8, 0), (-8, 1), (8, -1)):
        assert lib.pg_categorical_sample(1, sn, sk, 1, 1, n, c, k, 1.0, 0) == -1, (sn, sk)
    for inv_t in (0.0, -1.0, float("inf"), float("nan")):
        assert lib.pg_categorical_sample(1, k * c, 1, 1, 1, n, c, k, inv_t, 0) == -1, inv_t
    with pytest.raises(ValueError, match="null pointer"):
        _lib.check(lib.pg_categorical_nll_bwd(0, 1, 1, 1, 1, n, c, k, hw, 0), "pg_categorical_nll_bwd")


def test_plan_sweep(lib):
    lanes, vec = ctypes.c_int(), ctypes.c_int()
    seen = set()
    for n, c, k, hw in itertools.product((1, 2, 64, 1024), (1, 3), (2, 3, 7, 16, 255, 256, 257, 512, 4096),
                                         (1, 5, 16, 784, 1024)):
        what = (n, c, k, hw)
        assert lib.pg_categorical_plan(n, c, k, hw, ctypes.byref(lanes), ctypes.byref(vec)) == 0, what
        s, v = lanes.value, vec.value
        assert 1 <= s <= 64 and s & (s - 1) == 0, (what, s)
        assert v in (1, 4), (what, v)
        assert v == 1 or hw % 4 == 0, (what, v)
        assert v == (4 if hw % 4 == 0 else 1), (what, v)  # the vector path is taken whenever the shape allows it
        assert s == 1 or s * 64 <= k, (what, s)            # a lane keeps at least 64 classes ...
        assert s == 8 or 2 * s * 64 > k, (what, s)         # ... and the split goes as far as that allows, up to 8
        seen.add((s, v))
    # the recipe's shape splits the classes of a pixel over lanes
    assert lib.pg_categorical_plan(64, 1, 256, 784, ctypes.byref(lanes), ctypes.byref(vec)) == 0
    assert lanes.value > 1 and vec.value == 4
    assert {s for s, _ in seen} == {1, 2, 4, 8} and {v for _, v in seen} == {1, 4}


def test_gpu_parity_shapes_reach_every_split(lib):
    """The planner is a function of K and HW % 4: the GPU parity cases must between them run every split and both widths."""
    import test_gpu_categorical as gpu_cases

    lanes, vec = ctypes.c_int(), ctypes.c_int()
    reached = set()
    for n, c, k, h, w in gpu_cases.SHAPES + gpu_cases.SPLIT_SHAPES:
        assert lib.pg_categorical_plan(n, c, k, h * w, ctypes.byref(lanes), ctypes.byref(vec)) == 0
        reached.add((lanes.value, vec.value))
    assert {s for s, _ in reached} == {1, 2, 4, 8}, reached  # all the planner gives (test_plan_sweep)
    for s in (1, 2, 8):
        assert {(s, 1), (s, 4)} <= reached, (s, reached)
    for shape in gpu_cases.SHAPES + gpu_cases.SPLIT_SHAPES:
        assert (shape, "plain") in gpu_cases.VARIANTS
        assert (shape, "wide") in gpu_cases.VARIANTS or shape == gpu_cases.RECIPE


def test_cpu_tensors_raise():
    from pytorch_generative_amd import nn as pg_nn
    from pytorch_generative_amd import ops, recipes

    logits, images = torch.zeros(2, 8, 3, 3), torch.zeros(2, 1, 3, 3)
    with pytest.raises(RuntimeError, match="cuda"):
        ops.categorical_nll_sum_mean(logits, images, 8)
    with pytest.raises(RuntimeError, match="cuda"):
        ops.categorical_nll_per_sample(logits, images, 8)
    with pytest.raises(RuntimeError, match="cuda"):
        ops.categorical_sample(torch.zeros(2, 8), torch.zeros(2, 1), 8)
    with pytest.raises(RuntimeError, match="cuda"):
        pg_nn.CategoricalSampler(8).draw(torch.zeros(2, 8), torch.zeros(2, 1))
    with pytest.raises(RuntimeError, match="cuda"):
        recipes.categorical_loss(8)(images, None, logits)
    for k in (1, 4097):
        with pytest.raises(ValueError):
            pg_nn.CategoricalSampler(k)
        with pytest.raises(ValueError):
            ops.categorical_sample(torch.zeros(2, 8), torch.zeros(2, 1), k)
    with pytest.raises(ValueError):
        pg_nn.CategoricalSampler(8, temperature=0.0)


def test_exports_and_alias():
    import pytorch_generative_amd.compat as compat
    from pytorch_generative_amd import nn as pg_nn
    from pytorch_generative_amd import ops, recipes

    assert "CategoricalSampler" in pg_nn.__all__
    for name in ("categorical_nll_sum_mean", "categorical_nll_per_sample", "categorical_sample"):
        assert callable(getattr(ops, name)), name
    assert callable(recipes.categorical_loss(256)) and callable(recipes.grey_mnist)
    pg = compat.install_alias()
    import pytorch_generative.nn as alias_nn
    from pytorch_generative.nn import utils as alias_utils

    assert alias_nn.CategoricalSampler is pg_nn.CategoricalSampler
    assert alias_utils.CategoricalSampler is pg_nn.CategoricalSampler
    assert pg.nn.CategoricalSampler is pg_nn.CategoricalSampler
    sampler = pg_nn.CategoricalSampler(256, temperature=0.5)
    assert (sampler.n_classes, sampler.temperature, sampler.generator) == (256, 0.5, None)

