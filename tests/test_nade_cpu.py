"""CPU: NADE without a device — the float64 closed form of tests/_nade_ref.py reproduces the reference's recorded probabilities,
loss, gradients, Adam step and sample (tests/golden/nade/cases.pt); the model's constructor, initialisation and state_dict are
the reference's; pg_nade_plan is consistent over a sweep of shapes and the launches accept exactly what it accepts; the inputs
of tests/test_gpu_nade.py satisfy the conditions that test rests on and hit every branch of the plan; the host surface."""

import ctypes
import inspect
import os
import random

import pytest
import torch

import _nade_ref as nref
import _util
import nade_cases as nc
from test_host_cpu import _fake_ptr, _no_gpu, _reached_launch

FIXTURES = os.path.join(_util.GOLDEN_DIR, "nade", "cases.pt")
PLAN_INTS = 15
EINVAL, ESHAPE = -1, -2
F32 = 2.0 ** -23


def load_cases():
    return torch.load(FIXTURES, map_location="cpu", weights_only=False)["cases"]


def nade_mod():
    from pytorch_generative_amd.models.autoregressive import nade

    return nade


def _close(got, want, tol, what):
    err = float((got.double() - want.double()).abs().max()) / max(float(want.double().abs().max()), 1e-30)
    print(f"[nade] {what}: {err:.3e}")
    assert err <= tol, (what, err)


# ---------------------------------------------------------------------------------------------
# the float64 restatement against the reference's recorded results
@pytest.mark.parametrize("name", sorted(load_cases()))
def test_closed_form_reproduces_the_fixture(name):
    """fp32 round-off: the reference sums D (H) terms of order 1 in float32, 50 units in the last place covers it."""
    case = load_cases()[name]
    st = case["state"]
    n = case["x"].shape[0]
    x = case["x"].reshape(n, -1)
    w = [st[k] for k in nref.KEYS]
    p, _, _ = nref.forward(x, *w)
    tol = 50 * F32
    _close(p, case["probs"].reshape(n, -1), tol, f"{name} probabilities")
    loss, g = nref.recipe_loss(x, p)
    _close(loss, case["loss"], tol, f"{name} loss")
    grads = nref.grads(x, *w, g)
    for k in nref.KEYS:
        _close(grads[k], case["grads"][k], tol, f"{name} d{k}")
        # Adam's first step is lr * g / (|g| + eps): compared where the gradient is far above eps and the fp32 round-off
        big = case["grads"][k].abs() > 1e-4 * case["grads"][k].abs().max()
        after = nref.adam_first_step(st[k], grads[k])
        assert float((after - case["params_after_adam"][k].double())[big].abs().max()) <= 1e-6, k


@pytest.mark.parametrize("name", sorted(load_cases()))
def test_chain_reproduces_the_fixture_sample(name):
    """With every uniform at 0.5 the draw is p > 0.5, what the reference's sample was recorded under. No probability of that
    pass is within 1e-3 of 0.5, so rounding decides nothing."""
    case = load_cases()[name]
    cond = case["conditioned_on"]
    n = cond.shape[0]
    canvas = cond.reshape(n, -1)
    got, logits = nref.sample(canvas, *[case["sample_state"][k] for k in nref.KEYS], torch.full(canvas.shape, 0.5))
    assert torch.equal(got.float().view(cond.shape), case["sample"])
    margin = float((torch.sigmoid(logits) - 0.5).abs().min())
    assert margin >= 0.9e-3 and case["sample_margin"] > 1e-3
    given = cond >= 0
    assert bool(given.any()) and bool((~given).any())
    assert torch.equal(case["sample"][given], cond[given])


def test_fixture_covers_the_listed_cases():
    cases = load_cases()
    shapes = {(c["kwargs"]["input_dim"], c["kwargs"]["hidden_dim"], c["x"].shape[0]) for c in cases.values()}
    assert {(12, 20, 5), (16, 9, 4), (7, 1, 3)} <= shapes
    assert tuple(cases["d16_h9_n4_img"]["x"].shape) == (4, 1, 4, 4)
    real = cases["d10_h6_n4_real"]["x"]
    assert bool(((real != 0) & (real != 1)).any()) and bool((real >= 0).all())
    assert os.path.getsize(FIXTURES) < 300 * 1024


# ---------------------------------------------------------------------------------------------
# the model's host side
def test_state_dict_and_initialisation_are_the_reference():
    nade = nade_mod()
    for case in load_cases().values():
        model = nade.NADE(**case["kwargs"])
        assert sorted(model.state_dict()) == sorted(case["state"]) == sorted(nref.KEYS)
        model.load_state_dict(case["state"], strict=True)
        for k in nref.KEYS:
            assert torch.equal(model.state_dict()[k], case["state"][k])
    torch.manual_seed(0)
    model = nade.NADE(784, 500)
    assert {k: tuple(v.shape) for k, v in model.state_dict().items()} == {
        "_in_W": (500, 784), "_in_b": (500,), "_h_W": (784, 500), "_h_b": (784,)}
    assert not bool(model._in_b.any()) and not bool(model._h_b.any())
    # kaiming_normal_: std = sqrt(2 / fan_in), fan_in the second dimension
    assert abs(float(model._in_W.detach().std()) - (2 / 784) ** 0.5) < 0.02 * (2 / 784) ** 0.5
    assert abs(float(model._h_W.detach().std()) - (2 / 500) ** 0.5) < 0.02 * (2 / 500) ** 0.5
    assert inspect.signature(nade.NADE.__init__).parameters.keys() == {"self", "input_dim", "hidden_dim", "sample_fn"}


def test_exports_and_recipe_table():
    import importlib.util

    import pytorch_generative_amd as pg
    from pytorch_generative_amd import ops

    nade = nade_mod()
    assert pg.models.autoregressive.nade is nade and nade.NADE.__module__ == nade.__name__
    assert callable(ops.nade) and callable(ops.nade_plan)
    spec = importlib.util.spec_from_file_location(
        "pg_train", os.path.join(os.path.dirname(_util.GOLDEN_DIR), "..", "pytorch-generative_amd", "train.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod.MODEL_DICT["nade"] is nade
    params = inspect.signature(nade.reproduce).parameters
    assert params["n_epochs"].default == 50 and params["batch_size"].default == 512
    assert "binary_cross_entropy_with_logits" in nade.__doc__ and "teacher forcing" in nade.__doc__


def test_sample_signature_and_routes():
    nade = nade_mod()
    params = inspect.signature(nade.NADE.sample).parameters
    assert list(params) == ["self", "n_samples", "conditioned_on", "incremental", "return_logits", "generator"]
    assert all(params[k].kind is inspect.Parameter.KEYWORD_ONLY for k in ("incremental", "return_logits", "generator"))
    model = nade.NADE(12, 20)
    assert model._sample_route is None
    assert model._route(5, True) == "chain" and model._route(5, False) == "full"
    assert nade.NADE(784, 500)._route(16, True) == "chain"
    assert nade.NADE(12, 8193)._route(5, True) == "full"  # outside the sampler's plan: the reference's procedure, not an error
    with pytest.raises(ValueError, match="return_logits"):
        model.sample(conditioned_on=torch.full((2, 12), -1.0), incremental=False, return_logits=True)
    assert tuple(model._start_canvas(5, None).shape) == (5, 12)
    cond = torch.full((2, 1, 3, 4), -1.0)
    assert model._start_canvas(None, cond).shape == cond.shape and model._start_canvas(None, cond) is not cond
    model.input_codes = 4
    with pytest.raises(ValueError, match="input_codes"):
        model(torch.zeros(2, 12))
    with pytest.raises(ValueError, match="input_codes"):
        model.sample(2)


def test_cpu_tensors_and_x_grad_raise():
    from pytorch_generative_amd import ops

    t = nc.exact_inputs((12, 20, 5))
    with pytest.raises(RuntimeError, match="cuda"):
        ops.nade(t["x"], *nc.params(t))
    with pytest.raises(ValueError, match="requires_grad"):
        ops.nade(t["x"].clone().requires_grad_(True), *nc.params(t))
    model = nade_mod().NADE(12, 20)
    with pytest.raises(RuntimeError, match="cuda"):
        model(t["x"])
    with pytest.raises(RuntimeError, match="cuda"):
        model.sample(conditioned_on=torch.full((3, 12), -1.0))
    assert model._sample_route == "chain"
    with pytest.raises(RuntimeError, match="cuda"):
        model.sample(conditioned_on=torch.full((3, 12), -1.0), incremental=False)
    assert model._sample_route == "full"


# ---------------------------------------------------------------------------------------------
# planner
def _plan(lib, d, h, n):
    out = (ctypes.c_longlong * PLAN_INTS)()
    return lib.pg_nade_plan(d, h, n, out, PLAN_INTS), list(out)


def _sweep(seed=0, count=3000):
    rng = random.Random(seed)
    edge_h = [1, 2, 63, 64, 65, 255, 256, 257, 500, 512, 513, 8000, 8191, 8192, 8193, 10000, 20000]
    shapes = [(d, h, n) for d in (1, 2, 31, 32, 33, 784, 2000) for h in edge_h for n in (1, 15, 16, 17, 64, 65, 256, 257, 100000)]
    shapes += [(rng.randint(1, 3000), rng.randint(1, 20000), rng.randint(1, 5000)) for _ in range(count)]
    return shapes


def test_plan_domain_and_geometry(lib):
    """Every H <= 8192 of the sweep is accepted for any D, N >= 1 and every larger H refused with a message; the chunks cover D
    exactly, H fits its padding, the LDS fits the device, and the partial-row workspace is bounded by the cap of the rows
    whatever N is."""
    for d, h, n in _sweep():
        rc, out = _plan(lib, d, h, n)
        assert rc == (0 if h <= 8192 else ESHAPE), (d, h, n, rc)
        if rc:
            assert b"hidden units" in lib.pg_last_error()
            continue
        (chunk, chunks, units, tile, hp, fwd_groups, btile, rows, loops, bwd_groups, lds, ckpt, ws, max_rows, max_h) = out
        assert (chunk, tile, btile, max_rows, max_h) == (nc.CHUNK, nc.TILE, nc.BWD_TILE, nc.MAX_ROWS, nc.MAX_H)
        assert (chunks - 1) * chunk < d <= chunks * chunk
        assert h <= hp < h + 64 and hp % (4 * units) == 0 and units == 16
        assert fwd_groups == -(-n // tile) * chunks
        btiles = -(-n // btile)
        assert rows == min(btiles, max_rows) and loops == -(-btiles // rows) and rows * loops >= btiles
        assert bwd_groups == -(-hp // 256) * chunks * rows
        assert 0 < lds <= 64 * 1024
        assert ckpt == chunks * n * hp
        dp = chunks * chunk
        assert ws == rows * (2 * dp * hp + dp + hp) <= max_rows * (2 * dp * hp + dp + hp)
    # the workspace does not depend on N once the rows are capped
    assert _plan(lib, 784, 500, 256)[1][12] == _plan(lib, 784, 500, 10 ** 6)[1][12]
    assert _plan(lib, 784, 500, 10 ** 6)[1][8] > 1
    assert lib.pg_nade_plan(24, 20, 2, (ctypes.c_longlong * PLAN_INTS)(), PLAN_INTS - 1) == EINVAL  # short array
    assert lib.pg_nade_plan(24, 20, 2, None, PLAN_INTS) == EINVAL
    for bad in ((0, 20, 2), (24, 0, 2), (24, 20, 0), (-1, 20, 2), (24, -5, 2), (24, 20, -3)):
        assert _plan(lib, *bad)[0] == EINVAL, bad


@_no_gpu
def test_what_the_plan_accepts_reaches_the_launch(lib):
    """Fake operands, no device: a launch entry that got past its host side comes back with hipErrorNoDevice. Over the sweep the
    forward and the backward get that far exactly where the plan accepts, and refuse with the plan's status where it refuses."""
    keep, ptr = _fake_ptr()
    p = ptr.value
    big = 1 << 40
    for d, h, n in _sweep(seed=1, count=1000):
        rc_plan, out = _plan(lib, d, h, n)
        rc_f = lib.pg_nade_fwd(p, p, p, p, p, p, p, p, n, d, h, None)
        rc_b = lib.pg_nade_bwd(p, p, p, p, p, p, p, p, p, p, p, n, d, h, p, big, None)
        if rc_plan == 0:
            assert _reached_launch(lib, rc_b), (d, h, n, rc_b, lib.pg_last_error())
            rc_f = lib.pg_nade_fwd(p, p, p, p, p, p, p, p, n, d, h, None)
            assert _reached_launch(lib, rc_f), (d, h, n, rc_f, lib.pg_last_error())
            assert lib.pg_nade_bwd(p, p, p, p, p, p, p, p, p, p, p, n, d, h, p, out[12] - 1, None) == EINVAL  # short workspace
            rc_b = lib.pg_nade_bwd(p, p, p, p, p, p, p, None, None, None, None, n, d, h, p, out[12], None)  # optional outputs
            assert _reached_launch(lib, rc_b), (d, h, n, rc_b, lib.pg_last_error())
        else:
            assert rc_f == rc_b == rc_plan == ESHAPE, (d, h, n, rc_f, rc_b, rc_plan)
    for k in range(8):
        args = [p] * 8
        args[k] = None
        assert lib.pg_nade_fwd(*args, 2, 24, 20, None) == EINVAL, k
    assert lib.pg_nade_fwd(p, p, p, p, p, p + 4, p, p, 2, 24, 20, None) == EINVAL  # the checkpoints' alignment
    for k in range(7):
        args = [p] * 11
        args[k] = None
        assert lib.pg_nade_bwd(*args, 2, 24, 20, p, big, None) == EINVAL, k
    assert lib.pg_nade_bwd(*[p] * 11, 2, 24, 20, None, big, None) == EINVAL
    for n, d, h in ((0, 24, 20), (2, 0, 20), (2, 24, 0), (-1, 24, 20)):
        assert lib.pg_nade_fwd(p, p, p, p, p, p, p, p, n, d, h, None) == EINVAL
        assert lib.pg_nade_bwd(*[p] * 11, n, d, h, p, big, None) == EINVAL
    del keep


def test_plan_query_of_the_operator_layer():
    from pytorch_generative_amd import ops

    plan = ops.nade_plan(784, 500, 512)
    assert plan == {"chunk": 32, "chunks": 25, "units_per_thread": 16, "samples_per_workgroup": 64, "hidden_padded": 512,
                    "forward_workgroups": 200, "backward_tile": 16, "partial_rows": 16, "tiles_per_row": 2,
                    "backward_workgroups": 2 * 25 * 16, "lds_bytes": 48 * 1024, "checkpoint_floats": 25 * 512 * 512,
                    "workspace_floats": 16 * (2 * 800 * 512 + 800 + 512), "max_partial_rows": 16, "max_hidden": 8192}
    assert ops.nade_plan(784, 8193, 16) is None and ops.nade_plan(1, 1, 1) is not None


# ---------------------------------------------------------------------------------------------
# the inputs of the GPU test
def test_the_gpu_shapes_hit_every_branch_of_the_plan():
    """Read from ops.nade_plan: each side of every decision the geometry takes is a shape of the list."""
    from pytorch_generative_amd import ops

    plan = ops.nade_plan(784, 500, 70)
    assert (plan["chunk"], plan["samples_per_workgroup"], plan["backward_tile"], plan["max_partial_rows"]) == (
        nc.CHUNK, nc.TILE, nc.BWD_TILE, nc.MAX_ROWS)
    seen = {}
    for d, h, n in nc.EXACT_SHAPES:
        p = ops.nade_plan(d, h, n)
        assert p is not None
        facts = {"one chunk": p["chunks"] == 1, "ragged last chunk": d % p["chunk"] != 0, "padded hidden": p["hidden_padded"] > h,
                 "several hidden slabs": p["hidden_padded"] > 4 * p["units_per_thread"],
                 "several backward hidden blocks": p["hidden_padded"] > 256,
                 "several forward tiles": p["forward_workgroups"] > p["chunks"], "ragged forward tile": n % p["samples_per_workgroup"] != 0,
                 "rows at the cap": p["partial_rows"] == p["max_partial_rows"], "one row": p["partial_rows"] == 1,
                 "tile loop": p["tiles_per_row"] > 1, "ragged backward tile": n % p["backward_tile"] != 0}
        for k, v in facts.items():
            seen.setdefault(k, set()).add(v)
    assert all(v == {True, False} for v in seen.values()), seen
    ds, hs, ns = ({s[i] for s in nc.EXACT_SHAPES} for i in range(3))
    assert {1, nc.CHUNK - 1, nc.CHUNK, nc.CHUNK + 1, 2 * nc.CHUNK + 3} <= ds and {1, 63, 64, 65, 500} <= hs
    assert {1, 2, nc.TILE - 1, nc.TILE + 1} <= ns and max(ns - {70}) > nc.BWD_TILE * nc.MAX_ROWS
    assert (784, 500, 70) in nc.EXACT_SHAPES


@pytest.mark.parametrize("shape", nc.EXACT_SHAPES, ids=nc.shape_id)
def test_exact_cases_have_one_recurrence_in_both_precisions(shape):
    """x in {0, 1} and weights on 2^-10 Z below 4, D <= 784: every partial sum fits 24 bits, so the fp32 sequential recurrence IS
    the float64 one (and the closed form), and the ReLU masks cannot differ."""
    t = nc.exact_inputs(shape)
    assert shape[0] <= 784 and bool(((t["x"] == 0) | (t["x"] == 1)).all())
    for k in ("_in_W", "_in_b"):
        assert bool((t[k] * 1024 == (t[k] * 1024).round()).all()) and float(t[k].abs().max()) < 4
    a32 = nref.recurrence(t["x"], t["_in_W"], t["_in_b"], torch.float32)
    a64 = nref.recurrence(t["x"], t["_in_W"], t["_in_b"], torch.float64)
    assert torch.equal(a32.double(), a64)
    assert torch.equal(a64, nref.preact(t["x"], t["_in_W"], t["_in_b"]))
    assert float(a64.abs().max()) < 2 ** 13


@pytest.mark.parametrize("shape", nc.GENERIC_SHAPES, ids=nc.shape_id)
def test_generic_cases_keep_every_relu_argument_off_zero(shape):
    t, margin = nc.generic_inputs(shape)
    assert shape[0] * shape[1] * shape[2] <= 10 ** 4
    a = nref.preact(t["x"], t["_in_W"], t["_in_b"])
    assert float(a.abs().min()) == margin >= nc.GENERIC_MARGIN
    assert bool((t["x"] < 0).any()) and bool(((t["x"] != 0) & (t["x"] != 1)).all())
    # both signs of the ReLU occur, so its mask matters
    assert bool((a > 0).any()) and bool((a < 0).any())
