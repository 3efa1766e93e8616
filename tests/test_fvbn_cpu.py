"""CPU: the FVBN without a device — the packed layout of ops.fvbn_offsets against the Python formula of tests/_fvbn_ref.py;
pg_fvbn_plan over a sweep of shapes up to the domain's edge and beyond (the rectangles it lists hold every (i, j < i) exactly
once, the workspace holds the reported slices); the float64 restatement against the reference's recorded results
(tests/golden/fvbn/cases.pt); the model's state_dict speaks the reference's keys, order, shapes and bits and keeps the pads
zero; the initialisation's distribution; the public surface."""

import ctypes
import inspect
import os
import random

import numpy as np
import pytest
import torch

import _fvbn_ref as fref
import _util

FIXTURES = os.path.join(_util.GOLDEN_DIR, "fvbn", "cases.pt")
PLAN_INTS = 22
EINVAL, ESHAPE = -1, -2
TILES_FWD, TILES_WGRAD = 0, 1
MAX_D, MAX_N = 8192, 1 << 30
F32 = 2.0 ** -23


def load_cases():
    return torch.load(FIXTURES, map_location="cpu", weights_only=False)["cases"]


def fvbn_mod():
    from pytorch_generative_amd.models.autoregressive import fvbn

    return fvbn


def _close(got, want, tol, what):
    err = float((got.double() - want.double()).abs().max()) / max(float(want.double().abs().max()), 1e-30)
    print(f"[fvbn] {what}: {err:.3e}")
    assert err <= tol, (what, err)


# ---------------------------------------------------------------------------------------------
# the packed layout
def test_offsets_match_the_python_formula(lib):
    from pytorch_generative_amd import ops

    assert [fref.pad(i) for i in range(10)] == [4, 4, 4, 4, 4, 8, 8, 8, 8, 12]
    assert fref.off(0) == 0 and fref.off(1) == 4 and fref.off(6) == 28
    for d in list(range(1, 301)) + [8192]:
        got = ops.fvbn_offsets(d)
        want = fref.offsets(d)
        assert got.dtype == torch.int64 and got.tolist() == want, d
        assert all(o % 4 == 0 for o in want)
        assert ops.fvbn_plan(d, 1)["packed_floats"] == want[-1] == fref.packed_floats(d)
    assert lib.pg_fvbn_row_offset(-1) == -1
    # the closed form the kernels use stays inside 64 bits and above D^2 / 2
    assert fref.packed_floats(8192) >= 8192 * 8191 // 2


def test_pack_and_unpack_restatement_round_trips():
    g = torch.Generator().manual_seed(0)
    for d in (1, 2, 5, 9, 17):
        w = torch.randn(d, d, generator=g)
        p = fref.pack(w)
        assert p.numel() == fref.packed_floats(d) and not bool(p[fref.pad_mask(d)].any())
        back = fref.unpack(p, d)
        want = torch.tril(w, -1)
        want[0, 0] = w[0, 0]
        assert torch.equal(back, want) and torch.equal(fref.pack(back), p)


# ---------------------------------------------------------------------------------------------
# planner
def _plan(lib, d, n):
    out = (ctypes.c_longlong * PLAN_INTS)()
    return lib.pg_fvbn_plan(d, n, out, PLAN_INTS), list(out)


def _covered_once(d, tiles):
    """Every (i, j < i) lies in exactly one rectangle [i0, i1) x [j0, j1); a rectangle is non-empty and inside (D, D)."""
    count = np.zeros((d, d), dtype=np.int8)
    for i0, i1, j0, j1 in tiles:
        assert 0 <= i0 < i1 <= d and 0 <= j0 < j1 <= d, (d, i0, i1, j0, j1)
        assert j0 <= i1 - 1, "a rectangle wholly above the diagonal is listed"
        count[i0:i1, j0:j1] += 1
    lower = np.tril(np.ones((d, d), dtype=bool), -1)
    return bool((count[lower] == 1).all())


def _sweep(seed=0, count=400):
    rng = random.Random(seed)
    shapes = [(d, n) for d in (1, 2, 3, 4, 5, 33, 63, 64, 65, 128, 129, 784, 3072, 8191, 8192)
              for n in (1, 2, 31, 32, 33, 64, 65, 127, 128, 129, 512, 100000, MAX_N)]
    shapes += [(rng.randint(1, MAX_D), rng.randint(1, 5000)) for _ in range(count)]
    shapes += [(rng.randint(1, 400), rng.randint(1, 5000)) for _ in range(count)]
    shapes += [(d, n) for d in (0, -1, 8193, 20000) for n in (1, 64)] + [(d, n) for d in (1, 784) for n in (0, -5, MAX_N + 1)]
    return shapes


def test_plan_domain_and_geometry(lib):
    from pytorch_generative_amd import ops

    lim = 2 ** 31 - 1
    for d, n in _sweep():
        rc, out = _plan(lib, d, n)
        inside = 1 <= d <= MAX_D and 1 <= n <= MAX_N
        tile = 64
        groups = -(-max(d, 1) // tile) * -(-max(n, 1) // tile)
        assert rc == (0 if inside and groups <= lim else ESHAPE), (d, n, rc)
        if rc:
            assert lib.pg_last_error()
            assert ops.fvbn_plan(d, n) is None
            continue
        (packed, t, kc, col_tiles, row_tiles, fwd_groups, fwd_tiles, tiles, slices, nper, wg_groups, red_groups, ws, s_per, s_groups,
         s_lds, max_d, slice_chunks, fwd_slices, fwd_split, fwd_red_groups, fwd_ws) = out
        assert (t, kc, max_d, slice_chunks) == (64, 32, MAX_D, 4)
        assert packed == fref.packed_floats(d) if d <= 400 else packed % 4 == 0 and packed >= d * (d - 1) // 2
        assert col_tiles == -(-d // t) and row_tiles == -(-n // t)
        # the forward's k slices: whole chunks of a column tile's k range j < min(D, 64 c + 64) - 1, split where tiles are few
        chunks = [-(-(min(d, t * c + t) - 1) // kc) for c in range(col_tiles)]
        assert fwd_tiles == sum(chunks) and fwd_slices == sum(-(-c // slice_chunks) for c in chunks)
        assert fwd_split == int(col_tiles * row_tiles < 128 and fwd_slices > col_tiles)
        assert fwd_groups == (fwd_slices * row_tiles if fwd_split else col_tiles * row_tiles)
        assert fwd_ws == (fwd_groups * t * t if fwd_split else 0) and fwd_ws < 2 ** 27
        assert fwd_red_groups == (-(-n * d // 256) if fwd_split else 0)
        assert tiles == col_tiles * (col_tiles + 1) // 2
        # the split along N: whole chunks per slice, every sample in exactly one slice, none empty, the workspace holds them
        assert 1 <= slices <= 64 and nper % kc == 0 and (slices - 1) * nper < n <= slices * nper
        assert slices == 1 or (tiles < 128 and nper >= 2 * kc)
        assert wg_groups == tiles * slices
        cells = tiles * t * t + col_tiles * t
        assert ws == (slices * cells if slices > 1 else 0)
        assert red_groups == (-(-cells // 256) if slices > 1 else 0)
        assert s_per in (1, 2, 4) and s_groups == -(-n // s_per) and s_lds == s_per * (-(-d // 4) * 4) * 4 <= 48 * 1024
    # the rectangles: a sample of D over the whole domain, every D up to 200, and the edge
    for d in list(range(1, 201)) + [255, 256, 257, 784, 1000, 3072, 8191, 8192]:
        _, out = _plan(lib, d, 1)
        for kind, want in ((TILES_FWD, out[6]), (TILES_WGRAD, out[7])):
            tiles = ops.fvbn_tiles(d, kind)
            assert len(tiles) == want, (d, kind)
            assert d == 1 or _covered_once(d, tiles), (d, kind)
    assert ops.fvbn_tiles(1, 0) == [] and ops.fvbn_tiles(1, 1) == [(0, 1, 0, 1)]  # D = 1: nothing below the diagonal
    with pytest.raises(ValueError):
        ops.fvbn_tiles(8193, 0)
    assert _plan(lib, 784, 512)[1][8] > 1 and _plan(lib, 3072, 512)[1][8] == 1  # the recipe's step splits, a full triangle does not
    assert lib.pg_fvbn_plan(24, 2, (ctypes.c_longlong * PLAN_INTS)(), PLAN_INTS - 1) == EINVAL  # short array
    assert lib.pg_fvbn_plan(24, 2, None, PLAN_INTS) == EINVAL


def test_launches_refuse_what_the_plan_refuses(lib):
    """Host side only: every argument check comes before the launch, so nothing here touches a device."""
    buf = np.zeros(1 << 10, dtype=np.float32)
    p = (buf.ctypes.data + 255) // 256 * 256
    for d, n in ((0, 4), (8193, 4), (4, 0), (-1, -1)):
        assert lib.pg_fvbn_fwd(p, p, p, p, n, d, p, 1 << 40, None) == ESHAPE
        assert lib.pg_fvbn_wgrad(p, p, p, p, n, d, p, 1 << 40, None) == ESHAPE
        assert lib.pg_fvbn_sample(p, p, p, p, p, n, d, None) == ESHAPE
    for d in (0, 8193):
        assert lib.pg_fvbn_pack(p, p, d, None) == ESHAPE and lib.pg_fvbn_unpack(p, p, d, None) == ESHAPE
    for k in range(4):
        args = [p] * 4
        args[k] = None
        assert lib.pg_fvbn_fwd(*args, 3, 24, None, 0, None) == EINVAL, k
        args = [p] * 5
        args[k] = None
        assert lib.pg_fvbn_sample(*args, 3, 24, None) == EINVAL, k
    for k in range(2):
        args = [p] * 4
        args[k] = None
        assert lib.pg_fvbn_wgrad(*args, 3, 24, p, 1 << 40, None) == EINVAL, k
        args = [p] * 2
        args[k] = None
        assert lib.pg_fvbn_pack(*args, 24, None) == EINVAL and lib.pg_fvbn_unpack(*args, 24, None) == EINVAL
    assert lib.pg_fvbn_fwd(p, p + 4, p, p, 3, 24, None, 0, None) == EINVAL and b"aligned" in lib.pg_last_error()
    assert lib.pg_fvbn_sample(p + 8, p, p, p, p, 3, 24, None) == EINVAL and b"aligned" in lib.pg_last_error()
    rc, out = _plan(lib, 130, 257)
    assert rc == 0 and out[8] > 1 and out[19] == 1
    assert lib.pg_fvbn_fwd(p, p, p, p, 257, 130, p, out[21] - 1, None) == EINVAL  # short workspace of the forward's split
    assert lib.pg_fvbn_fwd(p, p, p, p, 257, 130, None, out[21], None) == EINVAL
    assert lib.pg_fvbn_wgrad(p, p, p, p, 257, 130, p, out[12] - 1, None) == EINVAL  # short workspace
    assert lib.pg_fvbn_wgrad(p, p, p, p, 257, 130, None, out[12], None) == EINVAL
    assert lib.pg_fvbn_wgrad(p, p, None, None, 257, 130, None, 0, None) == 0  # nothing asked for: nothing launched
    count = ctypes.c_longlong(0)
    assert lib.pg_fvbn_tiles(24, 2, None, 0, ctypes.byref(count)) == EINVAL
    assert lib.pg_fvbn_tiles(24, 0, None, 0, None) == EINVAL


# ---------------------------------------------------------------------------------------------
# the float64 restatement against the reference's recorded results
@pytest.mark.parametrize("name", sorted(load_cases()))
def test_closed_form_reproduces_the_fixture(name):
    """fp32 round-off: the reference sums at most 16 terms of order 1 in float32, 50 units in the last place covers it."""
    case = load_cases()[name]
    d = case["kwargs"]["n_dims"]
    n = case["x"].shape[0]
    x = case["x"].reshape(n, -1)
    w, b = fref.state_to_dense(case["state"], d)
    logits = fref.forward(x, w, b)
    tol = 50 * F32
    _close(logits, case["logits"].reshape(n, -1), tol, f"{name} logits")
    loss, g = fref.recipe_loss(x, logits)
    _close(loss, case["loss"], tol, f"{name} loss")
    dw, db = fref.grads(x, g)
    assert not bool(dw[0].any()), "row 0 has no input"
    for i in range(d):
        want_w, want_b = case["grads"][f"_net.{i}.weight"], case["grads"][f"_net.{i}.bias"]
        assert tuple(want_w.shape) == (1, max(1, i)) and tuple(want_b.shape) == (1,)
        assert float((dw[i, :max(1, i)] - want_w[0].double()).abs().max()) <= tol * max(1.0, float(dw.abs().max())), (name, i)
        assert abs(float(db[i] - want_b[0].double())) <= tol * max(1.0, float(db.abs().max())), (name, i)
    assert not bool(case["grads"]["_net.0.weight"].any()), "the reference's dummy weight has an exactly zero gradient"


@pytest.mark.parametrize("name", sorted(load_cases()))
def test_chain_reproduces_the_fixture_sample(name):
    """With every uniform at 0.5 the draw is l > 0, what the reference's sample was recorded under. No logit of that pass is
    within 4e-3 of 0, so rounding decides nothing."""
    case = load_cases()[name]
    d = case["kwargs"]["n_dims"]
    cond = case["conditioned_on"]
    n = cond.shape[0]
    canvas = cond.reshape(n, -1)
    w, b = fref.state_to_dense(case["sample_state"], d)
    got, logits = fref.sample(canvas, w, b, torch.full(canvas.shape, 0.5))
    assert torch.equal(got.float().view(cond.shape), case["sample"])
    assert float(logits.abs().min()) >= 0.9 * 4e-3 and case["sample_margin"] > 4e-3
    given = cond >= 0
    assert cond.dim() == 4 and torch.equal(case["sample"][given], cond[given])


def test_fixture_covers_the_listed_cases():
    cases = load_cases()
    shapes = {(c["kwargs"]["n_dims"], c["x"].shape[0]) for c in cases.values()}
    assert shapes == {(12, 5), (16, 4), (1, 3), (5, 4)}
    assert tuple(cases["d16_n4_img"]["x"].shape) == (4, 1, 4, 4) and tuple(cases["d12_n5"]["x"].shape) == (5, 12)
    real = cases["d5_n4_real"]["x"]
    assert bool(((real != 0) & (real != 1)).any())
    given = [c["conditioned_on"] >= 0 for c in cases.values()]
    assert any(bool(g.any()) and bool((~g).any()) for g in given)
    assert os.path.getsize(FIXTURES) < 300 * 1024


# ---------------------------------------------------------------------------------------------
# the model's host side
@pytest.mark.parametrize("name", sorted(load_cases()))
def test_state_dict_round_trip_is_the_reference(name):
    fvbn = fvbn_mod()
    case = load_cases()[name]
    d = case["kwargs"]["n_dims"]
    for key in ("state", "sample_state"):
        state = case[key]
        model = fvbn.FullyVisibleBeliefNetwork(**case["kwargs"])
        assert [k for k, _ in model.named_parameters()] == ["_weight", "_bias"]
        assert tuple(model._weight.shape) == (fref.packed_floats(d),) and tuple(model._bias.shape) == (d,)
        result = model.load_state_dict(state, strict=True)
        assert not getattr(result, "missing_keys", None) and not getattr(result, "unexpected_keys", None)
        got = model.state_dict()
        assert list(got) == list(state), "keys and their order"
        assert "_weight" not in got and "_bias" not in got
        for k, v in state.items():
            assert got[k].shape == v.shape and got[k].dtype == v.dtype and torch.equal(got[k], v), k
        assert not bool(model._weight.detach()[fref.pad_mask(d)].any()), "pads after loading"
        w, b = fref.state_to_dense(state, d)
        assert torch.equal(model._weight.detach(), fref.pack(w)) and torch.equal(model._bias.detach(), b)
        # a second model loads what the first one saves
        again = fvbn.FullyVisibleBeliefNetwork(**case["kwargs"])
        again.load_state_dict(got, strict=True)
        assert torch.equal(again._weight, model._weight) and torch.equal(again._bias, model._bias)
    assert [k for k in case["state"] if k.startswith("_net")][:2] == ["_net.0.weight", "_net.0.bias"]


def test_state_dict_errors():
    fvbn = fvbn_mod()
    case = load_cases()["d12_n5"]
    model = fvbn.FullyVisibleBeliefNetwork(12)
    before = model._weight.detach().clone()
    missing = {k: v for k, v in case["state"].items() if k != "_net.7.weight"}
    with pytest.raises(RuntimeError, match=r"Missing key.*_net\.7\.weight"):
        model.load_state_dict(missing, strict=True)
    bad = dict(case["state"])
    bad["_net.7.weight"] = torch.zeros(1, 6)
    with pytest.raises(RuntimeError, match=r"size mismatch for _net\.7\.weight"):
        model.load_state_dict(bad, strict=True)
    extra = dict(case["state"], _weight=before)
    with pytest.raises(RuntimeError, match=r"Unexpected key.*_weight"):
        model.load_state_dict(extra, strict=True)
    with pytest.raises(RuntimeError, match="Missing key"):
        model.load_state_dict({"_weight": before, "_bias": model._bias.detach()}, strict=True)
    assert not bool(model._weight.detach()[fref.pad_mask(12)].any())
    # not strict: what is there is loaded, the rest keeps its value
    model = fvbn.FullyVisibleBeliefNetwork(12)
    before = model._weight.detach().clone()
    result = model.load_state_dict(missing, strict=False)
    assert result.missing_keys == ["_net.7.weight"]
    offs = fref.offsets(12)
    assert torch.equal(model._weight.detach()[offs[7]:offs[8]], before[offs[7]:offs[8]])
    assert torch.equal(model._weight.detach()[offs[8]:offs[8] + 8], case["state"]["_net.8.weight"][0])
    # an image batch's recorded shape travels with the state
    img = load_cases()["d16_n4_img"]["state"]
    assert list(img)[:3] == ["_c", "_h", "_w"]
    model = fvbn.FullyVisibleBeliefNetwork(16)
    model.load_state_dict(img, strict=True)
    assert (int(model._c), int(model._h), int(model._w)) == (1, 4, 4)


def test_initialisation_follows_nn_linear():
    """Row i and bias i uniform in +-1/sqrt(max(1, i)): every |w_ij| within the bound; w_ij sqrt(i) over all rows i >= 1 is
    uniform in +-1: mean 0, variance 1/3. 32 640 values at D = 256: the standard error of the mean is 0.003."""
    torch.manual_seed(0)
    d = 256
    model = fvbn_mod().FullyVisibleBeliefNetwork(d)
    weight = model._weight.detach()
    assert not bool(weight[fref.pad_mask(d)].any()), "pads"
    dense = fref.unpack(weight, d)
    bound = torch.arange(d).clamp_min(1).float().rsqrt()
    assert bool((dense.abs() <= bound[:, None]).all()) and bool((model._bias.detach().abs() <= bound).all())
    scaled = torch.cat([dense[i, :i] * i ** 0.5 for i in range(1, d)]).double()
    assert scaled.numel() == 32640
    assert abs(float(scaled.mean())) <= 0.02 and abs(float(scaled.var()) - 1 / 3) <= 0.02
    assert float(scaled.abs().max()) > 0.99
    assert float(dense[0, 0].abs()) <= 1 and float((model._bias.detach() * bound.reciprocal()).abs().max()) > 0.9
    assert inspect.signature(fvbn_mod().FullyVisibleBeliefNetwork.__init__).parameters.keys() == {"self", "n_dims", "sample_fn"}
    assert len(list(model.parameters())) == 2


# ---------------------------------------------------------------------------------------------
# the public surface
def test_alias_serves_the_module_and_the_top_level_name_still_raises():
    import pytorch_generative_amd.compat as compat

    pg = compat.install_alias()
    import pytorch_generative.models as models
    from pytorch_generative.models.autoregressive import fvbn as alias_fvbn

    fvbn = fvbn_mod()
    assert alias_fvbn is fvbn and pg.models.autoregressive.fvbn is fvbn
    assert isinstance(alias_fvbn.FullyVisibleBeliefNetwork(4), fvbn.FullyVisibleBeliefNetwork)
    assert "FullyVisibleBeliefNetwork" not in pg.models.__all__
    with pytest.raises(NotImplementedError):
        models.FullyVisibleBeliefNetwork(4)
    assert "fvbn" in compat.__doc__ and "2 tensors, not 1568" in fvbn.__doc__


def test_exports_and_recipe_table():
    import importlib.util

    from pytorch_generative_amd import ops

    fvbn = fvbn_mod()
    for name in ("fvbn", "fvbn_plan", "fvbn_offsets", "fvbn_pack", "fvbn_unpack", "fvbn_sample_chain"):
        assert callable(getattr(ops, name)), name
    spec = importlib.util.spec_from_file_location(
        "pg_train", os.path.join(os.path.dirname(_util.GOLDEN_DIR), "..", "pytorch-generative_amd", "train.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod.MODEL_DICT["fvbn"] is fvbn
    params = inspect.signature(fvbn.reproduce).parameters
    assert list(params) == ["n_epochs", "batch_size", "log_dir", "n_gpus", "device_id", "debug_loader"]
    assert params["n_epochs"].default == 50 and params["batch_size"].default == 512


def test_sample_signature_and_routes():
    fvbn = fvbn_mod()
    params = inspect.signature(fvbn.FullyVisibleBeliefNetwork.sample).parameters
    assert list(params) == ["self", "n_samples", "conditioned_on", "incremental", "return_logits", "generator"]
    assert all(params[k].kind is inspect.Parameter.KEYWORD_ONLY for k in ("incremental", "return_logits", "generator"))
    model = fvbn.FullyVisibleBeliefNetwork(12)
    assert model._sample_route is None
    assert model._route(5, True) == "chain" and model._route(5, False) == "full"
    assert fvbn.FullyVisibleBeliefNetwork(12, sample_fn=lambda l: (l > 0).float())._route(5, True) == "full"
    assert fvbn.FullyVisibleBeliefNetwork(8193)._route(5, True) == "full"  # outside the plan: the reference's procedure
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

    model = fvbn_mod().FullyVisibleBeliefNetwork(12)
    x = torch.zeros(3, 12)
    with pytest.raises(RuntimeError, match="cuda"):
        ops.fvbn(x, model._weight, model._bias)
    with pytest.raises(ValueError, match="requires_grad"):
        ops.fvbn(x.clone().requires_grad_(True), model._weight, model._bias)
    with pytest.raises(RuntimeError, match="cuda"):
        ops.fvbn_pack(torch.zeros(4, 4))
    with pytest.raises(RuntimeError, match="cuda"):
        ops.fvbn_unpack(model._weight.detach(), 12)
    with pytest.raises(RuntimeError, match="cuda"):
        ops.fvbn_sample_chain(x, model._weight.detach(), model._bias.detach(), x)
    with pytest.raises(RuntimeError, match="cuda"):
        model(x)
    with pytest.raises(RuntimeError, match="cuda"):
        model.sample(conditioned_on=torch.full((3, 12), -1.0))
    assert model._sample_route == "chain"
    with pytest.raises(RuntimeError, match="cuda"):
        model.sample(conditioned_on=torch.full((3, 12), -1.0), incremental=False)
    assert model._sample_route == "full"
