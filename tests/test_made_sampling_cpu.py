"""CPU: the one-launch MADE sampler without a device — the float64 chain of tests/made_sample_ref.py reproduces the reference's
recorded samples and agrees with the full masked forward; the inputs of tests/test_gpu_made_sampling.py keep every draw
further from its threshold than the GPU's logit tolerance can move it (which is what lets that test demand exact samples) and
straddle every boundary of the plan; pg_made_sample_plan and the launch agree over a sweep of shapes; the host surface of
ops.made_sample_chain and MADE.sample's routing."""

import ctypes
import inspect
import os
import random

import pytest
import torch

import _util
import made_sample_cases as mc
import made_sample_ref as mref
from test_host_cpu import _fake_ptr, _no_gpu, _reached_launch

FIXTURES = os.path.join(_util.GOLDEN_DIR, "made", "cases.pt")
PLAN_INTS = 8
EINVAL, ESHAPE = -1, -2


def made_mod():
    from pytorch_generative_amd.models.autoregressive import made

    return made


def fixture_net(case):
    """(w1, b1, w2, b2, order) of a fixture's sampling call: its state at that point under the masks of the index in turn."""
    import numpy as np

    made = made_mod()
    kw = case["kwargs"]
    d, (h,) = kw["input_dim"], kw["hidden_dims"]
    conn = made.connectivity(d, [d, h, d], case["sample_mask_seed"] % kw["n_masks"])
    m1, m2 = (m.float() for m in made.masks_from_connectivity(conn))
    st = case["sample_state"]
    order = torch.from_numpy(np.argsort(conn[-1]).astype(np.int32))
    return st["_net.0.weight"] * m1, st["_net.0.bias"], st["_net.2.weight"] * m2, st["_net.2.bias"], order


# ---------------------------------------------------------------------------------------------
# the reference chain
@pytest.mark.parametrize("name,min_logit", [("d12_h20_m1", 1.9e-3), ("d16_h20_m3_real", 1.9e-2)])
def test_chain_reproduces_the_fixture_samples(name, min_logit):
    """With every uniform at 0.5 the draw is `l > 0`, the sample_fn the reference's samples were recorded under: the chain gives
    them back exactly. No drawn entry's logit is near 0 (smallest |l|: 1.9e-3 and 1.9e-2), so rounding decides nothing."""
    case = torch.load(FIXTURES, map_location="cpu", weights_only=False)["cases"][name]
    cond = case["conditioned_on"]
    n = cond.shape[0]
    canvas = cond.reshape(n, -1)
    got, logits = mref.chain(canvas, *fixture_net(case), torch.full(canvas.shape, 0.5))
    assert torch.equal(got.float().view(cond.shape), case["sample"])
    assert torch.equal(cond, case["conditioned_on"])
    smallest = float(logits.abs()[canvas < 0].min())
    print(f"[made_sampling] {name}: smallest |logit| at a drawn entry {smallest:.3e}")
    assert smallest >= 0.9 * min_logit
    # the same through float32 arithmetic: the margin is far above its rounding
    got32, _ = mref.chain(canvas, *fixture_net(case), torch.full(canvas.shape, 0.5), dtype=torch.float32)
    assert torch.equal(got32.view(cond.shape), case["sample"])


SMALL_RUNS = [r for case in mc.CASES if case[1] * case[2] <= 130 * 300 for r in mc.runs(case)]


@pytest.mark.parametrize("run", SMALL_RUNS, ids=lambda r: "n{}-d{}-h{}-{}".format(*r[:4]))
def test_chain_logits_are_the_full_forward_on_the_finished_sample(run):
    """Teacher forcing: logit i of the chain saw exactly the entries that precede i in the order, and the masks hide the rest
    from output i of a full forward — the two agree in float64 to 1e-12, on drawn and on given (also non-binary) entries."""
    b = mc.build(*run)
    full = mref.forward(b["sample"], *b["net"][:4])
    assert float((b["logits"] - full).abs().max()) <= 1e-12 * max(1.0, float(full.abs().max()))
    given = b["canvas"] >= 0
    assert torch.equal(b["sample"][given], b["canvas"].double()[given])
    assert bool(((b["sample"][~given] == 0) | (b["sample"][~given] == 1)).all())


def test_chain_follows_the_order_of_each_mask_index():
    """Another mask index: another order and other masks; the chain under index k is the forward under index k and not under j."""
    n, d, h = 3, 11, 17
    canvas, u = mref.start_canvas(n, d, "some", 5)
    nets = [mref.masked_net(d, h, seed=3, mask_index=k) for k in range(3)]
    assert len({tuple(net[4].tolist()) for net in nets}) == 3
    for k, net in enumerate(nets):
        sample, logits = mref.chain(canvas, *net, u)
        assert float((logits - mref.forward(sample, *net[:4])).abs().max()) <= 1e-12
        other = nets[(k + 1) % 3]
        assert float((logits - mref.forward(sample, *other[:4])).abs().max()) > 1e-3


# ---------------------------------------------------------------------------------------------
# the inputs of the GPU test
@pytest.mark.parametrize("case", mc.CASES, ids=mc.case_id)
def test_no_draw_of_the_gpu_cases_is_within_the_logit_tolerance_of_its_threshold(case):
    """The GPU logits are held to max |dl| <= LOGIT_TOL * max |l|; the sigmoid's slope is at most 1 / 4, so p moves by at most
    0.25 * LOGIT_TOL * max |l|. No drawn entry of any run has |u - p| below that: a kernel inside the logit bound draws exactly
    the float64 chain's sample. A condition on the inputs (the seeds of made_sample_cases are picked for it), not a measurement."""
    for run in mc.runs(case):
        b = mc.build(*run)
        need = 0.25 * mc.LOGIT_TOL * float(b["logits"].abs().max())
        margin = mref.draw_margin(b["canvas"], b["logits"], b["uniforms"])
        print(f"[made_sampling] {run}: margin {margin:.3e}, needed {need:.3e}")
        assert margin >= need, (run, margin, need)
        if run[3] == "all":
            assert torch.equal(b["sample"], b["canvas"].double())
        if run[3] == "none":
            assert bool((b["canvas"] < 0).all())


def _plan(lib, d, h, n):
    out = (ctypes.c_int * PLAN_INTS)()
    return lib.pg_made_sample_plan(d, h, n, out, PLAN_INTS), list(out)


def test_the_gpu_cases_straddle_every_boundary_of_the_plan(lib):
    """Where (threads per workgroup, hidden units per thread) changes along H, the tile size, the end of the domain: read from the
    plan, and each side of each is a case."""
    classes = [tuple(_plan(lib, 24, h, 2)[1][1:3]) for h in range(1, mc.MAX_H + 1)]
    boundaries = tuple(h for h in range(1, mc.MAX_H) if classes[h - 1] != classes[h])
    assert boundaries == mc.H_BOUNDARIES
    rc, out = _plan(lib, 24, 64, 2)
    assert rc == 0 and out[0] == mc.TILE and out[7] == mc.MAX_H
    assert _plan(lib, 24, mc.MAX_H, 2)[0] == 0 and _plan(lib, 24, mc.MAX_H + 1, 2)[0] == ESHAPE
    hs = {case[2] for case in mc.CASES}
    ns = {case[0] for case in mc.CASES}
    for b in boundaries:
        assert {b, b + 1} <= hs, b
    assert mc.MAX_H in hs and {mc.TILE - 1, mc.TILE, mc.TILE + 1} <= ns
    assert any(case[0] > 2 * mc.TILE for case in mc.CASES)
    assert (2, 784, 8000) in {case[:3] for case in mc.CASES}


# ---------------------------------------------------------------------------------------------
# planner
def _sweep(seed=0, count=4000):
    rng = random.Random(seed)
    edge_h = [1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097, 8000, 8191, 8192, 8193, 10000, 20000]
    shapes = [(d, h, n) for d in (1, 2, 784, 2000) for h in edge_h for n in (1, 3, 4, 5, 5000)]
    shapes += [(rng.randint(1, 2000), rng.randint(1, 20000), rng.randint(1, 5000)) for _ in range(count)]
    return shapes


def test_plan_domain_and_geometry(lib):
    """Every H <= 8192 of the sweep is accepted and every larger one refused; the geometry stays inside the device's limits
    and is consistent with itself."""
    for d, h, n in _sweep():
        rc, out = _plan(lib, d, h, n)
        assert rc == (0 if h <= 8192 else ESHAPE), (d, h, n, rc)
        if rc:
            continue
        tile, threads, units, lds, pack, row, groups, max_h = out
        assert tile == mc.TILE and max_h == 8192
        assert threads % 64 == 0 and 64 <= threads <= 1024 and units in (1, 4, 8)
        assert row == threads * units and h <= row and row % 64 == 0
        assert tile * units <= 32, "the hidden sums of a tile must fit a thread's registers"
        assert 0 < lds <= 64 * 1024 and lds >= 2 * tile * (threads // 64) * 4
        assert pack == 2 * d * row and groups == (n + tile - 1) // tile
    # a pack of 2^31 floats or more is refused, from the size on where it happens
    assert _plan(lib, (1 << 31) // (2 * 8192) - 1, 8192, 1)[0] == 0
    assert _plan(lib, (1 << 31) // (2 * 8192), 8192, 1)[0] == ESHAPE
    assert b"too large" in lib.pg_last_error()
    assert lib.pg_made_sample_plan(24, 20, 2, (ctypes.c_int * PLAN_INTS)(), PLAN_INTS - 1) == EINVAL  # short array
    assert lib.pg_made_sample_plan(24, 20, 2, None, PLAN_INTS) == EINVAL
    for bad in ((0, 20, 2), (24, 0, 2), (24, 20, 0), (-1, 20, 2), (24, -5, 2), (24, 20, -3)):
        assert _plan(lib, *bad)[0] == EINVAL, bad


@_no_gpu
def test_what_the_plan_accepts_reaches_the_launch(lib):
    """Fake operands, no device: a launch entry that got past its host side comes back with hipErrorNoDevice. Over the sweep the
    pack and the chain get that far exactly where the plan accepts, and refuse with the plan's status where it refuses."""
    keep, ptr = _fake_ptr()
    p = ptr.value
    for d, h, n in _sweep(seed=1, count=1500):
        rc_plan, _ = _plan(lib, d, h, n)
        rc = lib.pg_made_sample(p, p, p, p, p, p, p, n, d, h, None)
        rc_pack = lib.pg_made_sample_pack(p, p, p, d, h, None)
        if rc_plan == 0:
            assert _reached_launch(lib, rc_pack), (d, h, n, rc_pack, lib.pg_last_error())
            rc = lib.pg_made_sample(p, p, p, p, p, p, None, n, d, h, None)  # logits_out is optional
            assert _reached_launch(lib, rc), (d, h, n, rc, lib.pg_last_error())
        else:
            assert rc == rc_pack == rc_plan == ESHAPE, (d, h, n, rc, rc_pack, rc_plan)
    big = (1 << 31) // (2 * 8192)
    assert lib.pg_made_sample(p, p, p, p, p, p, p, 1, big, 8192, None) == ESHAPE
    assert lib.pg_made_sample_pack(p, p, p, big, 8192, None) == ESHAPE
    # argument errors launch nothing either
    for k in range(6):  # every operand but logits_out
        args = [p] * 7
        args[k] = None
        assert lib.pg_made_sample(*args, 2, 24, 20, None) == EINVAL, k
    assert lib.pg_made_sample(p + 4, p, p, p, p, p, p, 2, 24, 20, None) == EINVAL  # the pack's alignment
    for k in range(3):
        args = [p] * 3
        args[k] = None
        assert lib.pg_made_sample_pack(*args, 24, 20, None) == EINVAL, k
    for n, d, h in ((0, 24, 20), (2, 0, 20), (2, 24, 0), (-1, 24, 20)):
        assert lib.pg_made_sample(p, p, p, p, p, p, p, n, d, h, None) == EINVAL
    assert lib.pg_made_sample_pack(p, p, p, 0, 20, None) == EINVAL
    assert lib.pg_made_sample_pack(p, p, p, 24, -1, None) == EINVAL


# ---------------------------------------------------------------------------------------------
# host surface
def test_cpu_tensors_raise():
    from pytorch_generative_amd import ops

    w1, b1, w2, b2, order = mref.masked_net(12, 20, seed=0)
    canvas, u = mref.start_canvas(3, 12, "some", 0)
    with pytest.raises(RuntimeError, match="cuda"):
        ops.made_sample_chain(canvas, w1, b1, w2, b2, order, u)
    model = made_mod().MADE(12, [20])
    with pytest.raises(RuntimeError, match="cuda"):
        model.sample(conditioned_on=canvas)
    assert model._sample_route == "chain"
    with pytest.raises(RuntimeError, match="cuda"):
        model.sample(conditioned_on=canvas, incremental=False)
    assert model._sample_route == "full"


def test_plan_query_of_the_operator_layer():
    from pytorch_generative_amd import ops

    plan = ops.made_sample_plan(784, 8000, 16)
    assert plan == {"samples_per_workgroup": 4, "threads": 1024, "units_per_thread": 8, "lds_bytes": 512,
                    "pack_floats": 2 * 784 * 8192, "row_floats": 8192, "workgroups": 4, "max_hidden": 8192}
    assert ops.made_sample_plan(784, 8193, 16) is None
    assert ops.made_sample_plan(12, 20, 1)["threads"] == 64


def test_sample_signature_and_routes():
    made = made_mod()
    params = inspect.signature(made.MADE.sample).parameters
    assert list(params) == ["self", "n_samples", "conditioned_on", "incremental", "return_logits", "generator"]
    assert all(params[k].kind is inspect.Parameter.KEYWORD_ONLY for k in ("incremental", "return_logits", "generator"))
    assert params["incremental"].default is True and params["return_logits"].default is False
    one = made.MADE(12, [20])
    assert one._sample_route is None
    assert one._route(5, True) == "chain" and one._route(5, False) == "full"
    assert made.MADE(784, [8000])._route(16, True) == "chain"
    assert made.MADE(12, [20], sample_fn=lambda l: (l > 0).float())._route(5, True) == "full"
    assert made.MADE(12, None)._route(5, True) == "full"
    assert made.MADE(16, [20, 9, 13])._route(5, True) == "full"
    assert made.MADE(12, [8193])._route(5, True) == "full"  # outside the plan: the reference's procedure, not an error
    # the full route has no logits to return; said before any device work
    with pytest.raises(ValueError, match="return_logits"):
        made.MADE(12, None).sample(conditioned_on=torch.full((2, 12), -1.0), return_logits=True)
    # no recorded image shape: vectors
    assert tuple(one._start_canvas(5, None).shape) == (5, 12)
    cond = torch.full((2, 1, 3, 4), -1.0)
    assert one._start_canvas(None, cond).shape == cond.shape and one._start_canvas(None, cond) is not cond
