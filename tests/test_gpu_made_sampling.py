"""GPU: the one-launch MADE sampler (csrc/made_sample.hip, ops.made_sample_chain, MADE.sample's "chain" route) — the reference's
recorded samples with every side effect of the old route; logits and samples against the float64 chain of
tests/made_sample_ref.py over tests/made_sample_cases.py (samples EXACT: tests/test_made_sampling_cpu.py shows that no draw
of those inputs is within the logit tolerance of its threshold); bit invariance under batch size, tile slot and repetition;
routing, generators and mask rotation at model level; the draw's frequencies; argument errors."""

import json
import os

import pytest
import torch

import _util
import made_sample_cases as mc
import made_sample_ref as mref

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
FIXTURES = os.path.join(_util.GOLDEN_DIR, "made", "cases.pt")


def made_mod():
    from pytorch_generative_amd.models.autoregressive import made

    return made


def run_chain(net, canvas, uniforms, return_logits=True):
    """ops.made_sample_chain on device copies of CPU operands; returns CPU results (the canvas argument is not touched)."""
    from pytorch_generative_amd import ops

    w1, b1, w2, b2, order = (t.to(DEV) for t in net)
    out = ops.made_sample_chain(canvas.to(DEV), w1, b1, w2, b2, order, uniforms.to(DEV), return_logits=return_logits)
    torch.cuda.synchronize()
    return tuple(t.cpu() for t in out) if return_logits else out.cpu()


def fixed_uniforms(monkeypatch, uniforms):
    """MADE.sample draws its uniforms with torch.rand((n, D), device=..., generator=...): hand it `uniforms` instead."""
    def rand(shape, *, device=None, generator=None):
        assert tuple(shape) == tuple(uniforms.shape)
        return uniforms.to(device)

    monkeypatch.setattr(torch, "rand", rand)


# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["d12_h20_m1", "d16_h20_m3_real"])
def test_fixture_samples_and_side_effects(name, monkeypatch):
    """Uniforms of 0.5 make the draw `l > 0`, the sample_fn the reference recorded its samples under: the operator and the
    model's chain route give them back, and the model leaves behind what the full route leaves."""
    import numpy as np

    made = made_mod()
    case = torch.load(FIXTURES, map_location="cpu", weights_only=False)["cases"][name]
    cond = case["conditioned_on"]
    n = cond.shape[0]
    half = torch.full((n, cond[0].numel()), 0.5)
    kw = case["kwargs"]
    index = case["sample_mask_seed"] % kw["n_masks"]
    conn = made.connectivity(kw["input_dim"], [kw["input_dim"]] + kw["hidden_dims"] + [kw["input_dim"]], index)
    masks = [m.float() for m in made.masks_from_connectivity(conn)]
    st = case["sample_state"]
    net = (st["_net.0.weight"] * masks[0], st["_net.0.bias"], st["_net.2.weight"] * masks[1], st["_net.2.bias"],
           torch.from_numpy(np.argsort(conn[-1]).astype(np.int32)))
    got, _ = run_chain(net, cond.reshape(n, -1), half)
    assert torch.equal(got.view(cond.shape), case["sample"])

    model = made.MADE(**kw)
    model.load_state_dict(st, strict=True)
    model = model.to(DEV)
    model._mask_seed = case["sample_mask_seed"]
    before = [layer.weight.detach().cpu().clone() for layer in model._masked_layers()]
    cond_dev = cond.to(DEV)
    fixed_uniforms(monkeypatch, half)
    got = model.sample(conditioned_on=cond_dev)
    torch.cuda.synchronize()
    assert model._sample_route == "chain"
    assert got.shape == cond.shape and torch.equal(got.cpu(), case["sample"])
    given = cond >= 0
    assert torch.equal(got.cpu()[given], cond[given])
    assert torch.equal(cond_dev.cpu(), case["conditioned_on"]), "conditioned_on must not be modified"
    assert model._mask_seed == case["sample_mask_seed"] + 1
    for layer, w, m in zip(model._masked_layers(), before, masks):
        assert torch.equal(layer.mask.cpu(), m), "mask buffer"
        assert torch.equal(layer.weight.detach().cpu(), w * m), "weight != before * mask"


@pytest.mark.parametrize("case", mc.CASES, ids=mc.case_id)
def test_parity_with_the_float64_chain(case):
    worst = 0.0
    for run in mc.runs(case):
        b = mc.build(*run)
        got, logits = run_chain(b["net"], b["canvas"], b["uniforms"])
        err = _util.rel_err(logits, b["logits"])
        worst = max(worst, err)
        print(f"[made_sampling] {run}: logits rel err {err:.3e}")
        _util.assert_close(logits, b["logits"], mc.LOGIT_TOL, f"{run} logits")
        assert torch.equal(got.double(), b["sample"]), f"{run}: sample differs from the float64 chain"
        if run[3] == "all":
            assert torch.equal(got, b["canvas"]), "a fully given canvas must come back as it went in"
        plain = run_chain(b["net"], b["canvas"], b["uniforms"], return_logits=False)
        assert torch.equal(plain, got), "the sample must not depend on whether logits are asked for"
    path = os.environ.get("PG_PARITY_REPORT")
    if path:
        with open(path, "a") as f:
            f.write(json.dumps({"case": "made_sample " + mc.case_id(case), "worst_logit_rel_err": worst,
                                "tol": mc.LOGIT_TOL}) + "\n")


@pytest.mark.parametrize("n,d,h,rows", [(37, 24, 300, (5, 34)), (9, 24, 4097, (1, 6)), (6, 70, 33, (0, 5))])
def test_rows_do_not_depend_on_the_batch_the_slot_or_the_run(n, d, h, rows):
    net = mc.net(d, h)
    canvas, uniforms = mref.start_canvas(n, d, "some", 1)
    first = run_chain(net, canvas, uniforms)
    again = run_chain(net, canvas, uniforms)
    assert torch.equal(first[0], again[0]) and torch.equal(first[1], again[1]), "two runs differ"
    assert rows[0] // mc.TILE != rows[1] // mc.TILE and rows[0] % mc.TILE != rows[1] % mc.TILE
    for k in rows:
        alone = run_chain(net, canvas[k:k + 1], uniforms[k:k + 1])
        assert torch.equal(alone[0][0], first[0][k]), f"sample row {k} of n = {n} differs from an n = 1 call"
        assert torch.equal(alone[1][0], first[1][k]), f"logits row {k} of n = {n} differ from an n = 1 call"


# ---------------------------------------------------------------------------------------------
def test_model_routes_shapes_and_generator():
    made = made_mod()
    torch.manual_seed(0)
    model = made.MADE(64, [96]).to(DEV)
    got = model.sample(5)
    assert model._sample_route == "chain" and tuple(got.shape) == (5, 64)
    assert bool(((got == 0) | (got == 1)).all())
    model(torch.bernoulli(torch.full((3, 1, 8, 8), 0.3)).to(DEV))
    seed0 = model._mask_seed
    a = model.sample(5, generator=torch.Generator(device=DEV).manual_seed(7))
    b = model.sample(5, generator=torch.Generator(device=DEV).manual_seed(7))
    c = model.sample(5, generator=torch.Generator(device=DEV).manual_seed(8))
    assert tuple(a.shape) == (5, 1, 8, 8) and model._mask_seed == seed0 + 3
    assert torch.equal(a, b) and not torch.equal(a, c)
    # the logits the draws were made from are the network's own on the finished sample (one mask: teacher forcing)
    sample, logits = model.sample(5, return_logits=True)
    assert sample.shape == logits.shape == (5, 1, 8, 8)
    _util.assert_close(logits, model(sample), 1e-4, "chain logits vs forward(sample)")

    model.sample(2, incremental=False)
    assert model._sample_route == "full"
    model.sample(2)
    assert model._sample_route == "chain"
    with pytest.raises(ValueError, match="return_logits"):
        model.sample(2, incremental=False, return_logits=True)
    for kwargs in (dict(hidden_dims=[96], sample_fn=lambda l: (l > 0).float()), dict(hidden_dims=[20, 9, 13]),
                   dict(hidden_dims=None)):
        other = made.MADE(16, **kwargs).to(DEV)
        got = other.sample(conditioned_on=torch.full((2, 16), -1.0, device=DEV))
        assert other._sample_route == "full" and tuple(got.shape) == (2, 16)
    coded = made.MADE(16, [20]).to(DEV)
    coded.input_codes = 4
    with pytest.raises(ValueError, match="input_codes"):
        coded.sample(conditioned_on=torch.full((2, 16), -1.0, device=DEV))


def test_mask_rotation_three_calls_three_indices(monkeypatch):
    """n_masks = 3: successive calls use the masks and the order of indices 0, 1, 2 (on weights the earlier calls have masked
    in place, as successive forwards would), each equal to the float64 chain under that index."""
    import numpy as np

    made = made_mod()
    d, h, n = 16, 20, 6
    torch.manual_seed(4)
    model = made.MADE(d, [h], n_masks=3)
    canvas, _ = mref.start_canvas(n, d, "some", 2)
    w1, b1, w2, b2 = (p.detach().clone() for p in (model._net[0].weight, model._net[0].bias, model._net[2].weight,
                                                   model._net[2].bias))
    model = model.to(DEV)
    all_uniforms = [torch.rand(n, d, generator=torch.Generator().manual_seed(100 + index)) for index in range(3)]
    for index, uniforms in enumerate(all_uniforms):
        conn = made.connectivity(d, [d, h, d], index)
        m1, m2 = (m.float() for m in made.masks_from_connectivity(conn))
        w1, w2 = w1 * m1, w2 * m2
        order = torch.from_numpy(np.argsort(conn[-1]).astype(np.int32))
        want, want_logits = mref.chain(canvas, w1, b1, w2, b2, order, uniforms)
        # the inputs' condition for an exact sample, as in tests/test_made_sampling_cpu.py
        assert mref.draw_margin(canvas, want_logits, uniforms) >= 0.25 * 1e-4 * float(want_logits.abs().max())
        fixed_uniforms(monkeypatch, uniforms)
        got, logits = model.sample(conditioned_on=canvas.to(DEV), return_logits=True)
        assert model._sample_route == "chain" and model._mask_seed == index + 1
        _util.assert_close(logits, want_logits, 1e-4, f"index {index} logits")
        assert torch.equal(got.cpu().double(), want), f"index {index}"
        assert torch.equal(model._net[0].weight.detach().cpu(), w1) and torch.equal(model._net[2].weight.detach().cpu(), w2)


def test_the_draw_uses_its_uniforms():
    """Zero weights: every logit is b2[i], every entry an independent Bernoulli(sigmoid(b2[i])) of its own uniform."""
    n, d, h = 4096, 8, 16
    b2 = torch.tensor([-3.0, -1.5, -0.5, 0.0, 0.25, 1.0, 2.0, 4.0])
    net = (torch.zeros(h, d), torch.zeros(h), torch.zeros(d, h), b2, torch.arange(d - 1, -1, -1, dtype=torch.int32))
    uniforms = torch.rand(n, d, generator=torch.Generator().manual_seed(11))
    got, logits = run_chain(net, torch.full((n, d), -1.0), uniforms)
    assert torch.equal(logits, b2[None, :].expand(n, d))
    p = torch.sigmoid(b2.double())
    # the inputs' condition for the last assertion: an fp32 sigmoid is within 1e-6 of p, no uniform is that close to it
    assert float((uniforms.double() - p[None, :]).abs().min()) > 2e-6
    freq = got.double().mean(0)
    sd = (p * (1 - p) / n).sqrt()
    assert bool(((freq - p).abs() <= 5 * sd).all()), (freq, p, sd)
    assert torch.equal(got, (uniforms.double() < p[None, :]).float()), "entry (n, i) is decided by uniform (n, i)"


def test_argument_errors():
    from pytorch_generative_amd import ops

    d, h, n = 12, 20, 3
    w1, b1, w2, b2, order = (t.to(DEV) for t in mref.masked_net(d, h, seed=0))
    canvas, uniforms = (t.to(DEV) for t in mref.start_canvas(n, d, "some", 0))
    keep = canvas.clone()
    with pytest.raises(ValueError, match="uniforms"):
        ops.made_sample_chain(canvas, w1, b1, w2, b2, order, uniforms[:, :-1].contiguous())
    with pytest.raises(ValueError, match="uniforms"):
        ops.made_sample_chain(canvas, w1, b1, w2, b2, order, uniforms[:-1])
    with pytest.raises(TypeError, match="int32"):
        ops.made_sample_chain(canvas, w1, b1, w2, b2, order.float(), uniforms)
    with pytest.raises(TypeError, match="int32"):
        ops.made_sample_chain(canvas, w1, b1, w2, b2, order.long(), uniforms)
    with pytest.raises(ValueError, match="b1"):
        ops.made_sample_chain(canvas, w1, torch.zeros(h + 1, device=DEV), w2, b2, order, uniforms)
    with pytest.raises(ValueError, match="w2"):
        ops.made_sample_chain(canvas, w1, b1, torch.zeros(d, h + 1, device=DEV), b2, order, uniforms)
    with pytest.raises(ValueError, match="contiguous"):
        ops.made_sample_chain(canvas.t().contiguous().t(), w1, b1, w2, b2, order, uniforms)
    # a shape the plan refuses is an error of the operator, never another route
    big = 8193
    assert ops.made_sample_plan(d, big, n) is None
    with pytest.raises(ValueError, match="hidden units"):
        ops.made_sample_chain(canvas, torch.zeros(big, d, device=DEV), torch.zeros(big, device=DEV),
                              torch.zeros(d, big, device=DEV), b2, order, uniforms)
    torch.cuda.synchronize()
    assert torch.equal(canvas, keep), "a refused call must not touch the canvas"
