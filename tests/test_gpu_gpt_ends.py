"""GPU: the four kernels of csrc/gpt_ends.hip (ImageGPT's stem and output head) and the merged reduce, against torch on the
CPU in float64: F.conv2d of img + pos with weight * mask, F.layer_norm over the channels, F.conv2d 1x1, gradients by autograd
with respect to the masked weight (all nine taps get one). Kernel-level cases go through the C-ABI with an explicit grid_cap;
the model-level cases run ImageGPT(in_size=8, 2 blocks, 4 heads, 16 channels) at N = 3 against the float64 oracle.
Tolerances are the project's (tests/_util.py)."""

import ctypes
import functools

import pytest
import torch
import torch.nn.functional as F

import _util

pytestmark = pytest.mark.gpu

TOL = 1e-4
EPS = 1e-5
# (N, H, W): every tap out of range | no row above | no column to the left | small | L = 35: scalar stores, ragged tile
SMALL = [(1, 1, 1), (2, 1, 5), (2, 5, 1), (3, 4, 4), (2, 5, 7)]
CASES = [(s, 0) for s in SMALL] + [((5, 28, 28), cap) for cap in (1, 2, 3, 0)]  # a workgroup walks many tiles, crosses images


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need the MI355X"
    from pytorch_generative_amd import _lib

    _lib.load()
    return torch.device("cuda:0")


def _rand(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def _mask():
    m = torch.zeros(16, 1, 3, 3)
    m[:, :, 0, :] = 1.0
    m[:, :, 1, 0] = 1.0
    return m


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _ptrs(ts):
    return (ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts])


# ------------------------------------------------------------------------------------------- float64 references (computed once)
@functools.lru_cache(maxsize=None)
def stem_case(n, h, w):
    img, pos, dx0 = (_rand(n, 1, h, w, seed=1) > 0).float(), 0.3 * _rand(1, 1, h, w, seed=2), _rand(n, 16, h, w, seed=3)
    weight, bias = 0.4 * _rand(16, 1, 3, 3, seed=4), 0.2 * _rand(16, seed=5)
    wm = (weight * _mask()).double().requires_grad_(True)
    b64, p64 = bias.double().requires_grad_(True), pos.double().requires_grad_(True)
    x0 = F.conv2d(img.double() + p64, wm, b64, padding=1)
    (x0 * dx0.double()).sum().backward()
    return dict(img=img, pos=pos, dx0=dx0, weight=weight, bias=bias, x0=x0.detach(), dw=wm.grad, db=b64.grad, dpos=p64.grad)


@functools.lru_cache(maxsize=None)
def head_case(n, h, w, cout, flat_pixel=False):
    x, dl = _rand(n, 16, h, w, seed=6), _rand(n, cout, h, w, seed=7)
    if flat_pixel:
        x[0, :, 0, 0] = 0.75  # one pixel whose 16 channels are equal: variance 0
    P = dict(lnw=1 + 0.3 * _rand(16, seed=8), lnb=0.2 * _rand(16, seed=9), cw=0.4 * _rand(cout, 16, 1, 1, seed=10),
             cb=0.2 * _rand(cout, seed=11))
    P64 = {k: v.double().requires_grad_(True) for k, v in P.items()}
    x64 = x.double().requires_grad_(True)
    y = F.layer_norm(x64.permute(0, 2, 3, 1), (16,), P64["lnw"], P64["lnb"], EPS).permute(0, 3, 1, 2)
    logits = F.conv2d(y, P64["cw"], P64["cb"])
    (logits * dl.double()).sum().backward()
    return dict(x=x, dl=dl, logits=logits.detach(), dx=x64.grad, grads={k: v.grad for k, v in P64.items()}, **P)


# ------------------------------------------------------------------------------------------- the kernels through the C-ABI
def run_stem_fwd(dev, c, cap):
    from pytorch_generative_amd import _lib

    lib = _lib.load()
    n, _, h, w = c["img"].shape
    img, pos, weight, bias = (c[k].to(dev) for k in ("img", "pos", "weight", "bias"))
    x0 = torch.full((n, 16, h, w), float("nan"), device=dev)
    _lib.check(lib.pg_gpt_stem_fwd(img.data_ptr(), pos.data_ptr(), weight.data_ptr(), bias.data_ptr(), x0.data_ptr(), n, h, w,
                                   cap, _stream()), "pg_gpt_stem_fwd")
    return x0, weight


def run_stem_bwd(dev, c, cap, fill=0.0):
    """(d weight, d bias, d pos), added to destinations pre-filled with `fill`"""
    from pytorch_generative_amd import _lib

    lib = _lib.load()
    n, _, h, w = c["img"].shape
    img, pos, dx0 = (c[k].to(dev) for k in ("img", "pos", "dx0"))
    weight = (c["weight"] * _mask()).to(dev)
    rows, slices = ctypes.c_int(0), ctypes.c_int(0)
    _lib.check(lib.pg_gpt_stem_bwd_plan(n, h, w, cap, ctypes.byref(rows), ctypes.byref(slices)), "plan")
    if cap:
        assert rows.value <= cap
    ws_n = lib.pg_gpt_stem_bwd_workspace_floats(n, h, w, cap)
    ws = torch.full((ws_n,), float("nan"), device=dev)  # every float the reduce reads must have been written
    _lib.check(lib.pg_gpt_stem_bwd(dx0.data_ptr(), img.data_ptr(), pos.data_ptr(), weight.data_ptr(), n, h, w, cap,
                                   ws.data_ptr(), ws_n, _stream()), "pg_gpt_stem_bwd")
    out = [torch.full(s, fill, device=dev) for s in ((16, 1, 3, 3), (16,), (1, 1, h, w))]
    _lib.check(lib.pg_gpt_model_reduce(0, None, None, None, n, 16, h * w, 0, 0, 0, None, ws.data_ptr(), rows.value,
                                       slices.value, h, w, _ptrs(out), _stream()), "pg_gpt_model_reduce")
    return out


def run_head_fwd(dev, c, cap):
    from pytorch_generative_amd import _lib

    lib = _lib.load()
    n, _, h, w = c["x"].shape
    cout = c["cw"].shape[0]
    x, lnw, lnb, cw, cb = (c[k].to(dev) for k in ("x", "lnw", "lnb", "cw", "cb"))
    logits = torch.full((n, cout, h, w), float("nan"), device=dev)
    _lib.check(lib.pg_gpt_out_head_fwd(x.data_ptr(), lnw.data_ptr(), lnb.data_ptr(), cw.data_ptr(), cb.data_ptr(),
                                       logits.data_ptr(), n, 16, cout, h * w, EPS, cap, _stream()), "pg_gpt_out_head_fwd")
    return logits


def run_head_bwd(dev, c, cap, fill=0.0):
    """dx and {name: gradient}, added to destinations pre-filled with `fill`"""
    from pytorch_generative_amd import _lib

    lib = _lib.load()
    n, _, h, w = c["x"].shape
    cout, L = c["cw"].shape[0], h * w
    x, lnw, lnb, cw, dl = (c[k].to(dev) for k in ("x", "lnw", "lnb", "cw", "dl"))
    rows = lib.pg_gpt_out_head_bwd_rows(n, L, cap)
    if cap:
        assert rows <= cap
    ws = torch.full((rows * (32 + 17 * cout),), float("nan"), device=dev)
    dx = torch.full((n, 16, h, w), float("nan"), device=dev)
    _lib.check(lib.pg_gpt_out_head_bwd(x.data_ptr(), lnw.data_ptr(), lnb.data_ptr(), cw.data_ptr(), dl.data_ptr(),
                                       dx.data_ptr(), n, 16, cout, L, EPS, cap, ws.data_ptr(), ws.numel(), _stream()),
               "pg_gpt_out_head_bwd")
    out = [torch.full(s, fill, device=dev) for s in ((16,), (16,), (cout, 16, 1, 1), (cout,))]
    _lib.check(lib.pg_gpt_model_reduce(0, None, None, None, n, 16, L, ws.data_ptr(), rows, cout, _ptrs(out), 0, 0, 0, 0, 0,
                                       None, _stream()), "pg_gpt_model_reduce")
    return dx, dict(zip(("lnw", "lnb", "cw", "cb"), out))


def _case_id(v):
    return "x".join(map(str, v)) if isinstance(v, tuple) else f"cap{v}"


# ------------------------------------------------------------------------------------------- 1. shapes
@pytest.mark.parametrize("shape,cap", CASES, ids=_case_id)
def test_stem_forward_and_backward_match_float64(dev, shape, cap):
    c = stem_case(*shape)
    x0, _ = run_stem_fwd(dev, c, cap)
    if shape == (1, 1, 1):  # every tap out of range: the output is the bias
        assert torch.equal(x0.cpu().flatten(), c["bias"])
    _util.assert_close(x0, c["x0"], TOL, "stem x0")
    dw, db, dpos = run_stem_bwd(dev, c, cap)
    rep = _util.GradReport(f"gpt stem {shape} cap {cap}")
    if float(c["dw"].abs().max()) > 0:  # (1, 1, 1): the only tap inside the image is the masked centre one
        rep.add("d weight", dw, c["dw"])
    rep.add("d bias", db, c["db"])
    if float(c["dpos"].abs().max()) > 0:
        rep.add("d pos", dpos, c["dpos"])
    else:
        assert not dpos.any()
    rep.finish()


def _check_head(dev, shape, cap, cout):
    c = head_case(*shape, cout)
    _util.assert_close(run_head_fwd(dev, c, cap), c["logits"], TOL, "head logits")
    dx, grads = run_head_bwd(dev, c, cap)
    rep = _util.GradReport(f"gpt out head {shape} cap {cap} cout {cout}")
    rep.add("dx", dx, c["dx"])
    for k, g in grads.items():
        rep.add("d " + k, g, c["grads"][k])
    rep.finish()


@pytest.mark.parametrize("shape,cap", CASES, ids=_case_id)
def test_head_forward_and_backward_match_float64(dev, shape, cap):
    _check_head(dev, shape, cap, 1)


@pytest.mark.parametrize("shape,cap,cout", [((2, 5, 7), 0, 2), ((5, 28, 28), 3, 3), ((3, 4, 4), 0, 4)], ids=_case_id)
def test_head_with_more_output_channels(dev, shape, cap, cout):
    _check_head(dev, shape, cap, cout)


# ------------------------------------------------------------------------------------------- 2. variance 0
def test_head_pixel_with_equal_channels(dev):
    c = head_case(2, 3, 4, 1, True)
    logits = run_head_fwd(dev, c, 0)
    dx, grads = run_head_bwd(dev, c, 0)
    assert torch.isfinite(logits).all() and torch.isfinite(dx).all() and all(torch.isfinite(g).all() for g in grads.values())
    _util.assert_close(logits, c["logits"], TOL, "logits")
    rep = _util.GradReport("gpt out head, variance 0")
    rep.add("dx", dx, c["dx"])
    rep.add("dx of the flat pixel", dx[0, :, 0, 0], c["dx"][0, :, 0, 0])
    for k, g in grads.items():
        rep.add("d " + k, g, c["grads"][k])
    rep.finish()


# ------------------------------------------------------------------------------------------- 3. masking
def test_stem_forward_masks_the_weight_in_place(dev):
    c = stem_case(3, 4, 4)
    m = _mask().bool()
    assert (c["weight"][~m] != 0).all()
    _, weight = run_stem_fwd(dev, c, 0)
    weight = weight.cpu()
    assert not weight[~m].any(), "masked entries must be exactly 0 after a forward"
    assert torch.equal(weight[m], c["weight"][m]), "unmasked entries must be untouched"
    assert torch.equal(weight * _mask(), weight)


def test_stem_weight_gradient_covers_the_masked_taps(dev):
    c = stem_case(3, 4, 4)
    dw, _, _ = run_stem_bwd(dev, c, 0)
    m = _mask().bool()
    want = c["dw"][~m]
    assert float(want.abs().min()) > 0
    rep = _util.GradReport("gpt stem, masked taps")
    rep.add("d weight[masked]", dw.cpu()[~m], want)
    rep.finish()


# ------------------------------------------------------------------------------------------- 4. reductions
@pytest.mark.parametrize("cap", [0, 3])
def test_reductions_are_deterministic(dev, cap):
    cs, ch = stem_case(5, 28, 28), head_case(5, 28, 28, 1)
    a, b = run_stem_bwd(dev, cs, cap), run_stem_bwd(dev, cs, cap)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    (dxa, ga), (dxb, gb) = run_head_bwd(dev, ch, cap), run_head_bwd(dev, ch, cap)
    assert torch.equal(dxa, dxb) and all(torch.equal(ga[k], gb[k]) for k in ga)


def test_gradients_agree_across_grids(dev):
    cs, ch = stem_case(5, 28, 28), head_case(5, 28, 28, 1)
    rep = _util.GradReport("gpt ends, grid_cap 1 against 3")
    for name, x, y in zip(("d weight", "d bias", "d pos"), run_stem_bwd(dev, cs, 1), run_stem_bwd(dev, cs, 3)):
        rep.add(name, x, y)
    (_, g1), (_, g3) = run_head_bwd(dev, ch, 1), run_head_bwd(dev, ch, 3)
    for k in g1:
        rep.add("head d " + k, g1[k], g3[k])
    rep.finish()


def _end_modules(dev, c_stem, c_head):
    from pytorch_generative_amd import nn as pg_nn

    conv = pg_nn.CausalConv2d(True, in_channels=1, out_channels=16, kernel_size=3, padding=1).to(dev)
    ln, out = pg_nn.NCHWLayerNorm(16).to(dev), pg_nn.Conv2d(in_channels=16, out_channels=1, kernel_size=1).to(dev)
    pos = torch.nn.Parameter(c_stem["pos"].to(dev))
    with torch.no_grad():
        conv.weight.copy_(c_stem["weight"]); conv.bias.copy_(c_stem["bias"])
        ln.weight.copy_(c_head["lnw"]); ln.bias.copy_(c_head["lnb"])
        out.weight.copy_(c_head["cw"]); out.bias.copy_(c_head["cb"])
    return conv, pos, ln, out


@pytest.mark.parametrize("with_sink", [False, True])
def test_ops_add_into_a_sink_or_return_the_gradient(dev, with_sink):
    """Through the autograd Functions: with a `_pg_grad` sink (pre-filled with 0.25: the kernels add) autograd gets None and the
    sink holds 0.25 + gradient; without one the gradient arrives in .grad. Both match the float64 reference."""
    from pytorch_generative_amd import ops

    cs, ch = stem_case(3, 4, 4), head_case(3, 4, 4, 1)
    conv, pos, ln, out = _end_modules(dev, cs, ch)
    params = dict(pos=pos, weight=conv.weight, bias=conv.bias, lnw=ln.weight, lnb=ln.bias, cw=out.weight, cb=out.bias)
    fill = 0.25 if with_sink else 0.0
    if with_sink:
        for p in params.values():
            p._pg_grad = torch.full_like(p, fill)
    assert ops.gpt_stem_supported(cs["img"].to(dev), pos, conv) and ops.gpt_out_head_supported(ch["x"].to(dev), ln, out)
    x0 = ops.gpt_stem(cs["img"].to(dev), pos, conv)
    x0.backward(cs["dx0"].to(dev))
    x = ch["x"].to(dev).requires_grad_(True)
    logits = ops.gpt_out_head(x, ln, out)
    logits.backward(ch["dl"].to(dev))
    _util.assert_close(x0, cs["x0"], TOL, "x0")
    _util.assert_close(logits, ch["logits"], TOL, "logits")
    want = dict(pos=cs["dpos"], weight=cs["dw"], bias=cs["db"], **ch["grads"])
    rep = _util.GradReport(f"gpt ends ops, sink={with_sink}")
    rep.add("dx", x.grad, ch["dx"])
    for k, p in params.items():
        if with_sink:
            assert p.grad is None, k
            rep.add(k, p._pg_grad, want[k] + fill)
        else:
            rep.add(k, p.grad, want[k])
    rep.finish()


# ------------------------------------------------------------------------------------------- model level
N_HEADS = 4


@pytest.fixture(scope="module")
def model_case():
    """Parameters, input, output gradient and the float64 oracle's logits and gradients — computed once, never changed."""
    from oracle import models as omodels
    from pytorch_generative_amd.models.autoregressive import image_gpt

    torch.manual_seed(0)
    model = image_gpt.ImageGPT(in_channels=1, out_channels=1, in_size=8, n_transformer_blocks=2, n_attention_heads=N_HEADS,
                               n_embedding_channels=16)
    with torch.no_grad():
        for p in model.parameters():
            p.add_(0.05 * torch.randn_like(p))
    state = {k: v.detach().clone() for k, v in model.state_dict().items()}
    x, dy = (_rand(3, 1, 8, 8, seed=20) > 0).float(), _rand(3, 1, 8, 8, seed=21)
    s64 = omodels.apply_masks_({k: v.double().clone() for k, v in state.items()})
    leaves = {k: v.requires_grad_(True) for k, v in s64.items() if not k.endswith(".mask")}
    logits = omodels.image_gpt({**s64, **leaves}, x.double(), n_heads=N_HEADS)
    (logits * dy.double()).sum().backward()
    return dict(state=state, x=x, dy=dy, logits=logits.detach(), grads={k: v.grad for k, v in leaves.items()})


def _model(dev, case):
    from pytorch_generative_amd.models.autoregressive import image_gpt

    model = image_gpt.ImageGPT(in_channels=1, out_channels=1, in_size=8, n_transformer_blocks=2, n_attention_heads=N_HEADS,
                               n_embedding_channels=16)
    model.load_state_dict(case["state"])
    return model.to(dev)


def test_model_with_fused_ends_matches_the_float64_oracle(dev, model_case):
    from pytorch_generative_amd import ops

    assert ops.FUSE_ENDS, "PG_FUSE_ENDS=0 selects the generic operators; this test is about the fused ends"
    model = _model(dev, model_case)
    logits = model(model_case["x"].to(dev))
    assert type(logits.grad_fn).__name__.startswith("_GPTOutHead"), "the model did not take the fused output head"
    logits.backward(model_case["dy"].to(dev))
    _util.assert_close(logits, model_case["logits"], TOL, "logits")
    assert torch.equal(model._input.weight * model._input.mask, model._input.weight)
    rep = _util.GradReport("ImageGPT 8x8, fused ends, plain autograd")
    for k, p in model.named_parameters():
        assert p.grad is not None, k
        rep.add(k, p.grad, model_case["grads"][k])
    rep.finish()


@pytest.mark.parametrize("freeze_first_block", [False, True])
def test_flat_adam_step_with_the_chain(dev, model_case, freeze_first_block):
    """One FlatAdam step: the stem's backward flushes the blocks' and both ends' rows in one launch. With the first block frozen
    (FlatAdam over the rest) its kernels reduce their own rows and the others still arrive: step() must not raise."""
    from pytorch_generative_amd import ops, optim

    model = _model(dev, model_case)
    if freeze_first_block:
        for p in model._transformer[0].parameters():
            p.requires_grad_(False)
    trainable = {k: p for k, p in model.named_parameters() if p.requires_grad}
    opt = optim.FlatAdam(trainable.values(), lr=1e-3)
    opt.zero_grad()
    logits = model(model_case["x"].to(dev))
    logits.backward(model_case["dy"].to(dev))
    ops.assert_no_pending_block_reductions()
    _util.assert_close(logits, model_case["logits"], TOL, "logits")
    rep = _util.GradReport(f"ImageGPT 8x8, FlatAdam, frozen first block={freeze_first_block}")
    for k, p in trainable.items():
        assert p._pg_grad is not None and p._pg_grad.data_ptr() >= opt.flat_grad.data_ptr(), k
        rep.add(k, p._pg_grad, model_case["grads"][k])
    rep.finish()
    before = opt.flat_param.clone()
    opt.step()
    ops.assert_no_pending_block_reductions()
    assert torch.isfinite(opt.flat_param).all() and not torch.equal(before, opt.flat_param)
