"""GPU: LinearCausalAttention on the chunked-scan kernels (csrc/linear_attention.hip) — output and every gradient
against the reference's own fp32 results (tests/golden/linear_attention/cases.pt) and against a float64 closed form at
larger shapes; causality, run-to-run bit reproducibility, hipGraph replay, the custom-feature path, the FlatAdam
gradient sinks and the O(L) memory footprint."""

import pytest
import torch
import torch.nn.functional as F

import _util
from test_linear_attention_cpu import FEATURES, _dims, add_grads, closed_form, load_cases

pytestmark = pytest.mark.gpu

TOL = 1e-4


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need the MI355X"
    from pytorch_generative_amd import _lib

    _lib.load()
    return torch.device("cuda:0")


def _rand(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def _module(kwargs, feature, dev, state=None, seed=0):
    from pytorch_generative_amd import nn as pg_nn

    torch.manual_seed(seed)
    extra = {} if feature == "default" else {"feature_fn": FEATURES[feature]}
    mod = pg_nn.LinearCausalAttention(**kwargs, **extra)
    if state is not None:
        mod.load_state_dict(state, strict=True)
    return mod.to(dev)


def _fwd_bwd(mod, x, g):
    x = x.clone().requires_grad_(True)
    for p in mod.parameters():
        p.grad = None
    y = mod(x)
    (y * g).sum().backward()
    torch.cuda.synchronize()
    return y.detach(), {"x": x.grad, **{k: p.grad for k, p in mod.named_parameters()}}


@pytest.mark.parametrize("name", sorted(load_cases()))
def test_matches_reference_fixture(dev, name):
    case = load_cases()[name]
    mod = _module(case["kwargs"], case["feature"], dev, case["state"])
    y, grads = _fwd_bwd(mod, case["x"].to(dev), case["g"].to(dev))
    _util.assert_close(y, case["y"], TOL, f"{name} y")
    rep = _util.GradReport(f"linear attention {name}")
    add_grads(rep, case, grads)
    rep.finish()


@pytest.mark.parametrize("n,c,heads,embed,out,h,w", [(2, 32, 4, 32, 32, 64, 64), (1, 16, 1, 64, 64, 64, 64),
                                                     (2, 16, 4, 20, 44, 37, 29)],
                         ids=["h4_d8_64x64", "h1_d64_64x64", "h4_dk5_dv11_37x29"])
def test_matches_float64_closed_form(dev, n, c, heads, embed, out, h, w):
    kwargs = dict(in_channels=c, n_heads=heads, embed_channels=embed, out_channels=out)
    mod = _module(kwargs, "default", dev, seed=3)
    x, g = _rand(n, c, h, w, seed=1), _rand(n, out, h, w, seed=2)
    y, grads = _fwd_bwd(mod, x.to(dev), g.to(dev))
    state = {k: v.detach().cpu().double().requires_grad_(True) for k, v in mod.state_dict().items()}
    x64 = x.double().requires_grad_(True)
    want = closed_form(state, x64, heads, embed, out, FEATURES["default"])
    (want * g.double()).sum().backward()
    _util.assert_close(y, want, TOL, "y")
    case = {"kwargs": kwargs, "grads": {"x": x64.grad, **{k: p.grad for k, p in state.items()}}}
    rep = _util.GradReport(f"linear attention vs float64 {n}x{c}x{h}x{w} heads {heads}")
    add_grads(rep, case, grads)
    rep.finish()


def test_causal_perturbing_a_pixel_leaves_earlier_outputs_bit_identical(dev):
    mod = _module(dict(in_channels=8, n_heads=2), "default", dev, seed=5)
    h, w = 20, 19  # L = 380: six chunks, the last one partial
    x = _rand(2, 8, h, w, seed=6).to(dev)
    with torch.no_grad():
        y0 = mod(x).reshape(2, 8, -1)
        for p in (0, 63, 64, 200, h * w - 1):
            x2 = x.clone().reshape(2, 8, -1)
            x2[:, :, p] += 3.0
            y2 = mod(x2.reshape(2, 8, h, w)).reshape(2, 8, -1)
            assert torch.equal(y2[:, :, :p], y0[:, :, :p]), p
            assert not torch.equal(y2[:, :, p], y0[:, :, p]), p


def test_two_runs_are_bit_identical(dev):
    mod = _module(dict(in_channels=16, n_heads=4, embed_channels=32, out_channels=16), "default", dev, seed=7)
    x, g = _rand(2, 16, 33, 31, seed=8).to(dev), _rand(2, 16, 33, 31, seed=9).to(dev)
    y1, g1 = _fwd_bwd(mod, x, g)
    y2, g2 = _fwd_bwd(mod, x, g)
    assert torch.equal(y1, y2)
    for k in g1:
        assert torch.equal(g1[k], g2[k]), k


def test_graph_replay_equals_eager(dev):
    from pytorch_generative_amd import ops

    n, heads, e, v, h, w = 2, 2, 16, 24, 17, 15
    q0 = _rand(n, e, h, w, seed=10).to(dev)
    kv0 = _rand(n, e + v, h, w, seed=11).to(dev)
    d_o = _rand(n, v, h, w, seed=12).to(dev)

    def run(q, kv):
        o = ops.linear_causal_attention(q, kv, heads, e, v)
        gq, gkv = torch.autograd.grad(o, (q, kv), d_o)
        return o.detach(), gq, gkv

    o_e, gq_e, gkv_e = run(q0.clone().requires_grad_(True), kv0.clone().requires_grad_(True))
    sq, skv = q0.clone().requires_grad_(True), kv0.clone().requires_grad_(True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run(sq, skv)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr, capture_error_mode="thread_local"):
        o_g, gq_g, gkv_g = run(sq, skv)
    for it in range(3):
        gr.replay()
        torch.cuda.synchronize()
        assert torch.equal(o_g, o_e), f"replay {it}: output"
        assert torch.equal(gq_g, gq_e), f"replay {it}: dq"
        assert torch.equal(gkv_g, gkv_e), f"replay {it}: dkv"


def test_custom_feature_matches_closed_form(dev):
    """A feature_fn that is not elementwise over the head dim (a softmax over it) runs on the (N, heads, L, d) views,
    as in the reference, and the kernels take the mapped q / k as they are."""
    def feature(t):
        return torch.softmax(t, dim=-1) + 0.1

    from pytorch_generative_amd import nn as pg_nn

    torch.manual_seed(13)
    mod = pg_nn.LinearCausalAttention(8, feature_fn=feature, n_heads=2, embed_channels=12, out_channels=8).to(dev)
    x, g = _rand(2, 8, 11, 13, seed=14), _rand(2, 8, 11, 13, seed=15)
    y, grads = _fwd_bwd(mod, x.to(dev), g.to(dev))
    state = {k: v.detach().cpu().double().requires_grad_(True) for k, v in mod.state_dict().items()}
    x64 = x.double().requires_grad_(True)
    want = closed_form(state, x64, 2, 12, 8, feature)
    (want * g.double()).sum().backward()
    _util.assert_close(y, want, TOL, "custom feature y")
    rep = _util.GradReport("linear attention custom feature")
    for k, p in state.items():
        rep.add(k, grads[k], p.grad)
    rep.add("x", grads["x"], x64.grad)
    rep.finish()


def test_flat_adam_sinks_equal_grad_path(dev):
    from pytorch_generative_amd import optim

    kwargs = dict(in_channels=16, n_heads=4, embed_channels=16, out_channels=24)
    ref = _module(kwargs, "default", dev, seed=16)
    sunk = _module(kwargs, "default", dev, state=ref.state_dict(), seed=16)
    opt = optim.FlatAdam(sunk.parameters(), lr=1e-3)
    assert all(getattr(p, "_pg_grad", None) is not None for p in sunk.parameters())
    x, g = _rand(2, 16, 12, 14, seed=17).to(dev), _rand(2, 24, 12, 14, seed=18).to(dev)
    y_r, g_r = _fwd_bwd(ref, x, g)
    opt.zero_grad()
    xs = x.clone().requires_grad_(True)
    y_s = sunk(xs)
    (y_s * g).sum().backward()
    torch.cuda.synchronize()
    _util.assert_close(y_s, y_r, TOL, "sink y")
    _util.assert_close(xs.grad, g_r["x"], TOL, "sink dx")
    for k, p in sunk.named_parameters():
        _util.assert_close(p._pg_grad, g_r[k], TOL, f"sink {k}")


def test_memory_is_linear_in_sequence_length(dev):
    """N = 4, C = 64, 128 x 128 (L = 16384): forward + backward stay far below ONE L x L fp32 plane (1 GiB)."""
    mod = _module(dict(in_channels=64), "default", dev, seed=19)
    x = _rand(4, 64, 128, 128, seed=20).to(dev).requires_grad_(True)
    g = torch.ones(4, 64, 128, 128, device=dev)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    y = mod(x)
    (y * g).sum().backward()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    print(f"[linear attention] peak extra memory at L = 16384: {peak / 2**20:.1f} MiB")
    assert torch.isfinite(y).all() and torch.isfinite(x.grad).all()
    assert peak < 2**30 // 2, peak
