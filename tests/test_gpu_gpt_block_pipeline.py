"""GPU: the software-pipelined tile loops of csrc/gpt_block.hip (prefetch of the wave's next tile, LDS transposes of the
weight-gradient operands) against a float64 restatement of the block's head and tail, at the tile counts where the
rotated loop takes a different path: waves without a tile, waves with one or two tiles (prologue and epilogue only),
and three to four tiles per wave under the grid caps (2048 / 1024 / 2048 / 512 workgroups of four waves: 6272 tiles
over 4096 and 2048 backward waves, 25 088 tiles over 8192 forward waves). Inputs live between NaN bands, so a prefetch that reads past a
tensor and is consumed shows in the result; through the C-ABI the outputs live between NaN bands too."""

import pytest
import torch
import torch.nn.functional as F

import _util

pytestmark = pytest.mark.gpu

TOL = 1e-4
PAD = 4096  # floats of NaN on either side of a guarded tensor (keeps 16-byte alignment)
# (N, H, W): tiles = N * H * W / 16
SHAPES = {"zero_tile_waves": (1, 4, 4), "prologue_epilogue": (3, 6, 8), "steady_bwd": (128, 28, 28), "steady_fwd": (512, 28, 28)}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need the MI355X"
    from pytorch_generative_amd import _lib

    _lib.load()
    return torch.device("cuda:0")


def _rand(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def _guarded(t, dev):
    """t on the device as a contiguous slice of a NaN-filled buffer: NaN before it and right behind its last element."""
    buf = torch.full((2 * PAD + t.numel(),), float("nan"), device=dev)
    buf[PAD:PAD + t.numel()] = t.flatten().to(dev)
    return buf, buf[PAD:PAD + t.numel()].view(t.shape)


def _bands_intact(buf, numel):
    return bool(torch.isnan(buf[:PAD]).all()) and bool(torch.isnan(buf[PAD + numel:]).all())


@pytest.fixture(scope="module")
def block(dev):
    from pytorch_generative_amd.models.autoregressive import image_gpt

    torch.manual_seed(0)
    blk = image_gpt.TransformerBlock(16, 4).to(dev)
    with torch.no_grad():
        for p in blk.parameters():
            p.add_(0.05 * torch.randn_like(p))
    return blk


def _mods(blk):
    return dict(ln1=blk._ln1, q=blk._attn._q, kv=blk._attn._kv, proj=blk._attn._proj, ln2=blk._ln2, fc1=blk._out[0],
                fc2=blk._out[2])


def _ln64(x, w, b, eps):
    return F.layer_norm(x.permute(0, 2, 3, 1), (16,), w, b, eps).permute(0, 3, 1, 2)


def _reference(blk, t, backward):
    """float64 restatement on the CPU: head qkv = [Wq; Wkv] LN1(x) + b with the alias x; tail x_new = x + x_mid +
    mlp(LN2(x_mid)), x_mid = x + Wp o + bp. Returns outputs, input gradients and the parameter gradients by name."""
    m = _mods(blk)
    P = {k: p.detach().double().cpu().requires_grad_(backward) for k, p in blk.named_parameters()}
    name = {id(p): k for k, p in blk.named_parameters()}
    w = lambda mod: P[name[id(mod.weight)]]  # noqa: E731
    b = lambda mod: P[name[id(mod.bias)]]  # noqa: E731
    x, o = (t[k].double().requires_grad_(backward) for k in ("x", "o"))
    y = _ln64(x, w(m["ln1"]), b(m["ln1"]), m["ln1"].eps)
    qkv = F.conv2d(y, torch.cat([w(m["q"]), w(m["kv"])]), torch.cat([b(m["q"]), b(m["kv"])]))
    xt = t["x"].double().requires_grad_(backward)
    xm = xt + F.conv2d(o, w(m["proj"]), b(m["proj"]))
    h = F.conv2d(_ln64(xm, w(m["ln2"]), b(m["ln2"]), m["ln2"].eps), w(m["fc1"]), b(m["fc1"]))
    xnew = xt + xm + F.conv2d(F.gelu(h), w(m["fc2"]), b(m["fc2"]))
    out = {"qkv": qkv.detach(), "xnew": xnew.detach()}
    if backward:
        ((qkv * t["dqkv"].double()).sum() + (x * t["gx"].double()).sum() + (xnew * t["d"].double()).sum()).backward()
        out.update(dx=x.grad, d_o=o.grad, gx_out=xt.grad, params={k: p.grad for k, p in P.items() if p.grad is not None})
    return out


def _inputs(shape):
    n, h, w = shape
    return {"x": _rand(n, 16, h, w, seed=1), "o": _rand(n, 16, h, w, seed=2), "dqkv": _rand(n, 48, h, w, seed=3),
            "gx": _rand(n, 16, h, w, seed=4), "d": _rand(n, 16, h, w, seed=5)}


@pytest.fixture(scope="module")
def references(block):
    """One float64 reference per shape, shared and left unchanged (the largest shape is forward-only)."""
    return {k: (_inputs(s), _reference(block, _inputs(s), backward=(k != "steady_fwd"))) for k, s in SHAPES.items()}


@pytest.mark.parametrize("case", list(SHAPES))
def test_block_kernels_match_float64_between_nan_bands(dev, block, references, case):
    """ops.gpt_block_head / gpt_block_tail forward (and backward, except at the forward steady-state shape) with every
    input a slice of a NaN-filled buffer whose NaN starts right behind the last image."""
    from pytorch_generative_amd import ops

    t, want = references[case]
    backward = "dx" in want
    m = _mods(block)
    assert ops.gpt_block_supported(t["x"], m["ln1"], m["q"], m["kv"], m["proj"], m["ln2"], m["fc1"], m["fc2"])
    g = {k: _guarded(v, dev)[1] for k, v in t.items()}
    block.zero_grad()
    o = g["o"].requires_grad_(backward)
    xh = g["x"].requires_grad_(backward)
    xt = _guarded(t["x"], dev)[1].requires_grad_(backward)
    qkv, xs = ops.gpt_block_head(xh, m["ln1"], m["q"], m["kv"])
    xnew = ops.gpt_block_tail(o, xt, m["proj"], m["ln2"], m["fc1"], m["fc2"])
    _util.assert_close(qkv, want["qkv"], TOL, f"{case} qkv")
    _util.assert_close(xnew, want["xnew"], TOL, f"{case} x_new")
    if not backward:
        return
    torch.autograd.backward([qkv, xs, xnew], [g["dqkv"], g["gx"], g["d"]])
    torch.cuda.synchronize()
    _util.assert_close(xh.grad, want["dx"], TOL, f"{case} dx")
    _util.assert_close(o.grad, want["d_o"], TOL, f"{case} d_o")
    _util.assert_close(xt.grad, want["gx_out"], TOL, f"{case} gx")
    rep = _util.GradReport(f"gpt_block_pipeline[{case}]")
    for k, p in block.named_parameters():
        if k in want["params"]:
            rep.add(k, p.grad, want["params"][k])
    assert len(rep.rows) >= 14
    rep.finish()


@pytest.mark.parametrize("case", list(SHAPES))
def test_block_kernels_leave_output_guard_bands_alone(dev, lib, block, references, case):
    """The four kernels through the C-ABI with inputs AND outputs between NaN bands: outputs equal the reference, every
    band is still NaN afterwards (at the forward steady-state shape the two forward kernels only, as above)."""
    t, want = references[case]
    backward = "dx" in want
    n, h, w = SHAPES[case]
    L, eps = h * w, 1e-5
    m = _mods(block)
    gi = {k: _guarded(v, dev) for k, v in t.items()}
    outs = (("qkv", 48), ("xnew", 16)) + ((("d_o", 16), ("gx_out", 16), ("dx", 16)) if backward else ())
    go = {k: _guarded(torch.zeros(n, c, h, w), dev) for k, c in outs}
    p = lambda k: (gi[k] if k in gi else go[k])[1].data_ptr()  # noqa: E731
    wp = lambda mod: mod.weight.data_ptr()  # noqa: E731
    bp = lambda mod: mod.bias.data_ptr()  # noqa: E731
    grads = {k: torch.zeros_like(q) for k, q in block.named_parameters()}
    name = {id(q): k for k, q in block.named_parameters()}
    gw = lambda mod: grads[name[id(mod.weight)]].data_ptr()  # noqa: E731
    gb = lambda mod: grads[name[id(mod.bias)]].data_ptr()  # noqa: E731
    st = torch.cuda.current_stream().cuda_stream
    hn, tn = lib.pg_gpt_block_head_bwd_workspace_floats(n, L), lib.pg_gpt_block_tail_bwd_workspace_floats(n, L)
    hws, tws = _guarded(torch.zeros(hn), dev), _guarded(torch.zeros(tn), dev)
    assert lib.pg_gpt_block_head_fwd(p("x"), wp(m["ln1"]), bp(m["ln1"]), wp(m["q"]), bp(m["q"]), wp(m["kv"]), bp(m["kv"]),
                                     p("qkv"), n, 16, L, eps, st) == 0
    assert lib.pg_gpt_block_tail_fwd(p("o"), p("x"), wp(m["proj"]), bp(m["proj"]), wp(m["ln2"]), bp(m["ln2"]), wp(m["fc1"]),
                                     bp(m["fc1"]), wp(m["fc2"]), bp(m["fc2"]), p("xnew"), n, 16, 64, L, eps, st) == 0
    if backward:
        assert lib.pg_gpt_block_tail_bwd(p("o"), p("x"), wp(m["proj"]), bp(m["proj"]), wp(m["ln2"]), bp(m["ln2"]), wp(m["fc1"]),
                                         bp(m["fc1"]), wp(m["fc2"]), p("d"), p("d_o"), p("gx_out"), gw(m["proj"]), gb(m["proj"]),
                                         gw(m["ln2"]), gb(m["ln2"]), gw(m["fc1"]), gb(m["fc1"]), gw(m["fc2"]), gb(m["fc2"]),
                                         n, 16, 64, L, eps, tws[1].data_ptr(), tn, st) == 0
        assert lib.pg_gpt_block_head_bwd(p("x"), wp(m["ln1"]), bp(m["ln1"]), wp(m["q"]), wp(m["kv"]), p("dqkv"), p("gx"), p("dx"),
                                         gw(m["ln1"]), gb(m["ln1"]), gw(m["q"]), gb(m["q"]), gw(m["kv"]), gb(m["kv"]),
                                         n, 16, L, eps, hws[1].data_ptr(), hn, st) == 0
    torch.cuda.synchronize()
    for k, (buf, view) in {**gi, **go, "head_ws": hws, "tail_ws": tws}.items():
        assert _bands_intact(buf, view.numel()), f"{case}: NaN band around {k} was written"
    for k in go:
        _util.assert_close(go[k][1], want[k], TOL, f"{case} {k} (C-ABI)")
    if not backward:
        return
    rep = _util.GradReport(f"gpt_block_pipeline_cabi[{case}]")
    for k in grads:
        if k in want["params"]:
            rep.add(k, grads[k], want["params"][k])
    rep.finish()


def test_block_accepts_a_batch_strided_view(dev, block, references):
    """gpt_block_supported looks at shapes only, so a view whose batch stride exceeds C * L is admitted; the kernels
    index with n * C * L, and the operator hands them a contiguous copy: results equal the contiguous call bit for bit."""
    from pytorch_generative_amd import ops

    t, _ = references["prologue_epilogue"]
    m = _mods(block)
    wide = torch.full((3, 32, 6, 8), float("nan"), device=dev)
    wide[:, :16] = t["x"].to(dev)
    view = wide[:, :16]
    assert not view.is_contiguous() and view.stride(0) == 2 * 16 * 48
    assert ops.gpt_block_supported(view, m["ln1"], m["q"], m["kv"], m["proj"], m["ln2"], m["fc1"], m["fc2"])
    o = t["o"].to(dev)
    outs = []
    for x in (view, t["x"].to(dev)):
        block.zero_grad()
        x = x.detach().requires_grad_(True)
        qkv, xs = ops.gpt_block_head(x, m["ln1"], m["q"], m["kv"])
        xnew = ops.gpt_block_tail(o, xs, m["proj"], m["ln2"], m["fc1"], m["fc2"])
        torch.autograd.backward([qkv, xnew], [t["dqkv"].to(dev), t["d"].to(dev)])
        outs.append((qkv.detach(), xnew.detach(), x.grad.clone(), [p.grad.clone() for p in block.parameters() if p.grad is not None]))
    a, b = outs
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])
    assert len(a[3]) == len(b[3]) >= 14 and all(torch.equal(u, v) for u, v in zip(a[3], b[3]))
    assert bool(torch.isnan(wide[:, 16:]).all())


def test_image_gpt_graph_replays_equal_eager_steps(dev):
    """ImageGPT (8 blocks / 4 heads / 16 channels) at N = 2: three replays of the captured step equal three eager steps
    bit for bit under ops.set_deterministic(True)."""
    import pytorch_generative_amd as pg
    from pytorch_generative_amd import graph, ops, optim

    def make():
        torch.manual_seed(0)
        return pg.models.ImageGPT(1, 1, in_size=28, n_transformer_blocks=8, n_attention_heads=4, n_embedding_channels=16).to(dev)

    g = torch.Generator().manual_seed(11)
    xs = [torch.bernoulli(torch.full((2, 1, 28, 28), 0.1307), generator=g).to(dev) for _ in range(3)]
    loss_fn = lambda x, preds: ops.bce_with_logits_sum_mean(preds, x)  # noqa: E731
    was = ops.set_deterministic(True)
    try:
        m1, m2 = make(), make()
        o1, o2 = optim.FlatAdam(m1.parameters(), lr=1e-3), optim.FlatAdam(m2.parameters(), lr=1e-3)
        for x in xs:
            o1.zero_grad()
            loss_fn(x, m1(x)).backward()
            o1.step()
        step = graph.GraphedTrainStep(m2, o2, loss_fn, xs[0], preserve_state=True)
        for x in xs:
            step(x)
        torch.cuda.synchronize()
        assert torch.equal(o1.flat_param, o2.flat_param), "graph replays differ from eager steps"
        assert torch.equal(o1.exp_avg, o2.exp_avg) and torch.equal(o1.exp_avg_sq, o2.exp_avg_sq)
    finally:
        ops.set_deterministic(was)
