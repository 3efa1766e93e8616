"""GPU: the one-launch decode step (csrc/gpt_decode.hip: pg_gpt_decode_step) through the C-ABI, against the float64 reference
of tests/_gpt_decode_ref.py (itself pinned on the CPU by tests/test_gpt_decode_ref_cpu.py, which also shows that a float32
evaluation of these very inputs stays inside the bounds used here); then ImageGPT.sample() on it.

Bounds are the project's: _util.assert_close at 1e-5 (the existing sampler tests) and _util.GradReport's element-wise
defaults; everything stated as unchanged, equal between two paths, or zero is torch.equal."""

import math

import pytest
import torch

import _categorical_ref as cref
import _gpt_decode_ref as gref
import _util

pytestmark = pytest.mark.gpu

TOL = 1e-5
GUARD = 256            # sentinel floats on either side of every buffer the kernel writes
GUARD_VALUE = 54321.0
STRICT_IDS = {0: "causal", 1: "strict"}


def _sid(shape):
    return "-".join(map(str, shape))


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need the MI355X"
    from pytorch_generative_amd import _lib

    _lib.load()  # fail loudly if the extension is missing
    return torch.device("cuda:0")


class _Guarded:
    """A device copy of `t` with GUARD sentinel floats before and after it in one allocation."""

    def __init__(self, t, dev):
        self.flat = torch.full((t.numel() + 2 * GUARD,), GUARD_VALUE, device=dev)
        self.t = self.flat[GUARD:GUARD + t.numel()].view(t.shape)
        self.t.copy_(t)

    def intact(self):
        want = torch.full((GUARD,), GUARD_VALUE)
        return torch.equal(self.flat[:GUARD].cpu(), want) and torch.equal(self.flat[-GUARD:].cpu(), want)


def _launch(x, out, pack, kc, vc, n, heads, p, strict, pos_dev=None):
    """The raw status of pg_gpt_decode_step, called as ops.gpt_decode_step calls it."""
    from pytorch_generative_amd import _lib

    blocks, nn, C, L = kc.shape
    ld = x.shape[1]
    assert nn == n and x.shape == out.shape == (C, ld) and vc.shape == kc.shape
    assert all(t.is_contiguous() for t in (x, out, pack, kc, vc))
    return _lib.load().pg_gpt_decode_step(x.data_ptr(), out.data_ptr(), pack.data_ptr(), kc.data_ptr(), vc.data_ptr(), n, C,
                                          heads, blocks, L, ld, p, strict, gref.EPS,
                                          None if pos_dev is None else pos_dev.data_ptr(),
                                          torch.cuda.current_stream().cuda_stream)


def _run(dev, params, x, kc, vc, n, heads, p, strict, pos_dev=None):
    """One guarded launch from host tensors; returns (out, k_cache, v_cache) on the host after checking every sentinel."""
    from pytorch_generative_amd import _lib

    out_in = torch.full_like(x, gref.SENTINEL)
    out, kcd, vcd = _Guarded(out_in, dev), _Guarded(kc, dev), _Guarded(vc, dev)
    _lib.check(_launch(x.to(dev), out.t, gref.pack(params).to(dev), kcd.t, vcd.t, n, heads, p, strict, pos_dev),
               "pg_gpt_decode_step")
    torch.cuda.synchronize()
    assert out.intact() and kcd.intact() and vcd.intact(), "written outside a buffer"
    o = out.t.cpu()
    assert torch.equal(o[:, n:], out_in[:, n:]), "padding columns of the output written"
    return o[:, :n], kcd.t.cpu(), vcd.t.cpu()


def _compare(rep, name, got, want):
    _util.assert_close(got, want, TOL, name)
    rep.add(name, got, want)


def _check_caches(rep, tag, got, before, want, p):
    """Column p is the step's k / v (to the bound), every other entry keeps its bits (NaN included)."""
    for name, g, b, w in (("k", got[0], before[0], want[0]), ("v", got[1], before[1], want[1])):
        _compare(rep, f"{tag} {name} cache column", g[..., p], w[..., p])
        g = g.clone()
        g[..., p] = b[..., p]
        assert torch.equal(g.view(torch.int32), b.view(torch.int32)), f"{tag}: {name} cache written outside column {p}"


# ---------------------------------------------------------------------------------------------
# pg_gpt_decode_step
@pytest.mark.parametrize("strict", [0, 1], ids=STRICT_IDS.get)
@pytest.mark.parametrize("shape", gref.SHAPES, ids=_sid)
def test_single_steps(dev, shape, strict):
    """One step at p on either side of the wave and workgroup strides from random caches, every written buffer between
    sentinels: output and cache column p equal the reference, nothing else is written."""
    C, heads, blocks, L, n, ld = shape
    rep = _util.GradReport(f"gpt_decode {shape} {STRICT_IDS[strict]}")
    for p in gref.positions(L):
        params, x, kc, vc = gref.single_case(shape, p)
        want, kw, vw = gref.step(params, x[:, :n], kc, vc, p, heads, strict)
        got, kg, vg = _run(dev, params, x, kc, vc, n, heads, p, strict)
        _compare(rep, f"p={p}", got, want)
        _check_caches(rep, f"p={p}", (kg, vg), (kc, vc), (kw, vw), p)
    rep.finish()


@pytest.mark.parametrize("shape", [gref.SHAPES[0], gref.SHAPES[1]], ids=_sid)
def test_strict_at_position_zero_is_the_block_without_attention(dev, shape):
    """strict = 1 at p = 0 admits no key: o = 0 exactly, so the output equals the no-attention restatement — and no cache
    entry is read: caches full of NaN give the same bits."""
    C, heads, blocks, L, n, ld = shape
    params, x, kc, vc = gref.single_case(shape, 0)
    want = gref.step(params, x[:, :n], kc, vc, 0, heads, 0, attention=False)[0]
    got = _run(dev, params, x, kc, vc, n, heads, 0, 1)[0]
    rep = _util.GradReport(f"gpt_decode no attention {shape}")
    _compare(rep, "out", got, want)
    rep.finish()
    nan = torch.full_like(kc, float("nan"))
    got_nan = _run(dev, params, x, nan, nan.clone(), n, heads, 0, 1)[0]
    assert torch.equal(got_nan, got)


@pytest.mark.parametrize("shape", gref.SHAPES, ids=_sid)
def test_whole_sequence_host_and_device_position(dev, shape):
    """p = 0 .. L-1 from zeroed caches with fresh input columns per step, in place (out = x): all outputs and the final
    caches against the reference, once with p from the host and once with a device counter — bit-equal."""
    from pytorch_generative_amd import _lib

    C, heads, blocks, L, n, ld = shape
    params = gref.block_params(C, blocks)
    xs = gref.sequence_columns(C, n, ld, L)
    want, kw, vw = gref.sequence_ref(params, xs, n, heads, 0)
    pack = gref.pack(params).to(dev)
    runs = []
    for device_pos in (False, True):
        io = _Guarded(xs, dev)
        kc, vc = _Guarded(torch.zeros(blocks, n, C, L), dev), _Guarded(torch.zeros(blocks, n, C, L), dev)
        pos_dev = torch.zeros(1, dtype=torch.int32, device=dev) if device_pos else None
        for p in range(L):
            _lib.check(_launch(io.t[p], io.t[p], pack, kc.t, vc.t, n, heads, 0 if device_pos else p, 0, pos_dev),
                       "pg_gpt_decode_step")
            if device_pos:
                pos_dev.add_(1)
        torch.cuda.synchronize()
        assert io.intact() and kc.intact() and vc.intact()
        runs.append((io.t.cpu(), kc.t.cpu(), vc.t.cpu()))
    for a, b, what in zip(runs[0], runs[1], ("out", "k cache", "v cache")):
        assert torch.equal(a, b), f"host p != device position: {what}"
    out, kg, vg = runs[0]
    assert torch.equal(out[:, :, n:], xs[:, :, n:]), "padding columns written"
    rep = _util.GradReport(f"gpt_decode sequence {shape}")
    for p in range(L):
        _compare(rep, f"p={p}", out[p, :, :n], want[p])
    _compare(rep, "k cache", kg, kw)
    _compare(rep, "v cache", vg, vw)
    rep.finish()


@pytest.mark.parametrize("strict", [0, 1], ids=STRICT_IDS.get)
@pytest.mark.parametrize("shape", [gref.SHAPES[0], gref.SHAPES[2]], ids=_sid)
def test_device_position_is_clamped(dev, shape, strict):
    """*pos_dev outside [0, L) is clamped before any address is formed: -5 is p = 0, L + 7 is p = L - 1, bit for bit
    (output and both caches, sentinels intact)."""
    C, heads, blocks, L, n, ld = shape
    for bad, p in ((-5, 0), (L + 7, L - 1)):
        params, x, kc, vc = gref.single_case(shape, p)
        host = _run(dev, params, x, kc, vc, n, heads, p, strict)
        device = _run(dev, params, x, kc, vc, n, heads, 0, strict, torch.tensor([bad], dtype=torch.int32, device=dev))
        for a, b, what in zip(host, device, ("out", "k cache", "v cache")):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), f"*pos_dev = {bad} != p = {p}: {what}"
        _util.assert_close(host[0], gref.step(params, x[:, :n], kc, vc, p, heads, strict)[0], TOL, f"p={p}")


@pytest.mark.parametrize("shape", gref.SPIKE_SHAPES, ids=_sid)
def test_softmax_rescale(dev, shape):
    """One key scores +60 above all others — the first, a middle and the last admitted key (the position's own, which never
    comes from the cache): finite, and equal to the reference."""
    C, heads, L = shape
    p = L - 1
    rep = _util.GradReport(f"gpt_decode spike {shape}")
    for where in gref.spike_wheres(L):
        params, x, kc, vc = gref.spike_case(gref.block_params(C, 1), C, heads, 1, L, p, where)
        want = gref.step(params, x, kc, vc, p, heads, 0)[0]
        got = _run(dev, params, x, kc, vc, 1, heads, p, 0)[0]
        assert bool(torch.isfinite(got).all())
        _compare(rep, f"where={where}", got, want)
    rep.finish()


@pytest.mark.parametrize("strict", [0, 1], ids=STRICT_IDS.get)
@pytest.mark.parametrize("shape", [gref.SHAPES[0], gref.SHAPES[5]], ids=_sid)
def test_future_cache_columns_are_never_read(dev, shape, strict):
    """Columns > p hold NaN (column p too: it is written before any use): the output is finite and equal to the reference,
    and those columns keep their NaN bits."""
    C, heads, blocks, L, n, ld = shape
    rep = _util.GradReport(f"gpt_decode NaN future {shape} {STRICT_IDS[strict]}")
    for p in (0, 1, 64, L - 2):
        params, x, kc, vc = gref.single_case(shape, p, future=float("nan"))
        zk, zv = kc.clone(), vc.clone()
        zk[..., p:], zv[..., p:] = 0, 0  # the reference must not multiply NaN by a zero weight
        want, kw, vw = gref.step(params, x[:, :n], zk, zv, p, heads, strict)
        got, kg, vg = _run(dev, params, x, kc, vc, n, heads, p, strict)
        assert bool(torch.isfinite(got).all()), f"p={p}"
        _compare(rep, f"p={p}", got, want)
        _check_caches(rep, f"p={p}", (kg, vg), (kc, vc), (kw, vw), p)
        assert bool(torch.isnan(kg[..., p + 1:]).all()) and bool(torch.isnan(vg[..., p + 1:]).all())
    rep.finish()


def test_batch_independence_and_run_to_run_bits(dev):
    """Column 0 of an n = 5 launch is bit-identical to the n = 1 launch of that sample alone (another ld too), and two
    identical launches are bit-identical."""
    C, heads, blocks, L, n, ld = 64, 2, 2, 81, 5, 16
    p = 70
    params, x, kc, vc = gref.single_case((C, heads, blocks, L, n, ld), p)
    a = _run(dev, params, x, kc, vc, n, heads, p, 0)
    b = _run(dev, params, x, kc, vc, n, heads, p, 0)
    for s, t in zip(a, b):
        assert torch.equal(s, t), "two identical launches differ"
    one = _run(dev, params, x[:, :1].contiguous(), kc[:, :1].contiguous(), vc[:, :1].contiguous(), 1, heads, p, 0)
    assert torch.equal(one[0], a[0][:, :1])
    assert torch.equal(one[1], a[1][:, :1]) and torch.equal(one[2], a[2][:, :1])


@pytest.mark.parametrize("C,L", [(260, 20), (64, 4097)])
def test_shape_outside_the_domain_is_refused(dev, C, L):
    """PG_ESHAPE with a message, nothing launched: the sentinel-filled output is untouched."""
    from pytorch_generative_amd import _lib

    n, ld, heads = 2, 16, 2
    x = torch.randn(C, ld, device=dev)
    out = _Guarded(torch.full((C, ld), gref.SENTINEL), dev)
    pack = torch.zeros(12 * C * C + 13 * C, device=dev)
    kc, vc = torch.zeros(1, n, C, L, device=dev), torch.zeros(1, n, C, L, device=dev)
    rc = _launch(x, out.t, pack, kc, vc, n, heads, 0, 0)
    assert rc == -2
    with pytest.raises(ValueError, match="unsupported"):
        _lib.check(rc, "pg_gpt_decode_step")
    torch.cuda.synchronize()
    assert out.intact() and torch.equal(out.t.cpu(), torch.full((C, ld), gref.SENTINEL))
    assert not kc.any() and not vc.any()


# ---------------------------------------------------------------------------------------------
# ImageGPT.sample() on the step kernel
def _model(dev, channels=64, heads=2, cin=1, size=9, sample_fn=None):
    import pytorch_generative_amd as pg

    torch.manual_seed(0)
    model = pg.models.ImageGPT(in_channels=cin, out_channels=cin, in_size=size, n_transformer_blocks=2,
                               n_attention_heads=heads, n_embedding_channels=channels, sample_fn=sample_fn).to(dev)
    with torch.no_grad():
        model._pos.normal_(0, 0.1)
    return model


def _binary_canvas(dev, n=3, cin=1, size=9):
    g = torch.Generator().manual_seed(3)
    return torch.bernoulli(torch.full((n, cin, size, size), 0.3), generator=g).to(dev)


@pytest.mark.parametrize("channels,heads", [(64, 2), (24, 3)])
def test_sampler_logits_equal_the_full_forward(dev, channels, heads):
    """Teacher forcing as test_incremental_sampler_logits_equal_full_forward at widths outside the block kernels: the canvas
    comes back unchanged and the per-position logits are those of one full forward. (Without the step kernel this raised
    ValueError: return_logits needs the incremental sampler.)"""
    model = _model(dev, channels, heads)
    canvas = _binary_canvas(dev)
    assert model._incremental_ok(3)
    with torch.no_grad():
        full = model(canvas)
    out, logits = model.sample(conditioned_on=canvas, return_logits=True)
    assert model._sample_route == "step"
    assert torch.equal(out, canvas)
    _util.assert_close(logits, full.flatten(2).permute(2, 0, 1), TOL, f"step-kernel sampler logits, {channels} channels")


class _Recorder:
    """sample_fn that records the logits it is shown and 'draws' the teacher's codes."""

    def __init__(self, levels):
        self.levels, self.seen = levels, []

    def __call__(self, logits):
        p = len(self.seen)
        self.seen.append(logits.clone())
        return self.levels.flatten(1)[:, p:p + 1]


def _code_model(dev, k=12, size=9):
    from pytorch_generative_amd import nn as pg_nn

    model = _model(dev, 64, 2, cin=k, size=size, sample_fn=pg_nn.CategoricalSampler(k))
    model.input_codes = k
    return model


def test_code_input_samplers_equal_the_full_forward(dev):
    """input_codes = 12 on 64 channels, as test_samplers_equal_the_full_forward: from a fully known and from an empty canvas
    (a recording sample_fn plays the teacher), and the per-pixel full-forward sampler, all against one full forward."""
    k, size = 12, 9
    model = _code_model(dev, k, size)
    codes = torch.randint(0, k, (3, 1, size, size), generator=torch.Generator().manual_seed(4))
    levels = cref.to_level(codes, k).to(dev)
    with torch.no_grad():
        full = model(levels)
    want = full.flatten(2).permute(2, 0, 1)
    for canvas in (levels, torch.full_like(levels, -1.0)):
        rec = _Recorder(levels)
        model._sample_fn = rec
        out = model.sample(conditioned_on=canvas)
        assert model._sample_route == "step"
        assert torch.equal(out, levels) and len(rec.seen) == size * size
        _util.assert_close(torch.stack(rec.seen), want, TOL, "step-kernel sampler logits on code input")
    rec = _Recorder(levels)
    model._sample_fn = rec
    out = model.sample(conditioned_on=levels, incremental=False)
    assert model._sample_route == "full"
    assert torch.equal(out, levels)
    _util.assert_close(torch.stack(rec.seen), want, TOL, "per-pixel full forwards vs one full forward")


def test_eager_fallback_equals_graph_path(dev, monkeypatch):
    """When graph capture is refused, sample() launches every step eagerly: same kernels, same order — logits bit-equal to
    the replayed graph's. Both paths are shown to have been taken (81 replays; then no graph at all)."""
    model, canvas = _model(dev), _binary_canvas(dev)
    replays = []
    real_replay = torch.cuda.CUDAGraph.replay
    monkeypatch.setattr(torch.cuda.CUDAGraph, "replay", lambda self: (replays.append(1), real_replay(self))[1])
    out_g, logits_g = model.sample(conditioned_on=canvas, return_logits=True)
    assert len(replays) == 81, "the graph path did not replay once per pixel"

    refused = []

    class Refused:
        def __init__(self, *a, **k):
            refused.append(1)
            raise RuntimeError("graph capture refused")

    monkeypatch.setattr(torch.cuda, "CUDAGraph", Refused)
    out_e, logits_e = model.sample(conditioned_on=canvas, return_logits=True)
    assert refused == [1] and len(replays) == 81, "the eager fallback was not taken"
    assert model._sample_route == "step"
    assert torch.equal(out_e, out_g) and torch.equal(logits_e, logits_g)


def test_refused_capture_still_equals_the_full_forward(dev, monkeypatch, capsys):
    """With the graph constructor refusing (as in test_gpu_pcnnpp_sampling), the 64-channel sampler gives up after that one
    construction and its eagerly launched steps still produce the logits of one full forward; PG_DEBUG names the fallback."""
    model, canvas = _model(dev, 64, 2), _binary_canvas(dev)
    with torch.no_grad():
        full = model(canvas)
    refused = []

    class Refused:
        def __init__(self, *a, **k):
            refused.append(1)
            raise RuntimeError("graph capture refused")

    monkeypatch.setattr(torch.cuda, "CUDAGraph", Refused)
    monkeypatch.setenv("PG_DEBUG", "1")
    out, logits = model.sample(conditioned_on=canvas, return_logits=True)
    assert refused == [1], "not exactly one graph construction was attempted"
    assert "capture failed: RuntimeError: graph capture refused" in capsys.readouterr().out
    assert model._sample_route == "step"
    assert torch.equal(out, canvas)
    _util.assert_close(logits, full.flatten(2).permute(2, 0, 1), TOL, "eager step-kernel sampler logits, 64 channels")


def test_seeded_draws_repeat(dev):
    """Two sample(n_samples=3) calls with the same seeded CategoricalSampler generator give equal canvases."""
    k, size = 12, 9
    model = _code_model(dev, k, size)
    with torch.no_grad():
        model(torch.zeros(1, 1, size, size, device=dev))  # registers the canvas shape
    outs = []
    for _ in range(2):
        model._sample_fn.generator = torch.Generator(device=dev).manual_seed(7)
        outs.append(model.sample(n_samples=3))
        assert model._sample_route == "step"
    assert outs[0].shape == (3, 1, size, size) and torch.equal(outs[0], outs[1])
    levels = outs[0] * (k - 1)
    assert float(outs[0].min()) >= 0 and float((levels - levels.round()).abs().max()) <= 1e-4


def test_baseline_width_keeps_the_block_kernels(dev):
    """A 16-channel model still takes the fused head / tail block kernels; the step kernel forced onto it through `route`
    (the benchmark tool's switch) gives the same logits to the bound."""
    model, canvas = _model(dev, 16, 4), _binary_canvas(dev)
    assert model._decode_route(3) == "blocks"
    out_b, logits_b = model.sample(conditioned_on=canvas, return_logits=True)
    assert model._sample_route == "blocks"
    out_s, logits_s = model.sample(conditioned_on=canvas, return_logits=True, route="step")
    assert model._sample_route == "step"
    assert torch.equal(out_b, canvas) and torch.equal(out_s, canvas)
    with torch.no_grad():
        full = model(canvas)
    _util.assert_close(logits_s, full.flatten(2).permute(2, 0, 1), TOL, "forced step kernel at 16 channels")
    _util.assert_close(logits_b, full.flatten(2).permute(2, 0, 1), TOL, "block kernels at 16 channels")
    with pytest.raises(ValueError, match="not available"):
        _model(dev, 64, 2).sample(conditioned_on=canvas, route="blocks")


def test_ops_entry_checks_its_operands(dev):
    """ops.gpt_decode_step: the planner's refusal and mismatched operands are ValueErrors; ops.gpt_decode_pack builds what
    the reference's pack builds."""
    from pytorch_generative_amd import ops

    model = _model(dev, 24, 3)
    blocks = list(model._transformer)
    flat = ops.gpt_decode_pack(blocks)
    sd = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    params = []
    for i in range(len(blocks)):
        pre = f"_transformer.{i}."
        g = lambda name: sd[pre + name].flatten(1) if sd[pre + name].dim() == 4 else sd[pre + name]  # noqa: E731, B023
        params.append({"ln1_w": g("_ln1.weight"), "ln1_b": g("_ln1.bias"), "wq": g("_attn._q.weight"), "bq": g("_attn._q.bias"),
                       "wkv": g("_attn._kv.weight"), "bkv": g("_attn._kv.bias"), "wproj": g("_attn._proj.weight"),
                       "bproj": g("_attn._proj.bias"), "ln2_w": g("_ln2.weight"), "ln2_b": g("_ln2.bias"),
                       "w1": g("_out.0.weight"), "b1": g("_out.0.bias"), "w2": g("_out.2.weight"), "b2": g("_out.2.bias")})
    assert torch.equal(flat.cpu(), gref.pack(params))
    assert ops.gpt_decode_supported(model) and ops.gpt_decode_supported((24, 3, 2, 81))
    assert not ops.gpt_decode_supported((260, 2, 2, 81)) and not ops.gpt_decode_supported((64, 2, 2, 4097))
    x = torch.zeros(24, 16, device=dev)
    kc, vc = torch.zeros(2, 3, 24, 10, device=dev), torch.zeros(2, 3, 24, 10, device=dev)
    assert ops.gpt_decode_step(x, flat, kc, vc, 0, heads=3) is x
    with pytest.raises(ValueError, match="pack size"):
        ops.gpt_decode_step(x, flat[:-1], kc, vc, 0, heads=3)
    with pytest.raises(ValueError, match="do not divide"):
        ops.gpt_decode_step(x, flat, kc, vc, 0, heads=5)
    with pytest.raises(ValueError, match="outside the sequence"):
        ops.gpt_decode_step(x, flat, kc, vc, 10, heads=3)
    assert math.isfinite(float(x.abs().max()))
