"""GPU: the two kernels of incremental sampling (csrc/sampling.hip: pg_sample_embed, pg_attn_decode), called through
the C-ABI exactly as models/autoregressive/image_gpt.py calls them, against the float64 reference of
tests/_sampling_ref.py (itself pinned on the CPU by tests/test_sampling_ref_cpu.py, which also shows that a float32
evaluation of these very inputs stays inside the bounds used here).

Bounds are the project's: _util.assert_close at 1e-5 (the existing sampler tests) and _util.GradReport's element-wise
defaults; everything stated as unchanged, equal between two paths, or zero is torch.equal. Both template
instantiations of the decode kernel (<4, 4> and <32, 32>), both `strict` values, host p and device pos_dev (with its
clamp), and the sentinel-filled surroundings of every buffer the kernels write are covered; then ImageGPT.sample()
above them at head counts other than the default, and its eager fallback."""

import pytest
import torch

import _sampling_ref as sref
import _util
from oracle import ops as oops

pytestmark = pytest.mark.gpu

TOL = 1e-5
L = sref.L_DECODE
STRICT_IDS = {0: "causal", 1: "strict"}


def _sid(shape):
    return "-".join(map(str, shape))


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need the MI355X"
    from pytorch_generative_amd import _lib

    _lib.load()  # fail loudly if the extension is missing
    return torch.device("cuda:0")


def _decode(qkv, kc, vc, o, N, heads, p, dk, dv, ld, strict, pos_dev=None, seq_len=L):
    from pytorch_generative_amd import _lib

    assert qkv.is_contiguous() and kc.is_contiguous() and vc.is_contiguous() and o.is_contiguous()
    assert qkv.shape == (2 * heads * dk + heads * dv, ld) and o.shape == (heads * dv, ld)
    assert kc.shape == (N, heads * dk, seq_len) and vc.shape == (N, heads * dv, seq_len)
    st = torch.cuda.current_stream().cuda_stream
    _lib.check(_lib.load().pg_attn_decode(qkv.data_ptr(), kc.data_ptr(), vc.data_ptr(), o.data_ptr(), N, heads,
                                          seq_len, p, dk, dv, ld, strict,
                                          None if pos_dev is None else pos_dev.data_ptr(), st), "pg_attn_decode")


def _compare(rep, name, got, want):
    _util.assert_close(got, want, TOL, name)
    rep.add(name, got, want)


# ---------------------------------------------------------------------------------------------
# pg_attn_decode
SINGLE_CASES = [(s, 3, 16) for s in sref.DECODE_SHAPES] + [((4, 4, 4), 16, 16)]


@pytest.mark.parametrize("strict", [0, 1], ids=STRICT_IDS.get)
@pytest.mark.parametrize("shape,N,ld", SINGLE_CASES, ids=lambda v: _sid(v) if isinstance(v, tuple) else str(v))
def test_attn_decode_single_steps(dev, shape, N, ld, strict):
    """One step at p on either side of the 64-lane stride, every buffer surrounded by sentinels: the output equals the
    reference, and the kernel wrote column p of the caches and columns < N of o — nothing else."""
    heads, dk, dv = shape
    E, V = heads * dk, heads * dv
    rep = _util.GradReport(f"attn_decode {shape} N={N} {STRICT_IDS[strict]}")
    for p in sref.P_SINGLE:
        qkv = sref.decode_qkv(heads, dk, dv, N, ld, seed=p)
        kc, vc = sref.decode_caches(heads, dk, dv, N, L, p, seed=p)
        o_in = torch.full((V, ld), sref.SENTINEL)
        want = sref.decode_step(qkv, kc, vc, N, heads, L, p, dk, dv, ld, strict)[0][:, :N]
        kc_d, vc_d, o_d = kc.to(dev), vc.to(dev), o_in.to(dev)
        _decode(qkv.to(dev), kc_d, vc_d, o_d, N, heads, p, dk, dv, ld, strict)
        o, kc_o, vc_o = o_d.cpu(), kc_d.cpu(), vc_d.cpu()
        assert torch.equal(o[:, N:], o_in[:, N:]), f"p={p}: o written at columns n >= N"
        assert torch.equal(kc_o[:, :, p], qkv[E:2 * E, :N].t()), f"p={p}: k cache column p"
        assert torch.equal(vc_o[:, :, p], qkv[2 * E:, :N].t()), f"p={p}: v cache column p"
        kc_o[:, :, p], vc_o[:, :, p] = kc[:, :, p], vc[:, :, p]
        assert torch.equal(kc_o, kc), f"p={p}: k cache written outside column p"
        assert torch.equal(vc_o, vc), f"p={p}: v cache written outside column p"
        if p - strict < 0:
            assert torch.equal(o[:, :N], torch.zeros(V, N)), "no admitted key must give exactly 0"
            continue
        _compare(rep, f"p={p}", o[:, :N], want)
    rep.finish()


@pytest.mark.parametrize("strict", [0, 1], ids=STRICT_IDS.get)
@pytest.mark.parametrize("shape", sref.DECODE_SHAPES, ids=_sid)
def test_attn_decode_whole_sequence_host_and_device_position(dev, shape, strict):
    """p = 0 .. 129 from zeroed caches with a fresh qkv per step: all 130 outputs and the final caches against the
    reference, once with p from the host and once with a device position advanced between launches — bit-equal."""
    heads, dk, dv = shape
    N, ld = 3, 16
    E, V = heads * dk, heads * dv
    seq = sref.decode_sequence_qkv(heads, dk, dv, N, ld, L, seed=strict)
    want, kc_want, vc_want = sref.decode_sequence_ref(seq, N, heads, L, dk, dv, ld, strict)
    seq_d = seq.to(dev)
    runs = []
    for device_pos in (False, True):
        kc, vc = torch.zeros(N, E, L, device=dev), torch.zeros(N, V, L, device=dev)
        o = torch.full((L, V, ld), sref.SENTINEL, device=dev)
        pos_dev = torch.zeros(1, dtype=torch.int32, device=dev) if device_pos else None
        for p in range(L):
            _decode(seq_d[p], kc, vc, o[p], N, heads, 0 if device_pos else p, dk, dv, ld, strict, pos_dev)
            if device_pos:
                pos_dev.add_(1)
        runs.append((o.cpu(), kc.cpu(), vc.cpu()))
    (o_h, kc_h, vc_h), (o_d, kc_d, vc_d) = runs
    assert torch.equal(o_h, o_d) and torch.equal(kc_h, kc_d) and torch.equal(vc_h, vc_d), "host p != device pos_dev"
    assert torch.equal(o_h[:, :, N:], torch.full((L, V, ld - N), sref.SENTINEL))
    assert torch.equal(kc_h.double(), kc_want) and torch.equal(vc_h.double(), vc_want)
    if strict:
        assert torch.equal(o_h[0, :, :N], torch.zeros(V, N))
    rep = _util.GradReport(f"attn_decode sequence {shape} {STRICT_IDS[strict]}")
    for p in range(strict, L):
        _compare(rep, f"p={p}", o_h[p, :, :N], want[p])
    rep.finish()


@pytest.mark.parametrize("strict", [0, 1], ids=STRICT_IDS.get)
@pytest.mark.parametrize("shape", [(4, 4, 4), (1, 7, 29)], ids=_sid)
def test_attn_decode_device_position_is_clamped(dev, shape, strict):
    """*pos_dev outside [0, L) is clamped before any address is formed: -3 is p = 0, L + 5 is p = L - 1, bit for bit
    (outputs and both caches)."""
    heads, dk, dv = shape
    N, ld = 3, 16
    V = heads * dv
    for bad, p in ((-3, 0), (L + 5, L - 1)):
        qkv = sref.decode_qkv(heads, dk, dv, N, ld, seed=p).to(dev)
        kc, vc = sref.decode_caches(heads, dk, dv, N, L, p, seed=p)
        got = []
        for pos in (None, torch.tensor([bad], dtype=torch.int32, device=dev)):
            kc_d, vc_d = kc.to(dev), vc.to(dev)
            o = torch.full((V, ld), sref.SENTINEL, device=dev)
            _decode(qkv, kc_d, vc_d, o, N, heads, p if pos is None else 0, dk, dv, ld, strict, pos)
            got.append((o.cpu(), kc_d.cpu(), vc_d.cpu()))
        for a, b, what in zip(got[0], got[1], ("o", "k cache", "v cache")):
            assert torch.equal(a, b), f"*pos_dev = {bad} != p = {p}: {what}"
        want = sref.decode_step(qkv.cpu(), kc, vc, N, heads, L, p, dk, dv, ld, strict)[0][:, :N]
        if p - strict < 0:
            assert torch.equal(got[0][0][:, :N], torch.zeros(V, N))
        else:
            _util.assert_close(got[0][0][:, :N], want, TOL, f"p={p}")


@pytest.mark.parametrize("where,p", [("cache", 70), ("cache", 129), ("self", 70), ("self", 129)])
@pytest.mark.parametrize("score", [60.0, 100.0])
@pytest.mark.parametrize("shape", [(4, 4, 4), (1, 7, 29)], ids=_sid)
def test_attn_decode_softmax_rescale(dev, shape, score, where, p):
    """One key scores +60 (+100: past exp2's float range without the running maximum) and all others ~0 — first a key
    cached early in lane 3, whose lane maximum the merge must carry over, then the position's own key, which lane 0 adds
    from registers after its cached keys. Finite, and equal to the reference (the spike's value row)."""
    heads, dk, dv = shape
    N, ld = 3, 16
    qkv, kc, vc = sref.spike_case(heads, dk, dv, N, ld, L, p, score, where, seed=1)
    want = sref.decode_step(qkv, kc, vc, N, heads, L, p, dk, dv, ld, 0)[0][:, :N]
    o = torch.full((heads * dv, ld), sref.SENTINEL, device=dev)
    _decode(qkv.to(dev), kc.to(dev), vc.to(dev), o, N, heads, p, dk, dv, ld, 0)
    o = o.cpu()
    assert bool(torch.isfinite(o).all())
    rep = _util.GradReport(f"attn_decode spike {shape} {score} {where} p={p}")
    _compare(rep, "o", o[:, :N], want)
    rep.finish()


@pytest.mark.parametrize("strict", [0, 1], ids=STRICT_IDS.get)
@pytest.mark.parametrize("shape", [(4, 4, 4), (1, 1, 1), (2, 5, 4), (1, 7, 29)], ids=_sid)
def test_attn_decode_admitted_set_is_bit_exact(dev, shape, strict):
    """As test_attention_allowed_set_is_bit_exact (tests/test_gpu_ops.py) for the decode kernel: q = k = 0 and one-hot
    values make o[h * dv + j, n] of step p equal P[p, n * dv + j]; its non-zero pattern must be row p of
    oracle.ops.attention_mask for every p, and P * count == 1 to the 5e-6 of that test."""
    heads, dk, dv = shape
    E, V = heads * dk, heads * dv
    N = -(-L // dv)
    ld = (N + 15) // 16 * 16
    want = oops.attention_mask(L, bool(strict))
    steps = torch.stack([sref.onehot_value_step(heads, dk, dv, N, ld, p) for p in range(L)]).to(dev)
    kc, vc = torch.zeros(N, E, L, device=dev), torch.zeros(N, V, L, device=dev)
    o = torch.full((L, V, ld), sref.SENTINEL, device=dev)
    for p in range(L):
        _decode(steps[p], kc, vc, o[p], N, heads, p, dk, dv, ld, strict)
    o = o.cpu()
    assert torch.equal(o[:, :, N:], torch.full((L, V, ld - N), sref.SENTINEL))
    probs = o[:, :, :N].reshape(L, heads, dv, N).transpose(2, 3).reshape(L, heads, N * dv)[:, :, :L]  # [p, head, key]
    count = want.sum(1)
    for h in range(heads):
        assert torch.equal((probs[:, h] != 0).float(), want), f"admitted set, head {h}"
        assert float((probs[:, h] * count[:, None] - want).abs().max()) <= 5e-6, "P * count != 1"
    if strict:
        assert torch.equal(o[0, :, :N], torch.zeros(V, N))


# ---------------------------------------------------------------------------------------------
# pg_sample_embed
def _embed(canvas, pos, w, b, out, r, c, ld, pos_dev=None):
    from pytorch_generative_amd import _lib

    N, Cin, H, W = canvas.shape
    Cout, _, KH, KW = w.shape
    assert all(t is None or t.is_contiguous() for t in (canvas, pos, w, b, out)) and out.shape == (Cout, ld)
    st = torch.cuda.current_stream().cuda_stream
    _lib.check(_lib.load().pg_sample_embed(canvas.data_ptr(), None if pos is None else pos.data_ptr(), w.data_ptr(),
                                           None if b is None else b.data_ptr(), out.data_ptr(), N, Cin, H, W, Cout,
                                           KH, KW, r, c, ld, None if pos_dev is None else pos_dev.data_ptr(), st),
               "pg_sample_embed")


@pytest.mark.parametrize("kh,kw", sref.EMBED_KERNELS)
@pytest.mark.parametrize("cout", [1, 16])
@pytest.mark.parametrize("cin", [1, 3])
@pytest.mark.parametrize("n", [3, 70])
def test_sample_embed_every_pixel(dev, n, cin, cout, kh, kw):
    """Every pixel of a 4x5 image (all corners and edges) with an unmasked weight, pos / b given and each NULL: equal to
    the direct sum; columns n >= N untouched; (r, c) from the host and the raster position from the device — including
    values clamped at both ends — bit-equal."""
    H, W = sref.EMBED_HW
    ld = (n + 15) // 16 * 16
    canvas, pos, w, b = sref.embed_inputs(n, cin, cout, kh, kw)
    canvas_d, pos_d, w_d, b_d = (t.to(dev) for t in (canvas, pos, w, b))
    rep = _util.GradReport(f"sample_embed N={n} Cin={cin} Cout={cout} {kh}x{kw}")
    for use_pos, use_b in ((True, True), (False, True), (True, False)):
        args = (canvas_d, pos_d if use_pos else None, w_d, b_d if use_b else None)
        host = torch.full((H * W, cout, ld), sref.SENTINEL, device=dev)
        device = torch.full((H * W + 2, cout, ld), sref.SENTINEL, device=dev)
        pos_dev = torch.zeros(1, dtype=torch.int32, device=dev)
        for i in range(H * W):
            _embed(*args, host[i], i // W, i % W, ld)
            _embed(*args, device[i], 0, 0, ld, pos_dev)
            pos_dev.add_(1)
        for slot, bad in ((H * W, -2), (H * W + 1, H * W + 7)):  # clamped to the first / the last pixel
            pos_dev.fill_(bad)
            _embed(*args, device[slot], 0, 0, ld, pos_dev)
        host, device = host.cpu(), device.cpu()
        assert torch.equal(device[:H * W], host), "host (r, c) != device position"
        assert torch.equal(device[H * W], host[0]) and torch.equal(device[H * W + 1], host[H * W - 1]), "clamp"
        assert torch.equal(host[:, :, n:], torch.full((H * W, cout, ld - n), sref.SENTINEL)), "columns n >= N written"
        for i in range(H * W):
            want = sref.embed_pixel(canvas, pos if use_pos else None, w, b if use_b else None, i // W, i % W, ld)
            _compare(rep, f"pos={use_pos} b={use_b} ({i // W},{i % W})", host[i, :, :n], want[:, :n])
    rep.finish()


# ---------------------------------------------------------------------------------------------
# ImageGPT.sample() above them
def _sampler_model(dev, heads):
    import pytorch_generative_amd as pg

    torch.manual_seed(0)
    model = pg.models.ImageGPT(in_channels=2, out_channels=2, in_size=9, n_transformer_blocks=2,
                               n_attention_heads=heads).to(dev)
    with torch.no_grad():
        model._pos.normal_(0, 0.1)
    g = torch.Generator().manual_seed(3)
    canvas = torch.bernoulli(torch.full((3, 2, 9, 9), 0.3), generator=g).to(dev)
    return model, canvas


@pytest.mark.parametrize("heads", [1, 2, 8])
def test_incremental_sampler_other_head_counts(dev, heads):
    """Teacher forcing as test_incremental_sampler_logits_equal_full_forward, at head counts other than the default 4:
    16 channels in 1 / 2 heads are head dims 16 / 8 — the decode kernel's 32 template — and L = 81 crosses 64."""
    model, canvas = _sampler_model(dev, heads)
    with torch.no_grad():
        full = model(canvas)
    out, logits = model.sample(conditioned_on=canvas, return_logits=True)
    assert torch.equal(out, canvas)
    _util.assert_close(logits, full.flatten(2).permute(2, 0, 1), TOL, f"incremental logits, {heads} heads")


def test_incremental_sampler_eager_fallback_equals_graph_path(dev, monkeypatch):
    """When graph capture is refused, sample() launches every step eagerly: same kernels, same order — its logits equal
    the replayed graph's bit for bit. Both paths are shown to have been taken (81 replays; then no graph at all)."""
    model, canvas = _sampler_model(dev, 4)
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
    assert torch.equal(out_e, out_g) and torch.equal(logits_e, logits_g)
    with torch.no_grad():
        full = model(canvas)
    _util.assert_close(logits_e, full.flatten(2).permute(2, 0, 1), TOL, "eager incremental logits")
