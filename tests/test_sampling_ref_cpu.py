"""CPU: tests/_sampling_ref.py (the float64 reference of the incremental sampler's two kernels) is itself pinned —
decode_step against oracle.ops.causal_attention_core / attention_mask, embed_pixel against torch's conv2d — and the
inputs of tests/test_gpu_sampling_kernels.py are shown to leave a correct float32 evaluation inside the project's
tolerances (_util.assert_close at 1e-5, _util.GradReport's element-wise defaults), so that a miss on the GPU is the
kernel's and not the inputs'."""

import pytest
import torch
import torch.nn.functional as F

import _sampling_ref as sref
import _util
from oracle import ops as oops

TOL = 1e-5  # the bound of the existing sampler tests (tests/test_gpu_models.py)


@pytest.mark.parametrize("strict", [0, 1])
@pytest.mark.parametrize("heads,dk,dv,h,w", [(2, 3, 5, 3, 4), (1, 1, 1, 2, 3), (3, 4, 2, 1, 7)])
def test_decode_steps_equal_full_causal_attention(heads, dk, dv, h, w, strict):
    """p = 0 .. L-1 from empty caches IS causal attention: equal to oracle.ops.causal_attention_core in float64, and the
    caches end as the keys / values themselves. Padding columns of o pass through."""
    N, ld, L = 3, 16, h * w
    E, V = heads * dk, heads * dv
    g = torch.Generator().manual_seed(5)
    q = torch.randn(N, E, h, w, generator=g, dtype=torch.float64)
    k = torch.randn(N, E, h, w, generator=g, dtype=torch.float64)
    v = torch.randn(N, V, h, w, generator=g, dtype=torch.float64)
    want = oops.causal_attention_core(q, k, v, heads, bool(strict)).reshape(N, V, L)
    kc, vc = torch.zeros(N, E, L, dtype=torch.float64), torch.zeros(N, V, L, dtype=torch.float64)
    for p in range(L):
        qkv = torch.full((2 * E + V, ld), sref.GARBAGE, dtype=torch.float64)
        qkv[:, :N] = torch.cat([q.reshape(N, E, L)[:, :, p], k.reshape(N, E, L)[:, :, p], v.reshape(N, V, L)[:, :, p]], 1).t()
        o_in = torch.full((V, ld), sref.SENTINEL, dtype=torch.float64)
        o, kc, vc = sref.decode_step(qkv, kc, vc, N, heads, L, p, dk, dv, ld, strict, o=o_in)
        assert torch.equal(o[:, N:], o_in[:, N:])
        assert float((o[:, :N].t() - want[:, :, p]).abs().max()) <= 1e-13 * max(1.0, float(want.abs().max())), p
    assert torch.equal(kc, k.reshape(N, E, L)) and torch.equal(vc, v.reshape(N, V, L))
    if strict:
        assert float(want[:, :, 0].abs().max()) == 0.0  # the oracle's empty row, reproduced exactly above


@pytest.mark.parametrize("strict", [0, 1])
def test_decode_admitted_set_equals_attention_mask(strict):
    """q = k = 0, one-hot values: the non-zero outputs of step p mark exactly row p of oracle.ops.attention_mask."""
    heads, dk, dv, L = 2, 3, 4, 21
    N = -(-L // dv)
    ld = (N + 15) // 16 * 16
    want = oops.attention_mask(L, bool(strict))
    kc = torch.zeros(N, heads * dk, L, dtype=torch.float64)
    vc = torch.zeros(N, heads * dv, L, dtype=torch.float64)
    got = torch.zeros(heads, L, L)
    for p in range(L):
        qkv = sref.onehot_value_step(heads, dk, dv, N, ld, p)
        o, kc, vc = sref.decode_step(qkv, kc, vc, N, heads, L, p, dk, dv, ld, strict)
        got[:, p] = o[:, :N].reshape(heads, dv, N).transpose(1, 2).reshape(heads, N * dv)[:, :L]
    count = want.sum(1)
    for h in range(heads):
        assert torch.equal((got[h] != 0).float(), want)
        assert float((got[h] * count[:, None] - want).abs().max()) <= 1e-12


@pytest.mark.parametrize("k", [1, 3, 5])
@pytest.mark.parametrize("use_pos,use_b", [(True, True), (False, True), (True, False)])
def test_embed_pixel_equals_conv2d(k, use_pos, use_b):
    """Odd kernels: embed_pixel over all (r, c) is Conv2d(padding = k // 2) on canvas + pos."""
    N, Cin, Cout, ld = 3, 2, 5, 16
    H, W = sref.EMBED_HW
    canvas, pos, w, b = (t.double() for t in sref.embed_inputs(N, Cin, Cout, k, k))
    x = canvas + pos if use_pos else canvas
    want = F.conv2d(x, w, b if use_b else None, padding=k // 2)
    for r in range(H):
        for c in range(W):
            out_in = torch.full((Cout, ld), sref.SENTINEL, dtype=torch.float64)
            got = sref.embed_pixel(canvas, pos if use_pos else None, w, b if use_b else None, r, c, ld, out=out_in)
            assert torch.equal(got[:, N:], out_in[:, N:])
            assert float((got[:, :N].t() - want[:, :, r, c]).abs().max()) <= 1e-13 * float(want.abs().max())


def test_embed_pixel_even_kernel_taps():
    """2x2: tap (u, v) reads (r + u - 1, c + v - 1) — the kernel's integer division — so pixel (0, 0) sees only tap (1, 1)."""
    canvas, pos, w, b = (t.double() for t in sref.embed_inputs(3, 1, 2, 2, 2))
    got = sref.embed_pixel(canvas, None, w, None, 0, 0, 16)
    assert torch.equal(got[:, :3], w[:, 0, 1, 1].reshape(2, 1) * canvas[:, 0, 0, 0].reshape(1, 3))
    got = sref.embed_pixel(canvas, None, w, None, 2, 3, 16)
    want = sum(w[:, 0, u, v].reshape(2, 1) * canvas[:, 0, 1 + u, 2 + v].reshape(1, 3) for u in range(2) for v in range(2))
    assert float((got[:, :3] - want).abs().max()) <= 1e-14


# ---------------------------------------------------------------------------------------------
# the inputs of the GPU tier: a float32 evaluation of the same statement stays inside the project's bounds
def _check32(rep, name, got32, want64):
    _util.assert_close(got32, want64, TOL, name)
    rep.add(name, got32, want64)


@pytest.mark.parametrize("strict", [0, 1])
@pytest.mark.parametrize("shape", sref.DECODE_SHAPES, ids=lambda s: "-".join(map(str, s)))
def test_fp32_decode_single_steps_within_bounds(shape, strict):
    heads, dk, dv = shape
    L = sref.L_DECODE
    rep = _util.GradReport(f"fp32 decode {shape} strict={strict}")
    for N, ld in ((3, 16), (16, 16)) if shape == (4, 4, 4) else ((3, 16),):
        for p in sref.P_SINGLE:
            qkv = sref.decode_qkv(heads, dk, dv, N, ld, seed=p)
            kc, vc = sref.decode_caches(heads, dk, dv, N, L, p, seed=p)
            want = sref.decode_step(qkv, kc, vc, N, heads, L, p, dk, dv, ld, strict)[0][:, :N]
            got = sref.decode_step(qkv, kc, vc, N, heads, L, p, dk, dv, ld, strict, dtype=torch.float32)[0][:, :N]
            if p - strict < 0:
                assert float(want.abs().max()) == 0.0 and float(got.abs().max()) == 0.0
                continue
            _check32(rep, f"N={N} p={p}", got, want)
    rep.finish()


@pytest.mark.parametrize("strict", [0, 1])
@pytest.mark.parametrize("shape", sref.DECODE_SHAPES, ids=lambda s: "-".join(map(str, s)))
def test_fp32_decode_sequence_within_bounds(shape, strict):
    heads, dk, dv = shape
    N, ld, L = 3, 16, sref.L_DECODE
    seq = sref.decode_sequence_qkv(heads, dk, dv, N, ld, L, seed=strict)
    want = sref.decode_sequence_ref(seq, N, heads, L, dk, dv, ld, strict)[0]
    got = sref.decode_sequence_ref(seq, N, heads, L, dk, dv, ld, strict, dtype=torch.float32)[0]
    rep = _util.GradReport(f"fp32 decode sequence {shape} strict={strict}")
    for p in range(strict, L):
        _check32(rep, f"p={p}", got[p], want[p])
    rep.finish()


@pytest.mark.parametrize("where,p", [("cache", 70), ("cache", 129), ("self", 70), ("self", 129)])
@pytest.mark.parametrize("score", [60.0, 100.0])
@pytest.mark.parametrize("shape", [(4, 4, 4), (1, 7, 29)], ids=lambda s: "-".join(map(str, s)))
def test_fp32_decode_spike_within_bounds(shape, score, where, p):
    heads, dk, dv = shape
    N, ld, L = 3, 16, sref.L_DECODE
    qkv, kc, vc = sref.spike_case(heads, dk, dv, N, ld, L, p, score, where, seed=1)
    want = sref.decode_step(qkv, kc, vc, N, heads, L, p, dk, dv, ld, 0)[0][:, :N]
    got = sref.decode_step(qkv, kc, vc, N, heads, L, p, dk, dv, ld, 0, dtype=torch.float32)[0][:, :N]
    assert bool(torch.isfinite(got).all())
    # the spike really dominates: the output is the spike's value to ~e^-score
    spike_v = (qkv[2 * heads * dk:, :N] if where == "self" else vc[:, :, 3].t()).double()
    assert float((want - spike_v).abs().max()) < 1e-20
    rep = _util.GradReport(f"fp32 spike {shape} {score} {where} p={p}")
    _check32(rep, "o", got, want)
    rep.finish()


@pytest.mark.parametrize("kh,kw", sref.EMBED_KERNELS)
@pytest.mark.parametrize("cout", [1, 16])
@pytest.mark.parametrize("cin", [1, 3])
@pytest.mark.parametrize("n", [3, 70])
def test_fp32_embed_within_bounds(n, cin, cout, kh, kw):
    H, W = sref.EMBED_HW
    ld = (n + 15) // 16 * 16
    canvas, pos, w, b = sref.embed_inputs(n, cin, cout, kh, kw)
    rep = _util.GradReport(f"fp32 embed N={n} Cin={cin} Cout={cout} {kh}x{kw}")
    for use_pos, use_b in ((True, True), (False, True), (True, False)):
        for r in range(H):
            for c in range(W):
                args = (canvas, pos if use_pos else None, w, b if use_b else None, r, c, ld)
                want = sref.embed_pixel(*args)[:, :n]
                got = sref.embed_pixel(*args, dtype=torch.float32)[:, :n]
                _check32(rep, f"pos={use_pos} b={use_b} ({r},{c})", got, want)
    rep.finish()
