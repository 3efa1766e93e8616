"""CPU: tests/_gpt_decode_ref.py (the float64 reference of the one-launch decode step, csrc/gpt_decode.hip) is itself pinned —
iterated over all positions it IS oracle.models.image_gpt's full forward — the inputs of tests/test_gpu_gpt_decode.py are
shown to leave a correct float32 evaluation inside the bounds used there (_util.assert_close at 1e-5, _util.GradReport's
element-wise defaults), so that a miss on the GPU is the kernel's and not the inputs'; and the planner is swept without a
device: pg_gpt_decode_plan and the launch entry point accept exactly the same shapes, among them the whole stated domain."""

import ctypes

import pytest
import torch
import torch.nn.functional as F

import _gpt_decode_ref as gref
import _sampling_ref as sref
import _util
from oracle import models as omodels
from test_host_cpu import _fake_ptr, _no_gpu, _reached_launch

TOL = 1e-5  # the bound of the existing sampler tests


def _sid(shape):
    return "-".join(map(str, shape))


@pytest.mark.parametrize("C,heads,blocks,H,W", [(8, 2, 2, 3, 3), (24, 3, 1, 4, 5)])
def test_iterated_step_equals_the_full_forward(C, heads, blocks, H, W):
    """Stem pixel -> reference step over all blocks -> final LayerNorm + 1x1 head, for p = 0 .. L-1 from empty caches: the
    logits of oracle.models.image_gpt's one full forward, in float64 to 1e-12; the caches never change behind p."""
    N, L = 3, H * W
    state, params = gref.model_state(C, heads, blocks, H, W, in_ch=2, out_ch=3)
    g = torch.Generator().manual_seed(11)
    img = torch.bernoulli(torch.full((N, 2, H, W), 0.4), generator=g).double()
    full = omodels.image_gpt(state, img, heads)  # masks _input.weight in place, as every forward does
    kc = torch.zeros(blocks, N, C, L, dtype=torch.float64)
    vc = torch.zeros(blocks, N, C, L, dtype=torch.float64)
    for p in range(L):
        r, c = divmod(p, W)
        x = sref.embed_pixel(img, state["_pos"][0], state["_input.weight"], state["_input.bias"], r, c, N)
        before = (kc.clone(), vc.clone())
        h, kc, vc = gref.step(params, x, kc, vc, p, heads, 0)
        for new, old in zip((kc, vc), before):
            assert torch.equal(new[..., :p], old[..., :p]) and torch.equal(new[..., p + 1:], old[..., p + 1:])
        y = F.layer_norm(h.t(), (C,), state["_ln.weight"], state["_ln.bias"], gref.EPS)
        logits = y @ state["_out.weight"].reshape(3, C).t() + state["_out.bias"]
        assert float((logits - full[:, :, r, c]).abs().max()) <= 1e-12 * max(1.0, float(full.abs().max())), p


def test_no_attention_restatement_is_strict_at_position_zero():
    """strict = 1 at p = 0 admits no key: o = 0, which `attention=False` restates without the attention step."""
    C, heads, blocks, L, n = 24, 3, 2, 7, 3
    params = gref.block_params(C, blocks)
    x = gref.columns(C, n, n)
    kc, vc = gref.caches(C, blocks, n, L, 0)
    a = gref.step(params, x, kc, vc, 0, heads, 1)
    b = gref.step(params, x, kc, vc, 0, heads, 0, attention=False)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])
    assert not torch.equal(a[0], gref.step(params, x, kc, vc, 0, heads, 0)[0])


def test_pack_follows_the_plan(lib):
    """gref.pack lays the parameters out as the plan says: every field where its offset is, transposed to (in, out)."""
    from pytorch_generative_amd import ops

    C, blocks = 12, 3
    params = gref.block_params(C, blocks)
    flat = gref.pack(params)
    plan = ops.gpt_decode_plan(C, 3, blocks, 10)
    assert flat.numel() == plan["pack_floats"] == blocks * plan["block_floats"]
    assert tuple(plan["offsets"]) == gref.FIELDS
    for i, w in enumerate(params):
        blk = flat[i * plan["block_floats"]:(i + 1) * plan["block_floats"]]
        off = plan["offsets"]
        assert torch.equal(blk[off["wqkv"]:off["bqkv"]].reshape(C, 3 * C), torch.cat((w["wq"], w["wkv"])).t())
        assert torch.equal(blk[off["w2"]:off["b2"]].reshape(4 * C, C), w["w2"].t())
        assert torch.equal(blk[off["b2"]:], w["b2"]) and torch.equal(blk[off["ln2_b"]:off["w1"]], w["ln2_b"])


# ---------------------------------------------------------------------------------------------
# the inputs of the GPU tier: a float32 evaluation of the same statement stays inside the project's bounds
def _check32(rep, name, got32, want64):
    _util.assert_close(got32, want64, TOL, name)
    rep.add(name, got32, want64)


@pytest.mark.parametrize("strict", [0, 1])
@pytest.mark.parametrize("shape", gref.SHAPES, ids=_sid)
def test_fp32_single_steps_within_bounds(shape, strict):
    C, heads, blocks, L, n, ld = shape
    rep = _util.GradReport(f"fp32 gpt_decode {shape} strict={strict}")
    for p in gref.positions(L):
        params, x, kc, vc = gref.single_case(shape, p)
        want = gref.step(params, x[:, :n], kc, vc, p, heads, strict)[0]
        got = gref.step(params, x[:, :n], kc, vc, p, heads, strict, dtype=torch.float32)[0]
        _check32(rep, f"p={p}", got, want)
    rep.finish()


@pytest.mark.parametrize("shape", gref.SHAPES, ids=_sid)
def test_fp32_sequence_within_bounds(shape):
    C, heads, blocks, L, n, ld = shape
    params = gref.block_params(C, blocks)
    xs = gref.sequence_columns(C, n, ld, L)
    want = gref.sequence_ref(params, xs, n, heads, 0)[0]
    got = gref.sequence_ref(params, xs, n, heads, 0, dtype=torch.float32)[0]
    rep = _util.GradReport(f"fp32 gpt_decode sequence {shape}")
    for p in range(L):
        _check32(rep, f"p={p}", got[p], want[p])
    rep.finish()


@pytest.mark.parametrize("shape", gref.SPIKE_SHAPES, ids=_sid)
def test_fp32_spike_within_bounds(shape):
    C, heads, L = shape
    p = L - 1
    rep = _util.GradReport(f"fp32 gpt_decode spike C={C}")
    for where in gref.spike_wheres(L):
        params, x, kc, vc = gref.spike_case(gref.block_params(C, 1), C, heads, 1, L, p, where)
        want = gref.step(params, x, kc, vc, p, heads, 0)[0]
        got = gref.step(params, x, kc, vc, p, heads, 0, dtype=torch.float32)[0]
        assert bool(torch.isfinite(got).all())
        # the spike really dominates: all the weight of every head is on the spiked key, to ~L e^-60
        assert float(gref.attention_weights(params[0], x, kc[0], p, heads)[:, :, where].min()) > 1 - 1e-12
        _check32(rep, f"where={where}", got, want)
    rep.finish()


# ---------------------------------------------------------------------------------------------
# planner
NO_DEVICE = 100  # hipErrorNoDevice
DOMAIN_L = (1, 63, 64, 65, 1024, 4096, 4097)
DOMAIN_BLOCKS = (1, 8, 64, 65)


def _plan(lib, C, heads, blocks, L):
    out = (ctypes.c_int * 16)()
    rc = lib.pg_gpt_decode_plan(C, heads, blocks, L, out, 16)
    return rc, list(out)


def test_plan_domain_lds_and_offsets(lib):
    """Every point of the stated domain is accepted and everything outside it refused with PG_ESHAPE; LDS stays at or below
    64 KB; the field offsets are disjoint, in order, and cover the block, and the blocks cover the pack."""
    sizes = lambda C: [C, C, 3 * C * C, 3 * C, C * C, C, C, C, 4 * C * C, 4 * C, 4 * C * C, C]  # noqa: E731
    for C in range(4, 261, 4):
        for heads in [h for h in range(1, C + 1) if C % h == 0]:
            for L in DOMAIN_L:
                for blocks in DOMAIN_BLOCKS:
                    rc, out = _plan(lib, C, heads, blocks, L)
                    inside = C <= 256 and L <= 4096 and blocks <= 64
                    assert rc == (0 if inside else -2), (C, heads, blocks, L, rc)
                    if not inside:
                        continue
                    pack, per_block, lds, threads = out[:4]
                    assert 0 < lds <= 64 * 1024 and threads == 256
                    at = 0
                    for off, size in zip(out[4:16], sizes(C)):
                        assert off == at
                        at += size
                    assert at == per_block and pack == blocks * per_block
    assert lib.pg_gpt_decode_plan(64, 3, 1, 10, (ctypes.c_int * 16)(), 16) == -2  # heads must divide C
    assert b"do not divide" in lib.pg_last_error()
    assert lib.pg_gpt_decode_plan(6, 1, 1, 10, (ctypes.c_int * 16)(), 16) == -2   # C % 4
    assert lib.pg_gpt_decode_plan(64, 2, 1, 10, (ctypes.c_int * 16)(), 15) == -1  # short array
    assert lib.pg_gpt_decode_plan(64, 2, 1, 10, None, 16) == -1
    assert lib.pg_gpt_decode_plan(64, 0, 1, 10, (ctypes.c_int * 16)(), 16) == -1


@_no_gpu
def test_what_the_plan_accepts_reaches_the_launch(lib):
    """Fake operands, no device: a launch entry that got past its host side comes back with hipErrorNoDevice. Over the same
    sweep, the launch gets that far exactly where the plan accepts, and refuses with the plan's status where it refuses."""
    keep, ptr = _fake_ptr()
    p = ptr.value
    checked = 0
    for C in range(4, 261, 4):
        for heads in [h for h in range(1, C + 1) if C % h == 0]:
            for L in DOMAIN_L:
                for blocks in DOMAIN_BLOCKS:
                    rc_plan, _ = _plan(lib, C, heads, blocks, L)
                    rc = lib.pg_gpt_decode_step(p, p, p, p, p, 3, C, heads, blocks, L, 16, 0, 0, 1e-5, None, None)
                    if rc_plan == 0:
                        assert _reached_launch(lib, rc), (C, heads, blocks, L, rc, lib.pg_last_error())
                    else:
                        assert rc == rc_plan == -2, (C, heads, blocks, L, rc, rc_plan)
                    checked += 1
    assert checked > 10000
    # argument errors come before the plan and launch nothing either
    assert lib.pg_gpt_decode_step(p, p, p, p, p, 3, 64, 2, 1, 10, 2, 0, 0, 1e-5, None, None) == -1   # ld < N
    assert lib.pg_gpt_decode_step(p, p, p, p, p, 3, 64, 2, 1, 10, 16, 10, 0, 1e-5, None, None) == -1  # p outside
    assert lib.pg_gpt_decode_step(p, p, p, p, p, 3, 64, 2, 1, 10, 16, 0, 2, 1e-5, None, None) == -1   # strict
    assert lib.pg_gpt_decode_step(p, None, p, p, p, 3, 64, 2, 1, 10, 16, 0, 0, 1e-5, None, None) == -1
