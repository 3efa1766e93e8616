"""CPU: tests/_attn_row_ref.py (the float64 restatement of pg_attn_row's contract, csrc/attention_row.hip) is pinned against
the oracle's whole-image attention row by row; the inputs of the GPU tier's large-score case are shown to leave a correct
float32 evaluation inside the bound used there; the planner is swept without a device (what it accepts is what the launch
accepts, among it the whole stated domain); and ops.RowDecode's row / row_dev pair is exercised."""

import ctypes

import pytest
import torch

import _attn_row_ref as aref
import _util
from oracle import ops as oops
from test_host_cpu import _fake_ptr, _no_gpu, _reached_launch

EINVAL, ESHAPE = -1, -2


@pytest.mark.parametrize("hw", [(1, 1), (1, 6), (4, 1), (3, 5)], ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("heads", [1, 2, 3])
@pytest.mark.parametrize("mask_center", [0, 1])
def test_rows_of_the_helper_are_rows_of_the_oracle(mask_center, heads, hw):
    """For every row r, the helper fed with rows < r as cache (garbage from row r on) and row r as input gives row r of
    oracle.ops.causal_attention_core on the whole image, and its cache write is row r of k / v."""
    h, w = hw
    n, dk, dv = 2, 2, 3
    e = heads * dk
    q, kv = (t.double() for t in aref.case((n, heads, dk, dv, h, w), seed=heads))
    want = oops.causal_attention_core(q, kv[:, :e], kv[:, e:], heads, bool(mask_center))
    for r in range(h):
        q_row, kv_row, kc, vc = aref.row_inputs(q, kv, e, r, fill=float("nan"))
        got, kc2, vc2 = aref.attn_row_ref(q_row, kv_row, kc, vc, heads, r, mask_center)
        assert bool(torch.isfinite(got).all())
        assert float((got[:, :, 0] - want[:, :, r]).abs().max()) <= 1e-12, (r, mask_center, heads, hw)
        assert torch.equal(kc2[:, :, r], kv[:, :e, r]) and torch.equal(vc2[:, :, r], kv[:, e:, r])
        assert torch.equal(kc2[:, :, :r], kc[:, :, :r]) and torch.equal(vc2[:, :, :r], vc[:, :, :r])
    if mask_center:  # the first pixel admits nothing
        got = aref.attn_row_ref(*aref.row_inputs(q, kv, e, 0), heads, 0, 1)[0]
        assert float(got[:, :, 0, 0].abs().max()) == 0.0


@pytest.mark.parametrize("where", [(0, 0), (2, 3)])
def test_fp32_evaluation_of_the_spike_case_stays_within_the_bound(where):
    """The large-score inputs are fair: the same statement in float32 is within the GPU tier's bound of float64, the
    scores really are ~80, and a query that admits the spiked key puts all its weight there."""
    shape = (2, 1, 4, 32, 3, 5)
    q, kv = aref.spike_case(shape, where)
    e = 4
    score = (q[0, :, 2, 4] * kv[0, :e, where[0], where[1]]).sum() / 2.0
    assert 70.0 < float(score) < 90.0
    for mask_center in (0, 1):
        for r in range(3):
            args = aref.row_inputs(q, kv, e, r)
            want = aref.attn_row_ref(*args, 1, r, mask_center)[0]
            got = aref.attn_row_ref(*args, 1, r, mask_center, dtype=torch.float32)[0]
            assert bool(torch.isfinite(got).all())
            _util.assert_close(got, want, aref.TOL, f"fp32 spike r={r}")
    r = 2
    want = aref.attn_row_ref(*aref.row_inputs(q, kv, e, r), 1, r, 1)[0]
    v_spike = kv[:, e:, where[0], where[1]].double()
    assert float((want[:, :, 0, 4] - v_spike).abs().max()) < 1e-12


# ---------------------------------------------------------------------------------------------
# planner
def _plan(lib, heads, dk, dv, H, W):
    out = (ctypes.c_int * aref.PLAN_INTS)()
    rc = lib.pg_attn_row_plan(heads, dk, dv, H, W, out, aref.PLAN_INTS)
    return rc, list(out)


DOMAIN_DK = (1, 3, 4, 16, 63, 64, 65)
DOMAIN_DV = (1, 7, 32, 64, 127, 128, 129)
DOMAIN_HW = ((1, 1), (28, 28), (32, 32), (64, 64), (16, 256), (4096, 1), (1, 256), (1, 257), (4097, 1), (65, 64), (17, 241))


def _inside(dk, dv, H, W):
    return dk <= 64 and dv <= 128 and W <= 256 and H * W <= 4096


def test_plan_domain_and_geometry(lib):
    """Every point of the stated domain is accepted, each edge + 1 refused with PG_ESHAPE; the geometry is sane: whole
    waves, LDS within 64 KB, a key tile of whole waves' worth or less, the row covered by the workgroups."""
    seen_in = seen_out = 0
    for heads in (1, 2, 5):
        for dk in DOMAIN_DK:
            for dv in DOMAIN_DV:
                for H, W in DOMAIN_HW:
                    rc, out = _plan(lib, heads, dk, dv, H, W)
                    inside = _inside(dk, dv, H, W)
                    assert rc == (0 if inside else ESHAPE), (heads, dk, dv, H, W, rc, lib.pg_last_error())
                    seen_in += inside
                    seen_out += not inside
                    if not inside:
                        continue
                    threads, lds, tile, gx, gy, qb = out
                    assert threads % 64 == 0 and 0 < threads <= 1024
                    assert 0 < lds <= 64 * 1024
                    assert tile >= 1 and gy == heads
                    assert qb >= 1 and gx * qb >= W and (gx - 1) * qb < W
    assert seen_in > 500 and seen_out > 500
    out = (ctypes.c_int * aref.PLAN_INTS)()
    assert lib.pg_attn_row_plan(1, 4, 32, 28, 28, out, aref.PLAN_INTS - 1) == EINVAL  # short array
    assert lib.pg_attn_row_plan(1, 4, 32, 28, 28, None, aref.PLAN_INTS) == EINVAL
    for bad in ((0, 4, 32, 28, 28), (1, 0, 32, 28, 28), (1, 4, 0, 28, 28), (1, 4, 32, 0, 28), (1, 4, 32, 28, -1)):
        assert lib.pg_attn_row_plan(*bad, out, aref.PLAN_INTS) == EINVAL, bad


def test_supported_asks_the_plan(lib):
    from pytorch_generative_amd import ops

    assert ops.attention_row_supported(1, 4, 32, 28, 28) and ops.attention_row_supported(3, 64, 128, 16, 256)
    assert not ops.attention_row_supported(1, 65, 32, 28, 28) and not ops.attention_row_supported(1, 4, 32, 65, 64)
    assert not ops.attention_row_supported(0, 4, 32, 28, 28)
    plan = ops.attention_row_plan(1, 4, 32, 28, 28)
    rc, out = _plan(lib, 1, 4, 32, 28, 28)
    assert rc == 0 and plan["key_tile"] == out[2] and plan["lds_bytes"] == out[1] and plan["threads"] == out[0]


@_no_gpu
def test_what_the_plan_accepts_reaches_the_launch(lib):
    """Fake operands, no device: a launch entry that got past its host side comes back with hipErrorNoDevice. The launch gets
    that far exactly where the plan accepts, refuses with the plan's status where it refuses, and argument errors come first."""
    keep, ptr = _fake_ptr()
    p = ptr.value
    checked = 0
    for heads in (1, 3):
        for dk in DOMAIN_DK:
            for dv in DOMAIN_DV:
                for H, W in DOMAIN_HW:
                    rc_plan, _ = _plan(lib, heads, dk, dv, H, W)
                    rc = lib.pg_attn_row(p, p, p, p, p, 2, heads, dk, dv, H, W, 0, 1, 1, None, None)
                    if rc_plan == 0:
                        assert _reached_launch(lib, rc), (heads, dk, dv, H, W, rc, lib.pg_last_error())
                    else:
                        assert rc == rc_plan == ESHAPE, (heads, dk, dv, H, W, rc, rc_plan)
                    checked += 1
    assert checked > 1000
    ok = dict(N=2, heads=1, dk=4, dv=32, H=5, W=6, r=0, mask_center=1, write_cache=1)

    def call(ptrs=(p, p, p, p, p), **kw):
        a = dict(ok, **kw)
        return lib.pg_attn_row(*ptrs, a["N"], a["heads"], a["dk"], a["dv"], a["H"], a["W"], a["r"], a["mask_center"],
                               a["write_cache"], None, None)

    assert _reached_launch(lib, call())
    for i in range(5):  # each null pointer
        assert call(ptrs=tuple(None if j == i else p for j in range(5))) == EINVAL
    for bad in (dict(N=0), dict(heads=0), dict(dk=0), dict(dv=-1), dict(H=0), dict(W=0), dict(r=-1), dict(r=5),
                dict(mask_center=2), dict(write_cache=-1), dict(write_cache=2)):
        assert call(**bad) == EINVAL, bad
    assert call(N=65536) == ESHAPE
    # pg_row_gather
    assert _reached_launch(lib, lib.pg_row_gather(p, p, 2, 3, 4, 5, 3, None, None))
    assert lib.pg_row_gather(None, p, 2, 3, 4, 5, 0, None, None) == EINVAL
    assert lib.pg_row_gather(p, None, 2, 3, 4, 5, 0, None, None) == EINVAL
    assert lib.pg_row_gather(p, p, 2, 3, 4, 5, 4, None, None) == EINVAL
    assert lib.pg_row_gather(p, p, 2, 0, 4, 5, 0, None, None) == EINVAL
    del keep


# ---------------------------------------------------------------------------------------------
# ops.RowDecode
def test_row_decode_row_and_row_dev():
    from pytorch_generative_amd import ops

    ctx = ops.RowDecode(7, device="cpu")  # the device scalar lives where it is asked to: the mechanism needs no GPU
    assert ctx.height == 7 and ctx.row == 0 and ctx.commit is False and ctx._row_dev is None
    ctx.row = 3  # no device scalar yet: a plain attribute
    assert ctx.row == 3 and ctx._row_dev is None
    ctx.row, ctx.commit = 4, True  # the form base.sample uses
    assert ctx.row == 4 and ctx.commit is True
    dev = ctx.row_dev  # created on first request, with the current row
    assert dev.dtype == torch.int32 and dev.numel() == 1 and int(dev) == 4
    ctx.row = 6  # from now on every assignment fills it, in place
    assert ctx.row == 6 and int(dev) == 6 and ctx.row_dev is dev
    with ctx as inside:
        assert ops.RowDecode.current is ctx and inside is ctx
    assert ops.RowDecode.current is None
